"""Writes tsdf_tables.h: the six Kuhn tetrahedra of a cube and the 16 cases of marching tetrahedra (fp_tsdf_count_triangles /
fp_tsdf_emit_triangles, include/fp_amd.h).  `python3 gen_tsdf_tables.py` rewrites the header next to this file; the header is
committed, and tests/test_tsdf_host.py compares it with the table the numpy restatement derives on its own.

A tetrahedron's corners are 0..3; bit k of a case is set when corner k is inside (tsdf < 0).  A triangle is three tetrahedron edges
(i, j), i < j, each packed as i * 4 + j; its corners lie on them.  The winding is the one for a tetrahedron with
det(p1 - p0, p2 - p0, p3 - p0) > 0 (an even permutation of the axes): (v1 - v0) x (v2 - v0) points from the inside corners to the
outside ones.  An odd permutation mirrors the tetrahedron, and the kernels swap v1 and v2 for it."""
import itertools
import os

import numpy as np

PERMS = list(itertools.permutations(range(3)))          # lexicographic: (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0)


def perm_odd(p):
    return sum(p[i] > p[j] for i in range(3) for j in range(i + 1, 3)) % 2


def tet_corners(p):
    """the (4,3) offsets (dx, dy, dz) of the corners of the tetrahedron of axis permutation p: 0, e_a, e_a + e_b, e_a + e_b + e_c"""
    c = np.zeros((4, 3), dtype=np.int64)
    for k, axis in enumerate(p):
        c[k + 1:, axis] += 1
    return c


def case_table():
    """[(edge, edge, edge), ...] per case 0..15, wound for the even tetrahedron (0,1,2)"""
    P = tet_corners((0, 1, 2)).astype(np.float64)
    table = []
    for case in range(16):
        ins = [k for k in range(4) if case >> k & 1]
        out = [k for k in range(4) if not case >> k & 1]
        if len(ins) in (0, 4):
            table.append([])
            continue
        if len(ins) == 1:
            tris = [[(ins[0], o) for o in out]]
        elif len(ins) == 3:
            tris = [[(i, out[0]) for i in ins]]
        else:
            (i, j), (k, l) = ins, out
            quad = [(i, k), (i, l), (j, l), (j, k)]
            tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
        outward = P[out].mean(0) - P[ins].mean(0)
        fixed = []
        for t in tris:
            v = [(P[a] + P[b]) / 2 for a, b in t]
            if np.dot(np.cross(v[1] - v[0], v[2] - v[0]), outward) < 0:
                t = [t[0], t[2], t[1]]
            fixed.append(tuple(tuple(sorted(e)) for e in t))
        table.append(fixed)
    return table


def header_text():
    rows = []
    for case, tris in enumerate(case_table()):
        codes = [a * 4 + b for t in tris for a, b in t] + [0] * (6 - 3 * len(tris))
        rows.append("  {%d, {%s}},   // case %2d" % (len(tris), ", ".join("%2d" % c for c in codes), case))
    corners = []
    for p in PERMS:
        c = tet_corners(p)
        corners.append("  {{%s}, %d},   // axes %s" % (", ".join("{%d, %d, %d}" % tuple(r) for r in c), perm_odd(p), p))
    return ("// Written by gen_tsdf_tables.py -- do not edit.  Marching tetrahedra over the six Kuhn tetrahedra of a cube.\n"
            "#pragma once\n"
            "struct TsdfCase { int n; int e[6]; };            // n triangles; e[3 * t + k] = i * 4 + j: the tetrahedron edge (i, j), i < j\n"
            "struct TsdfTet { int c[4][3]; int odd; };        // corner offsets (dx, dy, dz); odd: swap v1 and v2 of every triangle\n"
            "static __constant__ const TsdfCase kTsdfCases[16] = {\n" + "\n".join(rows) + "\n};\n"
            "static __constant__ const TsdfTet kTsdfTets[6] = {\n" + "\n".join(corners) + "\n};\n")


if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tsdf_tables.h"), "w") as f:
        f.write(header_text())
