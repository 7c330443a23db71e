"""numpy restatement of the uniform grid of include/fp_amd.h (fp_mesh_grid_count, fp_mesh_grid_fill, fp_mesh_grid_point_distance): the
cell of a coordinate, the three classes of a triangle and its cell range, the tables, and the walk with its stop rule, every float
operation one float32 operation in the order the header writes it.  The pair tests themselves are mesh_distance_model's
closest_points: pair_matrix evaluates every (query, triangle) pair once per case, and the walk picks from that matrix, so a pair has
the bits the brute-force restatement gives it.

The walk is restated per shell, not per cell: shell r of the block around cell c visits exactly the stored triangles whose cell range
is at Chebyshev distance r from c (`rmeet`), and a minimum over (dd, face) does not depend on the order inside a shell.  The number of
pair tests counts a triangle once for every cell of its range inside the final block, as the device meets it.  walk_cells is the
literal form over the tables (cell by cell, entry by entry), for small cases: the host tests hold the two to each other.

`wrong=` names a deliberately wrong variant:
  "no_pad"          triangles stored without the slack (pad = 0 in the ranges)
  "plane_c_plus_r"  the high plane at c + r in place of c + r + 1 (the low plane at c - r + 1): under the rule "m > 0" this one is
                    conservative -- it never stops on a plane behind the query -- so it shows in the pair count, not in an answer
  "plane_too_far"   the planes one cell farther out than the block (c + r + 2, c - r - 1): stops too early
  "first_met"       the first-met face kept on a tie (dd < best only), with the entries of a cell reversed
  "no_overflow"     the overflow list ignored
  "drop_outside"    triangles whose range lies outside the grid box dropped rather than clamped into boundary cells"""
import os
import re
from typing import NamedTuple

import numpy as np

import mesh_distance_model as mm

f32 = np.float32
DROPPED, OVERFLOW, STORED = 0, 1, 2
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foundationpose_amd", "csrc", "mesh_grid.h")
MAX_CELLS_PER_TRIANGLE = int(re.search(r"constexpr int kMaxCellsPerTriangle = (\d+);", open(_SRC).read()).group(1))


class Grid(NamedTuple):
    lo: np.ndarray      # (3,) float32
    h: np.float32
    n: np.ndarray       # (3,) int
    pad: np.float32

    @property
    def inv_h(self):
        return f32(1) / f32(self.h)

    @property
    def ncells(self):
        return int(self.n[0]) * int(self.n[1]) * int(self.n[2])


def make_grid(lo, h, n, pad=None):
    lo, h, n = np.asarray(lo, f32).reshape(3), f32(h), np.asarray(n, np.int64).reshape(3)
    M = f32(max(np.abs(lo).max(), np.abs(lo + n.astype(f32) * h).max()))
    return Grid(lo, h, n, f32(2.0 ** -16) * M if pad is None else f32(pad))


def unclamped(g, k, x):
    with np.errstate(all="ignore"):
        return np.floor((np.asarray(x, f32) - g.lo[k]) * g.inv_h)


def cell(g, k, x):
    """clamp(floorf((x - lo_k) * inv_h), 0, n_k - 1), clamped in float32"""
    t = unclamped(g, k, x)
    top = f32(int(g.n[k]) - 1)
    t = np.where(t > 0, t, f32(0))
    t = np.where(t < top, t, top)
    return t.astype(np.int64)


def plane(g, k, i):
    """X = lo_k + (float)i * h: two float32 operations"""
    return g.lo[k] + np.asarray(i).astype(f32) * g.h


def classify(g, pos, faces, wrong=None):
    """-> cls (F,) int8, i0 (F,3), i1 (F,3) int64 (the ranges mean something for STORED only)"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    cls = np.full(F, DROPPED, np.int8)
    i0, i1 = np.zeros((F, 3), np.int64), np.zeros((F, 3), np.int64)
    if F == 0:
        return cls, i0, i1
    ok = ((faces >= 0) & (faces < len(pos))).all(axis=1)
    tri = np.zeros((F, 3, 3), f32)
    tri[ok] = pos[faces[ok]]
    finite = np.isfinite(tri).all(axis=(1, 2))
    pad = f32(0) if wrong == "no_pad" else g.pad
    with np.errstate(all="ignore"):
        tmin, tmax = tri.min(axis=1), tri.max(axis=1)
        outside = np.zeros(F, bool)
        for k in range(3):
            i0[:, k] = cell(g, k, tmin[:, k] - pad)
            i1[:, k] = cell(g, k, tmax[:, k] + pad)
            outside |= (unclamped(g, k, tmax[:, k] + pad) < 0) | (unclamped(g, k, tmin[:, k] - pad) > int(g.n[k]) - 1)
    cells = (i1 - i0 + 1).prod(axis=1)
    cls[ok] = np.where(finite[ok] & (cells[ok] <= MAX_CELLS_PER_TRIANGLE), STORED, OVERFLOW)
    if wrong == "drop_outside":
        cls[ok & finite & outside] = DROPPED
    return cls, i0, i1


def tables(g, pos, faces, wrong=None):
    """-> dict(cls, i0, i1, cell_start (ncells + 1,), entries (ascending inside a cell), overflow (ascending), n_entries, n_overflow)"""
    cls, i0, i1 = classify(g, pos, faces, wrong)
    st = np.nonzero(cls == STORED)[0]
    ext = (i1[st] - i0[st] + 1)
    per = ext.prod(axis=1)
    total = int(per.sum())
    owner = np.repeat(np.arange(len(st)), per)
    local = np.arange(total) - np.repeat(np.cumsum(per) - per, per)
    x = i0[st][owner, 0] + local % ext[owner, 0]
    y = i0[st][owner, 1] + (local // ext[owner, 0]) % ext[owner, 1]
    z = i0[st][owner, 2] + local // (ext[owner, 0] * ext[owner, 1])
    lin = (z * int(g.n[1]) + y) * int(g.n[0]) + x
    order = np.lexsort((st[owner], lin))
    counts = np.bincount(lin, minlength=g.ncells)
    cell_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    overflow = np.nonzero(cls == OVERFLOW)[0].astype(np.int32)
    return dict(cls=cls, i0=i0, i1=i1, cell_start=cell_start, entries=st[owner][order].astype(np.int32), overflow=overflow,
                n_entries=total, n_overflow=len(overflow))


def pair_matrix(pos, faces, points, block=1 << 21):
    """every pair once -> dd (Q,F) float32, +inf where the pair does not count, and exc (Q,F) float32: how far the computed q lies
    outside its triangle's bounding box, the largest over the axes (0 inside; 0 where the pair does not count)"""
    points = np.asarray(points, f32).reshape(-1, 3)
    tri = mm.face_vertices(pos, faces)
    Q, F = len(points), len(tri)
    dd, exc = np.full((Q, F), np.inf, f32), np.zeros((Q, F), f32)
    if Q == 0 or F == 0:
        return dd, exc
    p = tuple(points[:, k][:, None] for k in range(3))
    step = max(1, block // Q)
    with np.errstate(all="ignore"):
        for f0 in range(0, F, step):
            t = tri[f0:f0 + step]
            a, b, c = (tuple(t[:, j, k][None, :] for k in range(3)) for j in range(3))
            q, d, _ = mm.closest_points(p, a, b, c)
            counts = d <= mm.FLT_MAX
            dd[:, f0:f0 + step] = np.where(counts, d, f32(np.inf))
            e = np.zeros(d.shape, f32)
            for k in range(3):
                tmin, tmax = t[:, :, k].min(axis=1)[None, :], t[:, :, k].max(axis=1)[None, :]
                e = np.maximum(e, np.where(counts, np.maximum(tmin - q[k], q[k] - tmax), f32(0)))
            exc[:, f0:f0 + step] = np.where(np.isnan(e), f32(np.inf), e)
    return dd, exc


def _take(best, face, cand, ids, rows, first_met=False):
    """merge the candidates cand (n, m) of faces ids (m,), ascending, into best / face at rows"""
    if cand.shape[1] == 0:
        return
    if first_met:                                     # entries reversed: the larger index of equals is met first, and then kept
        j = cand.shape[1] - 1 - np.argmin(cand[:, ::-1], axis=1)
    else:
        j = np.argmin(cand, axis=1)                   # the first of equal minima: the smaller face
    v, f = cand[np.arange(len(rows)), j], ids[j]
    better = v < best[rows]
    if not first_met:
        better |= (v == best[rows]) & (f < face[rows])
    better &= v <= mm.FLT_MAX
    best[rows] = np.where(better, v, best[rows])
    face[rows] = np.where(better, f, face[rows])


def stop_distance(g, c, p, r, wrong=None):
    """m of the stop rule for queries p (n,3) in cells c (n,3) after shell r -> (any side left (n,), m (n,) float32)"""
    up, down = (0, 1) if wrong == "plane_c_plus_r" else (2, -1) if wrong == "plane_too_far" else (1, 0)
    side = np.zeros(len(c), bool)
    m = np.full(len(c), np.inf, f32)
    with np.errstate(all="ignore"):
        for k in range(3):
            hi = c[:, k] + r < int(g.n[k]) - 1
            lo = c[:, k] - r > 0
            mh = plane(g, k, c[:, k] + r + up) - p[:, k]
            ml = p[:, k] - plane(g, k, c[:, k] - r + down)
            m = np.where(hi & (mh < m), mh, m)
            m = np.where(lo & (ml < m), ml, m)
            side |= hi | lo
    return side, m


def walk(g, tab, dd, points, wrong=None):
    """-> best (Q,) float32, face (Q,) int32, pairs_tested (Q,) int64, shells (Q,) int64 (the last shell visited; -1 without a walk)"""
    points = np.asarray(points, f32).reshape(-1, 3)
    Q = len(points)
    best, face = np.full(Q, np.inf, f32), np.full(Q, -1, np.int64)
    pairs, shells = np.zeros(Q, np.int64), np.full(Q, -1, np.int64)
    walks = np.isfinite(points).all(axis=1)
    st = np.nonzero(tab["cls"] == STORED)[0]
    ov = np.nonzero(tab["cls"] == OVERFLOW)[0]
    c = np.stack([cell(g, k, np.where(walks, points[:, k], f32(0))) for k in range(3)], axis=1)
    i0, i1 = tab["i0"][st], tab["i1"][st]
    rmeet = np.zeros((Q, len(st)), np.int64)
    for k in range(3):
        rmeet = np.maximum(rmeet, np.maximum(i0[None, :, k] - c[:, None, k], c[:, None, k] - i1[None, :, k]))
    dds = dd[:, st]
    active = walks.copy()
    r = 0
    while active.any():
        rows = np.nonzero(active)[0]
        _take(best, face, np.where(rmeet[rows] == r, dds[rows], f32(np.inf)), st, rows, wrong == "first_met")
        side, m = stop_distance(g, c[rows], points[rows], r, wrong)
        with np.errstate(all="ignore"):
            stop = ~side | ((m > 0) & (best[rows] < m * m))
        shells[rows[stop]] = r
        active[rows[stop]] = False
        r += 1
    # a stored triangle is tested once for every cell of its range inside the final block
    R = np.maximum(shells, 0)
    met = np.ones((Q, len(st)), np.int64)
    for k in range(3):
        a = np.maximum(i0[None, :, k], (c[:, k] - R)[:, None])
        b = np.minimum(i1[None, :, k], (c[:, k] + R)[:, None])
        met *= np.maximum(b - a + 1, 0)
    pairs[walks] = met[walks].sum(axis=1)
    if wrong != "no_overflow" and len(ov):
        rows = np.nonzero(walks)[0]
        _take(best, face, dd[np.ix_(rows, ov)], ov, rows, wrong == "first_met")
        pairs[walks] += len(ov)
    return best, face.astype(np.int32), pairs, shells


def walk_cells(g, tab, dd, points):
    """the literal walk of one query after another over the tables: cell by cell, entry by entry (small cases)"""
    points = np.asarray(points, f32).reshape(-1, 3)
    Q = len(points)
    best, face, pairs = np.full(Q, np.inf, f32), np.full(Q, -1, np.int32), np.zeros(Q, np.int64)
    n = [int(x) for x in g.n]
    for i in range(Q):
        p = points[i]
        if not np.isfinite(p).all():
            continue
        c = [int(cell(g, k, p[k])) for k in range(3)]
        b, bf = f32(np.inf), -1
        r = 0
        while True:
            for z in range(max(c[2] - r, 0), min(c[2] + r, n[2] - 1) + 1):
                for y in range(max(c[1] - r, 0), min(c[1] + r, n[1] - 1) + 1):
                    for x in range(max(c[0] - r, 0), min(c[0] + r, n[0] - 1) + 1):
                        if max(abs(x - c[0]), abs(y - c[1]), abs(z - c[2])) != r:
                            continue
                        lin = (z * n[1] + y) * n[0] + x
                        for f in tab["entries"][tab["cell_start"][lin]:tab["cell_start"][lin + 1]]:
                            d = dd[i, f]
                            pairs[i] += 1
                            if d < b or (d == b and f < bf):
                                b, bf = d, int(f)
            side, m = stop_distance(g, np.asarray([c]), p[None], r)
            with np.errstate(all="ignore"):
                if not side[0] or (m[0] > 0 and b < m[0] * m[0]):
                    break
            r += 1
        for f in tab["overflow"]:
            d = dd[i, f]
            pairs[i] += 1
            if d < b or (d == b and f < bf):
                b, bf = d, int(f)
        best[i], face[i] = b, bf
    return best, face, pairs


def closest_of(pos, faces, points, face):
    """the finish: q recomputed for the winning face with the same walk; zeros without an answer"""
    points = np.asarray(points, f32).reshape(-1, 3)
    tri = mm.face_vertices(pos, faces)
    out = np.zeros((len(points), 3), f32)
    has = face >= 0
    if has.any():
        t = tri[face[has]]
        a, b, c = (tuple(t[:, j, k] for k in range(3)) for j in range(3))
        q, _, _ = mm.closest_points(tuple(points[has][:, k] for k in range(3)), a, b, c)
        out[has] = np.stack(q, axis=1)
    return out


def mesh_grid_point_distance(pos, faces, points, g, wrong=None, dd=None):
    """-> (dist2 (Q,) float32, face (Q,) int32, closest (Q,3) float32, pairs_tested (Q,) int64), tables"""
    if dd is None:
        dd, _ = pair_matrix(pos, faces, points)
    tab = tables(g, pos, faces, wrong)
    best, face, pairs, _ = walk(g, tab, dd, points, wrong)
    return (best, face, closest_of(pos, faces, points, face), pairs), tab
