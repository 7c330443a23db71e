"""numpy restatement of fp_mesh_point_distance (include/fp_amd.h): the exact distance from points to a triangle mesh, operation for
operation in float32 -- the region walk of Ericson 5.1.5 on whole arrays, every difference, product and quotient one float32
operation, dot(x, y) = (x0*y0 + x1*y1) + x2*y2, the answer the smallest (dd, face).  Also the numpy stand-ins of
reconstruct.sample_surface and reconstruct.compare_meshes, and an independent float64 formulation of the distance for the host tests.

`wrong=` names a deliberately wrong variant (the host tests show that the bit-equality gate tells each from the definition):
  "strict"       the edge-ab test with vc < 0 where the book has vc <= 0 (a query over the edge's line falls through; a triangle
                 with a = b, whose edge-ab quotient is 0/0, is answered by a later region)
  "no_edge_bc"   the edge-bc region left out (its queries fall through to the interior formula)
  "larger_index" equal distances go to the larger face index
  "contracted"   dot products evaluated with one rounding (what a fused multiply-add chain approaches)
  "degenerate_a" a triangle whose quotient is 0/0 answered by its vertex a instead of being skipped"""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def _kernel_constant(name):
    """an integer constexpr of csrc/mesh_distance.hip, read from the source: the cases' sizes follow the kernel's tiles"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foundationpose_amd", "csrc", "mesh_distance.hip")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


TILE = _kernel_constant("kTile")           # triangles per LDS tile
CHUNK = _kernel_constant("kChunkMin")      # the fewest faces a workgroup scans; with one tile of queries the chunk is exactly this
REGIONS = ("vertex a", "vertex b", "edge ab", "vertex c", "edge ac", "edge bc", "interior")


def _dot(x, y, wrong=None):
    if wrong == "contracted":
        return (x[0].astype(np.float64) * y[0] + x[1].astype(np.float64) * y[1] + x[2].astype(np.float64) * y[2]).astype(f32)
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def closest_points(p, a, b, c, wrong=None):
    """p, a, b, c: tuples of three float32 arrays (x, y, z) that broadcast against each other -> (q tuple, dd, region 1..7)"""
    with np.errstate(all="ignore"):
        sub = lambda x, y: tuple(x[k] - y[k] for k in range(3))     # noqa: E731
        ab, ac, ap = sub(b, a), sub(c, a), sub(p, a)
        d1, d2 = _dot(ab, ap, wrong), _dot(ac, ap, wrong)
        bp = sub(p, b)
        d3, d4 = _dot(ab, bp, wrong), _dot(ac, bp, wrong)
        cp = sub(p, c)
        d5, d6 = _dot(ab, cp, wrong), _dot(ac, cp, wrong)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        zero = f32(0)
        t3 = (vc < zero) if wrong == "strict" else (vc <= zero)
        tests = [(d1 <= zero) & (d2 <= zero), (d3 >= zero) & (d4 <= d3), t3 & (d1 >= zero) & (d3 <= zero), (d6 >= zero) & (d5 <= d6),
                 (vb <= zero) & (d2 >= zero) & (d6 <= zero), (va <= zero) & (e >= zero) & (g >= zero)]
        if wrong == "no_edge_bc":
            tests[5] = np.zeros_like(tests[5])
        region = np.full(np.broadcast(d1, d6).shape, 7, np.int8)
        for k in range(5, -1, -1):                       # the first test that holds wins
            region = np.where(tests[k], np.int8(k + 1), region)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e / (e + g)
        denom = f32(1) / ((va + vb) + vc)
        v_in, w_in = vb * denom, vc * denom
        bc = sub(c, b)
        q = []
        for k in range(3):
            q_ab = a[k] + v_ab * ab[k]
            q_ac = a[k] + w_ac * ac[k]
            q_bc = b[k] + w_bc * bc[k]
            q_in = (a[k] + v_in * ab[k]) + w_in * ac[k]
            q.append(np.select([region == 1, region == 2, region == 3, region == 4, region == 5, region == 6],
                               [np.broadcast_to(a[k], region.shape), np.broadcast_to(b[k], region.shape), q_ab,
                                np.broadcast_to(c[k], region.shape), q_ac, q_bc], q_in).astype(f32))
        d = sub(p, tuple(q))
        dd = _dot(d, d, wrong)
        if wrong == "degenerate_a":
            zz = np.isnan(dd) & ~(np.isnan(a[0] + a[1] + a[2] + b[0] + b[1] + b[2] + c[0] + c[1] + c[2]) | np.isnan(p[0] + p[1] + p[2]))
            da = _dot(ap, ap)
            q = [np.where(zz, np.broadcast_to(a[k], region.shape), q[k]) for k in range(3)]
            dd = np.where(zz, da, dd)
        return tuple(q), dd, region


def face_vertices(pos, faces):
    """(F,3,3) float32 vertices of the faces, NaN for a face with an index outside 0..Nv-1"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(pos))).all(axis=1)
    tri = np.full((len(faces), 3, 3), np.nan, f32)
    if ok.any():
        tri[ok] = pos[faces[ok]]
    return tri


def mesh_point_distance(pos, faces, points, wrong=None, regions=False, block=1 << 22):
    """-> dist2 (Q,) float32, face (Q,) int32, closest (Q,3) float32 [, region (Q,) int8 of the winning face, 0 without one]"""
    points = np.asarray(points, f32).reshape(-1, 3)
    tri = face_vertices(pos, faces)
    Q, F = len(points), len(tri)
    best = np.full(Q, np.inf, f32)
    face = np.full(Q, -1, np.int32)
    closest = np.zeros((Q, 3), f32)
    reg = np.zeros(Q, np.int8)
    if Q == 0 or F == 0:
        return (best, face, closest, reg) if regions else (best, face, closest)
    step = max(1, block // Q)
    p = tuple(points[:, k][:, None] for k in range(3))
    rows = np.arange(Q)
    for f0 in range(0, F, step):
        t = tri[f0:f0 + step]
        a, b, c = (tuple(t[:, j, k][None, :] for k in range(3)) for j in range(3))
        q, dd, region = closest_points(p, a, b, c, wrong)
        dd = np.where(dd <= FLT_MAX, dd, f32(np.inf))            # what does not count (NaN, overflow) never wins
        if wrong == "larger_index":
            j = dd.shape[1] - 1 - np.argmin(dd[:, ::-1], axis=1)
            better = dd[rows, j] <= best
        else:
            j = np.argmin(dd, axis=1)                             # the first of equal minima: the smaller face
            better = dd[rows, j] < best
        better &= dd[rows, j] <= FLT_MAX
        best = np.where(better, dd[rows, j], best)
        face = np.where(better, (f0 + j).astype(np.int32), face)
        for k in range(3):
            closest[:, k] = np.where(better, q[k][rows, j], closest[:, k])
        reg = np.where(better, region[rows, j], reg)
    return (best, face, closest, reg) if regions else (best, face, closest)


# ------------------------------------------------------------------ an independent float64 formulation
def _segment_d2(p, a, b):
    ab = b - a
    L = np.einsum("...k,...k->...", ab, ab)
    with np.errstate(all="ignore"):
        t = np.where(L > 0, np.einsum("...k,...k->...", p - a, ab) / L, 0.0)
    t = np.clip(t, 0.0, 1.0)
    d = p - (a + t[..., None] * ab)
    return np.einsum("...k,...k->...", d, d)


def distance2_float64(points, tri):
    """squared distance of points (Q,3) to triangles (F,3,3) in float64, as the minimum over the plane projection where it falls inside
    the triangle and the three segment distances -> (Q,F).  Not the region walk: nothing is shared with the restatement."""
    p = np.asarray(points, np.float64)[:, None, :]
    a, b, c = (np.asarray(tri, np.float64)[None, :, j, :] for j in range(3))
    out = np.minimum(np.minimum(_segment_d2(p, a, b), _segment_d2(p, b, c)), _segment_d2(p, c, a))
    n = np.cross(b - a, c - a)
    nn = np.einsum("...k,...k->...", n, n)
    with np.errstate(all="ignore"):
        h = np.einsum("...k,...k->...", p - a, n)
        proj = p - (h / nn)[..., None] * n
        inside = np.broadcast_to(nn > 0, h.shape)
        for u, v in ((a, b), (b, c), (c, a)):
            inside = inside & (np.einsum("...k,...k->...", np.cross(v - u, proj - u), n) >= 0)
        plane = np.where(inside, h * h / nn, np.inf)
    return np.minimum(out, plane)


# ------------------------------------------------------------------ stand-ins of reconstruct.sample_surface / compare_meshes
def sample_surface(pos, faces, n, seed=0):
    """numpy stand-in of reconstruct.sample_surface -> (points (n,3) float32, face (n,) int64)"""
    from foundationpose_amd.reconstruct import _surface_strata
    pos = np.asarray(pos, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cum, target, w = _surface_strata(pos, faces, n, seed)
    f = np.searchsorted(cum, target, side="right")
    f = np.minimum(f, len(faces) - 1)
    a, b, c = pos[faces[f, 0]], pos[faces[f, 1]], pos[faces[f, 2]]
    return ((a * w[:, 0:1] + b * w[:, 1:2]) + c * w[:, 2:3]).astype(f32), f


def compare_meshes(a, b, samples, thresholds, seed=0, wrong=None):
    """numpy stand-in of reconstruct.compare_meshes on (pos, faces) pairs: the restatement's distances and ops.MeshComparison's own
    statistics -> ops.MeshComparison with numpy distance arrays"""
    from foundationpose_amd import ops
    pa, _ = sample_surface(a[0], a[1], samples, seed)
    pb, _ = sample_surface(b[0], b[1], samples, seed)
    d_ab = np.sqrt(mesh_point_distance(b[0], b[1], pa, wrong)[0])
    d_ba = np.sqrt(mesh_point_distance(a[0], a[1], pb, wrong)[0])
    return ops.MeshComparison.from_distances(d_ab, d_ba, thresholds)
