"""The cases and grids of the uniform-grid tests: every case of tests/mesh_distance_cases.py and of tests/mesh_signed_cases.py under
six grids each, the brute-force restatement's answer for each (shared with the tests that made it), and two cases of this file's own:
`ulp_plane` (a triangle one ulp below a cell plane that the cell function puts above it: what the slack `pad` is for) and `lattice_box`
(a closed box of 4 332 faces with its own surface samples, for the pruning figure).  The host tests run the model
(tests/mesh_grid_model.py) over them; the GPU tests hold the kernels to the same references."""
import functools

import numpy as np

import mesh_distance_cases as mc
import mesh_distance_model as mm
import mesh_grid_model as mg
import mesh_signed_cases as sc

f32 = np.float32
GRIDS = ("default", "1x1x1", "2x3x1", "half box", "tiny cells", "aligned")
TINY_CELLS = 66               # cells along the longest edge of the box under "tiny cells": a flat triangle as long as the box covers
                              # 67 x 67 > kMaxCellsPerTriangle cells, and a query in the middle of a hollow mesh walks some 20 shells
PLANE_QUERIES = 24


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(name, pos, faces, points); the signed cases carry the prefix "signed: " """
    out = {c["name"]: c for c in mc.all_cases()}
    for c in sc.closed_cases():
        out["signed: " + c["name"]] = dict(c, name="signed: " + c["name"])
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the brute-force restatement's (dist2, face, closest) of a case, from the module that already computed it"""
    if name.startswith("signed: "):
        from test_mesh_signed_host import restated
        r = restated(name[len("signed: "):])[3]
        return r["dist2"], r["face"], r["closest"]
    return mc.references()[name][:3]


def _box(pos, faces):
    pos = np.asarray(pos, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(pos))).all(axis=1) if len(faces) else np.zeros(0, bool)
    v = pos[faces[ok]].reshape(-1, 3) if ok.any() else np.zeros((0, 3), f32)
    v = v[np.isfinite(v).all(axis=1)]
    if len(v) == 0:
        return np.zeros(3), np.zeros(3)
    return v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)


def grid_of(pos, faces, kind):
    from foundationpose_amd import ops
    lo, h, n, pad = ops.mesh_grid_shape(pos, faces)
    if kind == "default":
        return mg.Grid(lo, h, n.astype(np.int64), pad)
    blo, bhi = _box(pos, faces)
    ext = bhi - blo
    big = float(ext.max()) if ext.max() > 0 else 1.0
    if kind == "1x1x1":
        return mg.make_grid(blo, big * 1.01, (1, 1, 1))
    if kind == "2x3x1":
        return mg.make_grid(blo, max(float((ext / np.array([2, 3, 1])).max()) * 1.01, big * 1e-3), (2, 3, 1))
    if kind == "half box":                       # the middle half of the box: most triangles clamp into boundary cells
        hh = float(h)
        while True:
            cnt = np.floor(ext / 2 / hh).astype(np.int64) + 1
            if cnt.prod() <= 1 << 21:
                return mg.make_grid(blo + ext / 4, hh, cnt)
            hh *= 1.25
    if kind == "tiny cells":                     # the largest triangles cover more than kMaxCellsPerTriangle cells
        hh = big / TINY_CELLS
        return mg.make_grid(blo, hh, np.floor(ext / hh).astype(np.int64) + 1)
    if kind == "aligned":                        # h a power of two and lo a multiple of it: planes pass through round coordinates
        hh = 2.0 ** np.ceil(np.log2(float(h)))
        while True:
            l0 = (np.floor(blo / hh) - 1) * hh
            cnt = np.ceil((bhi - l0) / hh).astype(np.int64) + 1
            if cnt.prod() <= 1 << 21:
                return mg.make_grid(l0, hh, cnt)
            hh *= 2
    raise KeyError(kind)


def plane_queries(g, points):
    """queries exactly on cell planes: the first finite queries with one coordinate moved onto the plane below or above its cell"""
    points = np.asarray(points, f32).reshape(-1, 3)
    base = points[np.isfinite(points).all(axis=1)][:PLANE_QUERIES]
    out = base.copy()
    for i in range(len(out)):
        k = i % 3
        out[i, k] = mg.plane(g, k, int(mg.cell(g, k, out[i, k])) + (i // 3) % 2)
    return out


@functools.lru_cache(maxsize=None)
def pairs_of(name):
    """(dd, exc) of a case: every pair through the restatement's closest_points, once"""
    c = cases()[name]
    return mg.pair_matrix(c["pos"], c["faces"], c["points"])


@functools.lru_cache(maxsize=None)
def queries(name, kind):
    """a case under a grid: dict(grid, points, ref, extra): under "aligned" the queries are the case's and then PLANE_QUERIES on cell
    planes (`extra` of them), and ref is the brute-force restatement's (dist2, face, closest) for all of them"""
    c = cases()[name]
    g = grid_of(c["pos"], c["faces"], kind)
    points, ref = c["points"], reference(name)
    extra = plane_queries(g, points) if kind == "aligned" else points[:0]
    if len(extra):
        r2 = mm.mesh_point_distance(c["pos"], c["faces"], extra)
        points = np.concatenate([points, extra])
        ref = tuple(np.concatenate([a, b]) for a, b in zip(ref, r2))
    return dict(grid=g, points=np.ascontiguousarray(points), ref=ref, extra=len(extra))


def setup(name, kind):
    """queries(name, kind) with the pair matrices of its queries: dd and exc (mesh_grid_model.pair_matrix)"""
    c, s = cases()[name], dict(queries(name, kind))
    dd, exc = pairs_of(name)
    if s["extra"]:
        d2, e2 = mg.pair_matrix(c["pos"], c["faces"], s["points"][-s["extra"]:])
        dd, exc = np.concatenate([dd, d2]), np.concatenate([exc, e2])
    return dict(s, dd=dd, exc=exc)


def ulp_plane():
    """h = 0.1f, lo = 0: the plane of cell 9 is X = fl(9 * h), yet x, the float32 just below X, already has cell(x) = 9, because
    fl(x * fl(1 / h)) = 9.  Face 1 lies in the plane x = x; the query (X - 0.03, 0, 0) sits in cell 8, m = X - p_x, and face 0, in the
    plane y = -d of cell 8 with d between the query's distances to x and to X, is farther than face 1 but nearer than the plane.
    Without the slack face 1 is stored in cell 9 only, and the walk stops on face 0."""
    g = mg.make_grid((0, 0, 0), f32(0.1), (64, 1, 1))
    X = f32(mg.plane(g, 0, 9))
    x = np.nextafter(X, f32(0))
    px = f32(X - f32(0.03))
    d = f32((float(X - px) + float(x - px)) / 2)
    pos = [[0.81, -d, -1], [0.89, -d, -1], [0.85, -d, 3], [x, -1, -1], [x, 3, -1], [x, -1, 3]]
    return dict(name="ulp_plane", pos=np.asarray(pos, f32), faces=np.asarray([[0, 1, 2], [3, 4, 5]], np.int32),
                points=np.asarray([[px, 0, 0]], f32), grid=g, plane=X, below=x)


@functools.lru_cache(maxsize=None)
def lattice_box(samples=1500, seed=3):
    """geometry_cases.box with 19 x 19 quads a side (4 332 faces, closed) and `samples` samples of its own surface"""
    import geometry_cases as gc
    m = gc.box(n=19)
    pos, faces = np.asarray(m.vertices, f32), np.asarray(m.faces, np.int32)
    pts, _ = mm.sample_surface(pos, faces, samples, seed)
    return dict(name="lattice_box", pos=pos, faces=faces, points=pts)
