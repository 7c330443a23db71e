"""Generated cases of fp_mesh_point_distance: a case is dict(name, pos (Nv,3) float32, faces (F,3) int32, points (Q,3) float32) and,
where the answer is known beforehand, expect_face {query: face}.  The host tests run the restatement (tests/mesh_distance_model.py)
over them, the GPU tests hold the kernel to the restatement bit for bit."""
import functools

import numpy as np

import mesh_distance_model as mm

f32 = np.float32
F_SIZES = (1, 2, mm.TILE - 1, mm.TILE, mm.TILE + 1, mm.CHUNK - 1, mm.CHUNK, mm.CHUNK + 1, 3000)
Q_SIZES = (1, 63, 64, 65, 257, 1000)
SCALES = (1e-3, 1.0, 50.0)
# a query per region of the triangle (0,0,0) (1,0,0) (0,1,0), in the order of the walk
REGION_QUERIES = ((-1.0, -1.0, 0.5), (2.0, -0.5, 0.3), (0.5, -1.0, 0.2), (-0.5, 2.0, 0.4), (-1.0, 0.5, 0.1), (1.0, 1.0, 0.1),
                  (0.25, 0.25, 0.7))


def _case(name, pos, faces, points, **kw):
    return dict(name=name, pos=np.ascontiguousarray(np.asarray(pos, np.float64).reshape(-1, 3).astype(f32)),
                faces=np.ascontiguousarray(np.asarray(faces, np.int64).reshape(-1, 3).astype(np.int32)),
                points=np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3).astype(f32)), **kw)


def soup(F, Q, seed, scale=0.1):
    """F random triangles with edges of a few centimetres in a box of 2 * scale, Q queries in and around the box"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (F, 3))
    tri = a[:, None, :] + rng.normal(size=(F, 3, 3)) * 0.2
    pts = rng.uniform(-1.5, 1.5, (Q, 3))
    return _case(f"soup F={F} Q={Q}", tri.reshape(-1, 3) * scale, np.arange(3 * F).reshape(F, 3), pts * scale)


def size_cases():
    """every F of F_SIZES with two of the Q_SIZES, so that every Q comes up three times"""
    out = []
    for i, F in enumerate(F_SIZES):
        for k in range(2):
            Q = Q_SIZES[(2 * i + k) % len(Q_SIZES)]
            out.append(soup(F, Q, 100 + 7 * i + k))
    return out


def region_case(scale):
    """one triangle, a query in each of its seven regions, then one on each vertex, on each edge and in the plane inside"""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    on = [tri[0], tri[1], tri[2], (tri[0] + tri[1]) / 2, (tri[0] + tri[2]) / 2, (tri[1] + tri[2]) / 2, [0.25, 0.5, 0.0]]
    pts = np.concatenate([np.asarray(REGION_QUERIES), np.asarray(on)])
    return _case(f"regions x{scale:g}", tri * scale, [[0, 1, 2]], pts * scale, expect_region=tuple(range(1, 8)))


def tie_case(scale):
    """faces 0 and 1 mirror each other in the plane y = 0 through their shared edge ab (the arithmetic of the two is the same up to
    signs that cancel in every product): the query under the roof is equally far from the interiors of both, the one above the ridge
    has the same closest point on the shared edge in both.  Faces 2, 3, 4 meet in the apex (0, 0, 3), which is vertex a of one, b of
    the next and c of the third: the query above it is answered by the apex in all three.  The smaller index wins every time."""
    pos = [[0, 0, 0], [1, 0, 0], [0.5, 1, -1], [0.5, -1, -1],
           [0, 0, 3], [1, 0, 2], [-0.5, 0.75, 2], [-0.5, -0.75, 2]]
    faces = [[0, 1, 2], [0, 1, 3], [4, 5, 6], [6, 4, 7], [7, 5, 4]]
    pts = [[0.5, 0, -2], [0.5, 0, 1], [0, 0, 4]]
    return _case(f"ties x{scale:g}", np.asarray(pos) * scale, faces, np.asarray(pts) * scale, expect_face={0: 0, 1: 0, 2: 2})


def skipped_case():
    """triangles that never count beside ones that do: a zero-area one (three equal vertices) and a collinear one, a triangle with two equal vertices whose quotient
    is 0/0, a triangle repeated under two indices, vertex indices at Nv, below 0 and at INT32_MAX, a NaN vertex, an infinite vertex; NaN and infinite queries"""
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0],          # 0-2   a plain triangle
           [2, 2, 2], [2, 2, 2], [2, 2, 2],          # 3-5   zero area
           [0, 0, 5], [1, 0, 5], [3, 0, 5],          # 6-8   collinear
           [np.nan, 0, 0], [np.inf, 0, 0], [0, 3, 0],
           [10, 10, 10], [10, 11, 10]]               # 12-13 a = b of face 12: its edge-ab quotient is 0/0 for the query beside it
    faces = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 1, 2], [0, 1, 14], [0, -1, 2], [2**31 - 1, 1, 2], [9, 1, 2], [10, 1, 2], [8, 7, 6],
             [3, 3, 3], [7, 6, 8], [12, 12, 13]]
    pts = [[0.2, 0.2, 1], [10.1, 10.2, 10], [2, 2, 2.5], [2, 2, 2], [2, 1, 5], [1.5, 0, 5], [0.5, 0.5, 5.5], [5, 0, 5], [-1, 0, 5], [np.nan, 0, 0],
           [0, np.inf, 0], [-np.inf, 0, 0], [1e30, 1e30, 1e30], [3, 3, 3]]
    return _case("skipped and degenerate", pos, faces, pts, expect_face={0: 0, 9: -1, 10: -1, 11: -1, 12: -1})


def all_skipped_case():
    pos = [[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [0, 0, 0]]
    faces = [[0, 1, 2], [3, 3, 4], [-1, 3, 3], [0, 3, 3]]
    pts = [[0, 0, 0], [1, 2, 3], [0.5, 0, 0]]
    return _case("every triangle skipped", pos, faces, pts, expect_face={0: -1, 1: -1, 2: -1})


def mesh_cases():
    """the generated meshes of tests/geometry_cases.py with their own vertices (a seeded subset for the soup) and seeded points around
    them as queries"""
    import geometry_cases as gc
    out = []
    for name, m, own in (("box", gc.box(), None), ("l_prism", gc.l_prism(), None), ("crossed_boxes", gc.crossed_boxes(), None),
                         ("sliver_soup", gc.sliver_soup(), 600)):
        rng = np.random.default_rng(len(name))
        v = np.asarray(m.vertices, np.float64)
        q = v if own is None else v[rng.choice(len(v), own, replace=False)]
        lo, hi = v.min(0), v.max(0)
        around = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (300, 3))
        out.append(_case(name, v, m.faces, np.concatenate([q, around])))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = size_cases()
    for s in SCALES:
        out += [region_case(s), tie_case(s)]
    out += [skipped_case(), all_skipped_case()] + mesh_cases()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def references():
    """the restatement's answer for every case, computed once: name -> (dist2, face, closest, region)"""
    return {c["name"]: mm.mesh_point_distance(c["pos"], c["faces"], c["points"], regions=True) for c in all_cases()}
