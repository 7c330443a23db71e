"""Generated cases of fp_mesh_ray_cast: a case is dict(name, pos (Nv,3) float32, faces (F,3) int32, origins (R,3) float32, dirs (R,3)
float32, t_min, t_max, cull) and, where the answer is known beforehand, expect_face {ray: face} and expect_t {ray: t}.  The host
tests run the restatement (tests/mesh_ray_model.py) over them, the GPU tests hold the kernel to the restatement bit for bit."""
import functools

import numpy as np

import mesh_distance_model as mm
import mesh_ray_model as rm

f32 = np.float32
F_SIZES = (1, 2, mm.TILE - 1, mm.TILE, mm.TILE + 1, mm.CHUNK - 1, mm.CHUNK, mm.CHUNK + 1, 3000)
R_SIZES = (1, 63, 64, 65, 257, 1000)
SCALES = (1e-3, 1.0, 50.0)
INF = float("inf")


def _case(name, pos, faces, origins, dirs, t_min=0.0, t_max=INF, cull=0, **kw):
    arr = lambda x, dt: np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, 3).astype(dt))     # noqa: E731
    return dict(name=name, pos=arr(pos, f32), faces=np.ascontiguousarray(np.asarray(faces, np.int64).reshape(-1, 3).astype(np.int32)),
                origins=arr(origins, f32), dirs=arr(dirs, f32), t_min=float(t_min), t_max=float(t_max), cull=int(cull), **kw)


def soup(F, R, seed, scale=1.0, tag=""):
    """F random triangles in a box of 2 * scale (mesh_distance_cases.soup's, with edges of half the length: the share of rays that
    pass within 1e-4, in barycentrics, of some triangle's edge line grows with the triangles' size, and the host test wants it under a
    tenth at 3000 faces; most rays still hit several triangles), R rays from the sphere of three box radii towards random points of
    the box; the directions are not unit vectors"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (F, 3))
    tri = a[:, None, :] + rng.normal(size=(F, 3, 3)) * 0.1
    u = rng.normal(size=(R, 3))
    o = 3.0 * np.sqrt(3.0) * u / np.linalg.norm(u, axis=1, keepdims=True)
    target = rng.uniform(-1, 1, (R, 3))
    d = (target - o) * rng.uniform(0.25, 4.0, (R, 1))
    return _case(f"soup F={F} R={R} x{scale:g}{tag}", tri.reshape(-1, 3) * scale, np.arange(3 * F).reshape(F, 3), o * scale, d * scale)


def size_cases():
    """every F of F_SIZES with two of the R_SIZES, so that every R comes up three times; the scales in turn"""
    out = []
    for i, F in enumerate(F_SIZES):
        for k in range(2):
            out.append(soup(F, R_SIZES[(2 * i + k) % len(R_SIZES)], 300 + 7 * i + k, SCALES[(2 * i + k) % len(SCALES)]))
    return out + list(margin_soups())


def margin_soups():
    """the 3000-face soup with 1000 rays at each scale: what the host test measures the float64 margins on"""
    return tuple(soup(3000, 1000, 400 + k, s, " (margins)") for k, s in enumerate(SCALES))


def tie_case():
    """small-integer coordinates: every product and sum is exact, so a ray through an edge or a vertex that faces share hits each of
    them with U, V or U + V exactly on the boundary and the same t: the smaller face answers.  Faces 0 and 1 share the edge (1,0,0)
    (0,1,0) (listed in both orders, as two windings); faces 2..5 are a fan around the vertex (4,4,0)."""
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0],
           [4, 4, 0], [6, 4, 0], [4, 6, 0], [2, 4, 0], [4, 2, 0]]
    faces = [[0, 1, 2], [3, 2, 1], [4, 5, 6], [4, 6, 7], [4, 7, 8], [4, 8, 5]]
    origins = [[0.5, 0.5, 2], [0.25, 0.75, -4], [4, 4, 8], [4, 4, -8], [0.5, 0.5, 2]]
    dirs = [[0, 0, -1], [0, 0, 2], [0, 0, -2], [0, 0, 1], [0, 0, -1]]
    return _case("ties on a shared edge and a shared vertex", pos, faces, origins, dirs,
                 expect_face={0: 0, 1: 0, 2: 2, 3: 2, 4: 0}, expect_t={0: 2.0, 1: 2.0, 2: 4.0, 3: 8.0})


def degenerate_case():
    """a ray in a triangle's plane (det == 0), a zero-area triangle, a zero direction: none answers; the plain triangle beside them
    does"""
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0],          # 0-2  a plain triangle in z = 0
           [2, 2, 2], [2, 2, 2], [2, 2, 2],          # 3-5  three equal vertices
           [0, 0, 5], [1, 0, 5], [3, 0, 5]]          # 6-8  collinear
    faces = [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    origins = [[-1, 0.25, 0], [0.25, 0.25, 1], [2, 2, 3], [1.5, 0, 6], [0.25, 0.25, 1], [0.25, 0.25, 0]]
    dirs = [[1, 0, 0], [0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, 0], [0, 0, 0]]
    return _case("in-plane ray, zero-area faces, zero direction", pos, faces, origins, dirs,
                 expect_face={0: -1, 1: 0, 2: -1, 3: -1, 4: -1, 5: -1})


def origin_on_triangle_case():
    """origins on the triangle: t = 0 is a hit (t_min = 0 is inclusive) and is recorded as +0.  Ray 1 leaves against the normal
    (det > 0, tn = +0); rays 0 and 2 leave along it (det < 0: T = -tn = -0 and the raw quotient is -0).  Ray 3 starts just behind the plane and
    runs away from it: t < 0, no hit."""
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    origins = [[0.25, 0.25, 0], [0.25, 0.5, 0], [0.5, 0.25, 0], [0.25, 0.25, -0.5]]
    dirs = [[0, 0, 1], [0, 0, -1], [1, 1, 1], [0, 0, -1]]
    return _case("origin on the triangle", pos, [[0, 1, 2]], origins, dirs, expect_face={0: 0, 1: 0, 2: 0, 3: -1},
                 expect_t={0: 0.0, 1: 0.0, 2: 0.0})


def range_cases():
    """power-of-two geometry: the hit is at t = 4 exactly.  t_min = 4 and t_max = 4 both keep it (inclusive); the next float32 above /
    below drops it"""
    pos = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
    o, d = [[1, 1, 8]], [[0, 0, -2]]
    up, down = float(np.nextafter(f32(4), f32(8))), float(np.nextafter(f32(4), f32(0)))
    return [_case("hit exactly at t_min", pos, [[0, 1, 2]], o, d, t_min=4.0, expect_face={0: 0}, expect_t={0: 4.0}),
            _case("hit exactly at t_max", pos, [[0, 1, 2]], o, d, t_max=4.0, expect_face={0: 0}, expect_t={0: 4.0}),
            _case("hit exactly at t_min = t_max", pos, [[0, 1, 2]], o, d, t_min=4.0, t_max=4.0, expect_face={0: 0}),
            _case("hit just below t_min", pos, [[0, 1, 2]], o, d, t_min=up, expect_face={0: -1}),
            _case("hit just above t_max", pos, [[0, 1, 2]], o, d, t_max=down, expect_face={0: -1})]


def cull_cases():
    """the same triangle under both windings, at z = 0 (face 0, normal +z) and z = 1 (face 1, normal -z); a ray down and a ray up
    through both.  none: the first met; back (1): only the face whose normal the ray runs against; front (2): the other"""
    pos = [[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 1], [4, 0, 1], [0, 4, 1]]
    faces = [[0, 1, 2], [3, 5, 4]]
    origins, dirs = [[1, 1, 3], [1, 1, -2]], [[0, 0, -1], [0, 0, 1]]
    expect = {0: {0: 1, 1: 0}, 1: {0: 0, 1: 1}, 2: {0: 1, 1: 0}}
    return [_case(f"cull={c} on a two-sided pair", pos, faces, origins, dirs, cull=c, expect_face=expect[c]) for c in (0, 1, 2)]


def skipped_case():
    """triangles that never answer in front of one that does: a NaN vertex, an infinite vertex, an index of -1, an index of Nv; the
    plain triangle behind them answers every ray"""
    pos = [[0, 0, 0], [4, 0, 0], [0, 4, 0], [np.nan, 0, 1], [np.inf, 0, 1], [0, 0, 1], [4, 0, 1], [0, 4, 1]]
    faces = [[3, 6, 7], [4, 6, 7], [5, -1, 7], [5, 6, 8], [0, 1, 2]]
    origins = [[1, 1, 3], [0.5, 2, 3], [1, 1, -3]]
    dirs = [[0, 0, -1], [0, 0, -0.5], [0, 0, 1]]
    return _case("skipped triangles", pos, faces, origins, dirs, expect_face={0: 4, 1: 4, 2: 4}, expect_t={0: 3.0, 1: 6.0, 2: 3.0})


def all_skipped_case():
    pos = [[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [0, 0, 0]]
    faces = [[0, 1, 2], [3, 3, 4], [-1, 3, 3], [0, 3, 3]]
    return _case("nothing answers", pos, faces, [[0, 0, 1], [1, 2, 3]], [[0, 0, -1], [0, 0, -1]], expect_face={0: -1, 1: -1})


def non_finite_ray_case():
    pos = [[-4, -4, 0], [4, -4, 0], [0, 4, 0]]
    origins = [[0, 0, 1], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, 1], [0, 0, 1], [0, 0, -np.inf], [0, 0, 1]]
    dirs = [[0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, np.nan], [0, 0, -np.inf], [0, 0, 1], [np.inf, 0, -1]]
    return _case("non-finite rays", pos, [[0, 1, 2]], origins, dirs, expect_face={0: 0, 1: -1, 2: -1, 3: -1, 4: -1, 5: -1, 6: -1})


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(size_cases() + [tie_case(), degenerate_case(), origin_on_triangle_case()] + range_cases() + cull_cases()
                 + [skipped_case(), all_skipped_case(), non_finite_ray_case()])


def cast(c, **kw):
    return rm.mesh_ray_cast(c["pos"], c["faces"], c["origins"], c["dirs"], c["t_min"], c["t_max"], c["cull"], **kw)


@functools.lru_cache(maxsize=None)
def references():
    """the restatement's answer for every case, computed once: name -> (t, face, bary, hit)"""
    return {c["name"]: cast(c) for c in all_cases()}


# ------------------------------------------------------------------ the two parallel squares of the visibility tests
def two_squares():
    """a blocker [0,1]^2 at z = 1 over a receiver [-2,2]^2 at z = 0, power-of-two coordinates, and an eye at (0.5, 0.5, 2): the
    blocker's shadow on the receiver is (-0.5, 1.5)^2, its diagonal's the line y = x -> (pos, faces: 0-1 the blocker, 2-3 the
    receiver; receiver alone (pos, faces); eye)"""
    pos = np.array([[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1], [-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], f32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    return pos, faces, (pos[4:], faces[2:] - 4), np.array([[0.5, 0.5, 2.0]], f32)
