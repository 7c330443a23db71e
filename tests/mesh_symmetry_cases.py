"""Cases of fp_mesh_transform_residuals and of the symmetry detector.  A kernel case is dict(name, pos (Nv,3) float32, faces (F,3)
int32, points (Q,3) float32, tfs (T,4,4) float32, thr2 (L,) float32): the meshes and points are those of
tests/mesh_distance_cases.py, the transforms and thresholds are made here.  A shape is (pos float64, faces) with the size of its
rotation group known in closed form; posed() puts it into a random rigid pose, so that no axis lies on a coordinate or grid axis."""
import functools
import math

import numpy as np

import mesh_distance_cases as mc
import mesh_symmetry_model as sm

f32 = np.float32
T_SIZES = (1, 2, 3, 70, 257)
L_SIZES = (0, 1, 4)


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rigid_transforms(T, seed, extent, identity_first=True):
    """T transforms: the identity, then random rotations with translations of up to a fifth of `extent`; the fourth row is poisoned
    (it is never read)"""
    rng = np.random.default_rng(seed)
    m = np.zeros((T, 4, 4))
    for t in range(T):
        m[t, :3, :3] = random_rotation(rng)
        m[t, :3, 3] = rng.uniform(-0.2, 0.2, 3) * extent
    if identity_first:
        m[0, :3] = np.eye(4)[:3]
    m[:, 3] = [np.nan, np.inf, -1e30, 7.0]
    return m.astype(f32)


def _thr2(L, seed, extent):
    return sm.square_thresholds(np.random.default_rng(seed).uniform(0.02, 0.4, L) * extent)


def _extent(c):
    p = c["pos"][np.isfinite(c["pos"]).all(axis=1)] if len(c["pos"]) else np.zeros((0, 3), f32)
    return float(np.abs(p).max()) if len(p) and np.abs(p).max() > 0 else 1.0


def _with(c, name, tfs, thr2, **kw):
    return dict(name=name, pos=c["pos"], faces=c["faces"], points=c["points"], tfs=np.ascontiguousarray(tfs, f32),
                thr2=np.ascontiguousarray(thr2, f32), **kw)


def _pick(c, q):
    d = dict(c)
    d["points"] = np.ascontiguousarray(c["points"][:q])
    return d


def special_transforms(extent):
    """identity, a random rigid one, one with scale, one with a NaN entry, one with an infinite translation, one that overflows"""
    m = rigid_transforms(6, 77, extent)
    m[2, :3, :3] *= f32(1.7)
    m[3, 1, 2] = np.nan
    m[4, 0, 3] = np.inf
    m[5, :3, :3] *= f32(3e38)
    return m


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """every mesh and size of mesh_distance_cases, each with one T of T_SIZES and one L of L_SIZES so that every value comes up
    several times, the queries cut where T * Q * F would take the restatement too long; then the named cases"""
    out = []
    for n, c in enumerate(mc.all_cases()):
        T, L = T_SIZES[n % len(T_SIZES)], L_SIZES[(n // 2) % len(L_SIZES)]
        F = max(1, len(c["faces"]))
        q = max(1, min(len(c["points"]), 600_000 // (T * F)))
        if T >= 70 and len(c["points"]) >= 65:
            q = max(q, 65)                            # more than one sample per lane stride of the finish, pairs across tiles
        c = _pick(c, q)
        out.append(_with(c, f"{c['name']} T={T} L={L}", rigid_transforms(T, 300 + n, _extent(c)), _thr2(L, 400 + n, _extent(c))))
    box = next(c for c in mc.all_cases() if c["name"] == "box")
    skipped = next(c for c in mc.all_cases() if c["name"] == "skipped and degenerate")
    for c in (box, skipped):
        out.append(_with(_pick(c, 300), f"{c['name']} special transforms", special_transforms(_extent(c)), _thr2(4, 9, _extent(c))))
    out.append(_with(_pick(box, 200), "box three transforms", rigid_transforms(3, 21, _extent(box)), _thr2(1, 21, _extent(box))))
    out.append(_with(dict(box, faces=box["faces"][:0]), "box without faces T=3", rigid_transforms(3, 5, 1.0), _thr2(4, 5, 0.1)))
    for Q in (1, 63, 64, 65, 257, 1000):                                # every Q with a T that is no divisor of the tile
        c = mc.soup(40, Q, 700 + Q)
        out.append(_with(c, f"soup F=40 Q={Q} T=3", rigid_transforms(3, Q, 0.1), _thr2(1, Q, 0.1)))
    c = mc.soup(3000, 70, 811)                                          # faces in three chunks of 1024, T > 1
    out.append(_with(c, "three chunks T=5", rigid_transforms(5, 12, 0.1), _thr2(4, 12, 0.1)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def references():
    """the restatement's answer for every kernel case, computed once: name -> (max_d2, over, dist2)"""
    return {c["name"]: sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], c["tfs"], c["thr2"]) for c in kernel_cases()}


# ------------------------------------------------------------------ shapes with known rotation groups
def box_shape(sx, sy, sz):
    h = np.array([sx, sy, sz]) / 2
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * h
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    return v, np.asarray(f, np.int32)


def prism(n, radius, height):
    """a right prism over a regular n-gon: the caps are fans from their centres"""
    ang = np.arange(n) / n * 2 * math.pi
    ring = np.stack([radius * np.cos(ang), radius * np.sin(ang)], axis=1)
    v = [[x, y, -height / 2] for x, y in ring] + [[x, y, height / 2] for x, y in ring] + [[0, 0, -height / 2], [0, 0, height / 2]]
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [[i, j, n + j], [i, n + j, n + i], [2 * n, j, i], [2 * n + 1, n + i, n + j]]
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


def tetrahedron(edge=1.0):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * (edge / (2 * math.sqrt(2)))
    return v, np.asarray([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def l_prism_shape(arm=0.09, width=0.03, h=0.025):
    """an L-shaped prism with equal arms (tests/geometry_cases.py's l_prism has arms of 0.08 and 0.09 and so no symmetry): its one
    symmetry is the half turn about the diagonal of the L in the mid-plane, (x, y, z) -> (y, x, -z)"""
    poly = np.array([[0, 0], [arm, 0], [arm, width], [width, width], [width, arm], [0, arm]], np.float64)
    verts = [[x, y, -h] for x, y in poly] + [[x, y, h] for x, y in poly]
    cap = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5]]
    faces = [[a, c, b] for a, b, c in cap] + [[a + 6, b + 6, c + 6] for a, b, c in cap]
    for i in range(6):
        j = (i + 1) % 6
        faces += [[i, j, j + 6], [i, j + 6, i + 6]]
    return np.asarray(verts, np.float64), np.asarray(faces, np.int32)


def pulled_box():
    v, f = box_shape(1.0, 1.0, 1.0)
    v = v.copy()
    v[7] += [0.35, 0.2, 0.5]
    return v, f


def posed(shape, seed):
    """the shape in a random rigid pose -> (pos float32, faces int32, R, t)"""
    rng = np.random.default_rng(seed)
    R, t = random_rotation(rng), rng.uniform(-0.5, 0.5, 3)
    v, f = shape
    return (v @ R.T + t).astype(f32), np.asarray(f, np.int32), R, t


def dihedral(n, axis=(0, 0, 1), first=(1, 0, 0), half_step=False):
    """the 2n rotations of a regular n-gon prism about the origin: n about `axis`, n half turns about axes in its plane (the first
    along `first`, then every pi / n)"""
    from foundationpose_amd.symmetry import axis_rotation
    a, u = np.asarray(axis, np.float64), np.asarray(first, np.float64)
    w = np.cross(a, u)
    out = [axis_rotation(a, 2 * math.pi * j / n) for j in range(n)]
    out += [axis_rotation(math.cos(math.pi * j / n) * u + math.sin(math.pi * j / n) * w, math.pi) for j in range(n)]
    return np.stack(out)


def cube_group():
    """the 24 rotations of the cube: the signed permutation matrices of determinant +1"""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((-1, 1), repeat=3):
            m = np.zeros((3, 3))
            for r in range(3):
                m[r, perm[r]] = signs[r]
            if np.linalg.det(m) > 0:
                out.append(m)
    return np.stack(out)


def tetrahedral_group():
    """the 12 rotations of tetrahedron(): the cube's rotations that keep its vertex set"""
    v = tetrahedron()[0]
    keys = {tuple(np.round(x, 6)) for x in v}
    return np.stack([m for m in cube_group() if {tuple(np.round(m @ x, 6)) for x in v} == keys])


def continuous_group(step_deg, flip):
    from foundationpose_amd.symmetry import axis_rotation
    steps = [axis_rotation((0, 0, 1), math.radians(d)) for d in np.arange(0.0, 360.0, step_deg)]
    return np.stack(steps + ([s @ axis_rotation((1, 0, 0), math.pi) for s in steps] if flip else []))


def match_groups(got, expected, tol_rad):
    """Are the two sets of rotations the same, element for element?  -> (ok, the largest angle of a matched pair): every returned
    rotation is paired with the expected one nearest to it by the rotation angle of R_a R_b^T, the counts are equal, no expected
    one is used twice and every pair is within tol_rad"""
    got, expected = np.asarray(got), np.asarray(expected)
    if len(got) != len(expected):
        return False, math.inf
    tr = np.einsum("aij,bij->ab", got, expected)
    ang = np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0))
    pick = ang.argmin(axis=1)
    worst = float(ang[np.arange(len(got)), pick].max())
    return len(set(pick.tolist())) == len(expected) and worst <= tol_rad, worst
