"""Cases of fp_mesh_icp_step.  A kernel case is dict(name, pos (Nv,3) float32, faces (F,3) int32, points (Q,3) float32, tfs (T,4,4)
float32, max_dist): the meshes and points are those of tests/mesh_distance_cases.py, the transforms those of
tests/mesh_symmetry_cases.py.  Also the shapes and the scans of the alignment tests."""
import functools

import numpy as np

import mesh_distance_cases as mc
import mesh_icp_model as mi
import mesh_symmetry_cases as sc

f32 = np.float32
T_SIZES = (1, 2, 70, 257)
NO_GATE = 1e18


def _with(c, name, tfs, max_dist):
    tfs = np.array(tfs, f32)
    tfs[:, 3] = (0.5, -2.0, 1e30, 7.0)               # row 3 is not read but must be finite (a non-finite entry is status 2) and is copied
    return dict(name=name, pos=c["pos"], faces=c["faces"], points=c["points"], tfs=np.ascontiguousarray(tfs, f32), max_dist=float(max_dist))


def threshold_case():
    """one triangle in the plane z = 0 and samples straight above its interior, under the identity: dd = h * h in float32, the very
    product max_dist * max_dist is for max_dist = h.  Six samples at h (pairs by `<=`, none by `<`), six one ulp higher (no pairs),
    six at half the height (pairs either way)"""
    h = f32(0.0371)
    up = np.nextafter(h, f32(1))
    assert up * up > h * h
    xy = [(0.2, 0.2), (0.3, 0.1), (0.1, 0.3), (0.25, 0.25), (0.4, 0.2), (0.2, 0.4)]
    pts = [[x, y, z] for z in (h, up, h / f32(2)) for x, y in xy]
    c = mc._case("threshold", [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], pts)
    return _with(c, "pairs on the threshold", np.eye(4, dtype=f32)[None], float(h))


def degenerate_winner_case():
    """the nearest face of every sample is face 0, a zero-area triangle whose vertex test answers (three equal vertices: region 1),
    so it wins with a finite dd and has no normal: no pair; the plain triangle far away never wins"""
    pos = [[0, 0, 0], [0, 0, 0], [0, 0, 0], [5, 0, 0], [6, 0, 0], [5, 1, 0]]
    pts = np.random.default_rng(4).uniform(-0.5, 0.5, (12, 3))
    c = mc._case("degenerate", pos, [[0, 1, 2], [3, 4, 5]], pts)
    return _with(c, "degenerate winning face", np.eye(4, dtype=f32)[None], NO_GATE)


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """every mesh and size of mesh_distance_cases, each with one T of T_SIZES, a gate that cuts some pairs on the even cases and none
    on the odd ones, the queries cut where T * Q * F would take the restatement too long; then the named cases"""
    out = []
    for n, c in enumerate(mc.all_cases()):
        T = T_SIZES[n % len(T_SIZES)]
        F = max(1, len(c["faces"]))
        q = max(1, min(len(c["points"]), 600_000 // (T * F)))
        if T >= 70 and len(c["points"]) >= 65:
            q = max(q, 65)
        c = sc._pick(c, q)
        ext = sc._extent(c)
        out.append(_with(c, f"{c['name']} T={T}", sc.rigid_transforms(T, 500 + n, ext), 0.3 * ext if n % 2 == 0 else NO_GATE))
    box = next(c for c in mc.all_cases() if c["name"] == "box")
    skipped = next(c for c in mc.all_cases() if c["name"] == "skipped and degenerate")
    for c in (box, skipped):
        out.append(_with(sc._pick(c, 300), f"{c['name']} special transforms", sc.special_transforms(sc._extent(c)), NO_GATE))
    out.append(_with(dict(box, faces=box["faces"][:0]), "box without faces T=3", sc.rigid_transforms(3, 5, 1.0), NO_GATE))
    for Q in (1, 63, 64, 65, 255, 256, 257, 1000):
        c = mc.soup(40, Q, 700 + Q)
        out.append(_with(c, f"soup F=40 Q={Q} T=3", sc.rigid_transforms(3, Q, 0.1), 0.05))
    c = mc.soup(3000, 70, 811)                                          # faces in three chunks of 1024, T > 1
    out.append(_with(c, "three chunks T=5", sc.rigid_transforms(5, 12, 0.1), 0.05))
    out += [threshold_case(), degenerate_winner_case()]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def references():
    """the restatement's answer for every kernel case, computed once: name -> dict(terms, S (T,29) exactly rounded, absS (T,28),
    sdd (T,))"""
    out = {}
    for c in kernel_cases():
        terms = mi.pair_terms(c["pos"], c["faces"], c["points"], c["tfs"], c["max_dist"])
        S, absS, sdd = mi.sums(terms, exact=True)
        out[c["name"]] = dict(terms=terms, S=S, absS=absS, sdd=sdd)
    return out


# ------------------------------------------------------------------ alignment
def unequal_l_prism():
    """tests/geometry_cases.py's L-prism (arms of 0.08 and 0.09: no symmetry, but a near one) -> (pos float64, faces)"""
    import geometry_cases as gc
    m = gc.l_prism()
    return np.asarray(m.vertices, np.float64), np.asarray(m.faces, np.int32)


SHAPES = {"pulled_box": sc.pulled_box, "l_prism": unequal_l_prism}


# the worst error of the restatement-driven policy over the seeds 1, 2, 3 (tests/test_mesh_icp_host.py prints them; COVERAGE.md):
# (rotation in degrees, translation as a fraction of the radius)
MEASURED = {"pulled_box": (2.866e-06, 4.445e-08), "l_prism": (3.562e-06, 4.401e-07)}


def alignment_gates(shape, pos):
    """-> (degrees, fraction of the radius): four times the measured error, and no tighter than 16 float32 ulps of the mesh extent
    (the largest coordinate magnitude of b's vertices) -- as a length over the radius, and as the angle that moves a point at the
    radius by that length"""
    p = np.asarray(pos, np.float64)
    radius = float(np.linalg.norm(p - p.mean(axis=0), axis=1).max())
    floor = 16.0 * float(np.spacing(f32(np.abs(np.asarray(pos, f32)).max()))) / radius
    deg, frac = MEASURED[shape]
    return max(4.0 * deg, float(np.degrees(floor))), max(4.0 * frac, floor)


def truth_of(R, t):
    tf = np.eye(4)
    tf[:3, :3], tf[:3, 3] = R, t
    return tf


def rigid_error(tf, truth, radius):
    """the error d = tf truth^-1, a rigid motion in b's frame -> (its rotation angle in degrees, from the skew part, which is well
    conditioned near zero where the arccos of the trace is not; the length of its translation over `radius`)"""
    d = np.asarray(tf, np.float64) @ np.linalg.inv(truth)
    w = 0.5 * np.array([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]])
    ang = float(np.arctan2(np.linalg.norm(w), (np.trace(d[:3, :3]) - 1.0) / 2.0))
    return np.degrees(ang), float(np.linalg.norm(d[:3, 3])) / radius


def noisy_partial_box(seed):
    """the pulled box without its first two triangles, in a seeded pose, sampled with noise of 0.004 of the radius -> (a (pos, faces):
    the partial mesh in its own frame, b (pos, faces): the whole box posed, (coarse, fine) noisy samples of a, truth (4,4))"""
    import mesh_distance_model as mm
    from foundationpose_amd.symmetry import surface_centre
    v, f = sc.pulled_box()
    pos_b, faces_b, R, t = sc.posed((v, f), seed)
    a = (v.astype(f32), f[2:])
    _, radius = surface_centre(v, f)
    rng = np.random.default_rng(seed + 50)
    pts = []
    for n, s in ((128, seed + 1), (2048, seed)):
        p = mm.sample_surface(a[0], a[1], n, seed=s)[0].astype(np.float64)
        pts.append((p + rng.normal(size=p.shape) * 0.004 * radius).astype(f32))
    return a, (pos_b, faces_b), tuple(pts), truth_of(R, t)
