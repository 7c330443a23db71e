"""numpy restatement of fp_mesh_icp_step (include/fp_amd.h): the float32 quantities of every (transform, sample) pair operation for
operation -- the transformed point of tests/mesh_symmetry_model.py, the closest point of tests/mesh_distance_model.py, the face
normal made a unit vector through float64, the residual and the Jacobian row -- then the float64 sums, the solve and the update of
tests/icp_model.py (numpy's order, or exactly rounded with math.fsum as the reference the device's sums are bounded against).  Also
the callable that drives foundationpose_amd.mesh_align.align on the host (host_align), and an independent float64 formulation
of the rows (rows_float64).

`wrong=` names a deliberately wrong variant (tests/test_mesh_icp_host.py shows that named cases tell each from the definition):
  "r_sign"        the normal's sign flipped in the residual alone, r = -(m.e)  (flipped in r and J alike it changes no output: A and b
                  are even in m, which is why the winding of b's faces does not matter)
  "e_swapped"     e = p - q
  "world_origin"  the rotation taken about the world origin (a = p) while t' = t + v is kept
  "unnormalised"  m = n, the cross product itself
  "lt"            a pair needs dd < max_dist^2 where the definition has <=
Test infrastructure only."""
import math

import numpy as np

import icp_model as im
import mesh_distance_model as mm
import mesh_symmetry_model as sm

f32 = np.float32
WRONG = ("r_sign", "e_swapped", "world_origin", "unnormalised", "lt")


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def pair_terms(pos, faces, points, tfs, max_dist, wrong=None):
    """-> dict(pair (T,Q) bool, J (T,Q,6) float32, r (T,Q) float32 (0 where there is no pair), dist2 (T,Q) float32, face (T,Q) int32)"""
    tfs = np.asarray(tfs, f32).reshape(-1, 4, 4)
    p = sm.transform_points(points, tfs)                                   # (T,Q,3)
    T, Q = p.shape[:2]
    dd, face, q = mm.mesh_point_distance(pos, faces, p.reshape(-1, 3))
    dd, face, q = dd.reshape(T, Q), face.reshape(T, Q), q.reshape(T, Q, 3)
    tri = mm.face_vertices(pos, faces)
    if len(tri) == 0:
        tri = np.full((1, 3, 3), np.nan, f32)
    t = tri[np.clip(face, 0, len(tri) - 1)]                               # (T,Q,3,3)
    with np.errstate(all="ignore"):
        ab, ac = t[..., 1, :] - t[..., 0, :], t[..., 2, :] - t[..., 0, :]
        n = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                      ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], -1).astype(f32)
        n64 = n.astype(np.float64)
        nn = _dot3(n64[..., 0], n64[..., 0], n64[..., 1], n64[..., 1], n64[..., 2], n64[..., 2])
        m = n if wrong == "unnormalised" else (n64 / np.sqrt(nn)[..., None]).astype(f32)
        e = (p - q) if wrong == "e_swapped" else (q - p)
        m0, m1, m2 = m[..., 0], m[..., 1], m[..., 2]
        r = _dot3(m0, e[..., 0], m1, e[..., 1], m2, e[..., 2])
        if wrong == "r_sign":
            r = -r
        c = np.zeros((T, 1, 3), f32) if wrong == "world_origin" else tfs[:, None, :3, 3]
        a = p - c
        a0, a1, a2 = a[..., 0], a[..., 1], a[..., 2]
        J = np.stack([a1 * m2 - a2 * m1, a2 * m0 - a0 * m2, a0 * m1 - a1 * m0, m0, m1, m2], -1)
        md2 = f32(max_dist) * f32(max_dist)
        gate = (dd < md2) if wrong == "lt" else (dd <= md2)
        pair = (face >= 0) & (nn > 0) & np.isfinite(m).all(-1) & gate
    J = np.where(pair[..., None], J, f32(0)).astype(f32)
    r = np.where(pair, r, f32(0)).astype(f32)
    return dict(pair=pair, J=J, r=r, dist2=dd.astype(f32), face=face.astype(np.int32))


def sums(terms, exact=False):
    """-> S (T,29) in system's order with the pair count, sdd (T,) the sum of the pairs' dd; with exact=True the exactly rounded sums
    and also absS (T,28) = sum |term| per column (the sum of dd is its own absolute sum)"""
    pair, dd = terms["pair"], terms["dist2"].astype(np.float64)
    got = im.sums(pair, terms["J"], terms["r"], exact=exact)
    sdd = np.zeros(len(pair))
    for t in range(len(pair)):
        v = dd[t][pair[t]]
        sdd[t] = math.fsum(v.tolist()) if exact else v.sum()
    return (got[0], got[1], sdd) if exact else (got, sdd)


def step(pos, faces, points, tfs, max_dist, damping=1e-3, min_pairs=6, wrong=None, exact=False):
    """one fp_mesh_icp_step call -> (tfs_out (T,4,4) float32, system (T,40), terms)"""
    terms = pair_terms(pos, faces, points, tfs, max_dist, wrong)
    got = sums(terms, exact=exact)
    S, sdd = got[0], got[-1]
    system, out = im.finish(S, np.asarray(tfs, f32).reshape(-1, 4, 4), damping, min_pairs)
    system[:, 36] = sdd
    return out, system, terms


# ------------------------------------------------------------------ an independent float64 formulation
def rows_float64(pos, faces, points, tf, face):
    """The rows of one transform written the way a textbook has them, in float64 throughout, for samples whose nearest point lies
    INSIDE the triangle `face` says (the caller selects those: region 7 of the walk) -> (J (k,6), r (k,)): p = R x + t, the unit
    normal m of the face from float64 vertices, r = m . (a - p) -- the signed distance to the face's plane, which is m . (q - p) for
    the foot q of the perpendicular -- and J = ((p - t) x m, m).  Nothing is shared with the restatement: no closest-point walk,
    numpy's cross and norm."""
    pos = np.asarray(pos, np.float64)
    tf = np.asarray(tf, np.float64)
    f = np.asarray(faces)[np.asarray(face)]
    a, b, c = pos[f[:, 0]], pos[f[:, 1]], pos[f[:, 2]]
    n = np.cross(b - a, c - a)
    m = n / np.linalg.norm(n, axis=1, keepdims=True)
    p = np.asarray(points, np.float64) @ tf[:3, :3].T + tf[:3, 3]
    return np.concatenate([np.cross(p - tf[:3, 3], m), m], axis=1), np.einsum("ij,ij->i", m, a - p)


# ------------------------------------------------------------------ the policy on the host
def host_align(a, b, starts=300, samples=(128, 2048), iterations=(12, 20), max_dist=None, min_overlap=0.5, init=None, seed=0,
               points=None, **kw):
    """mesh_align.align driven by the restatement: what reconstruct.align_meshes does on the device, on the host.  a, b: (pos, faces).
    points: (coarse, fine) sample arrays of a in the place of sample_surface's (for noisy or partial scans) -> ops.MeshAlignment"""
    from foundationpose_amd import mesh_align, ops
    from foundationpose_amd.symmetry import surface_centre
    pa, fa = np.asarray(a[0], f32).reshape(-1, 3), np.asarray(a[1], np.int32).reshape(-1, 3)
    pb, fb = np.asarray(b[0], f32).reshape(-1, 3), np.asarray(b[1], np.int32).reshape(-1, 3)
    if points is None:
        points = (mm.sample_surface(pa, fa, samples[0], seed=seed + 1)[0], mm.sample_surface(pa, fa, samples[1], seed=seed)[0])
    pts = {"coarse": np.asarray(points[0], f32), "fine": np.asarray(points[1], f32)}
    centre_b, radius_b = surface_centre(pb, fb)

    def steps(which, tfs, gate, n):
        m = np.asarray(tfs, np.float64).astype(f32)
        for _ in range(n):
            m, _, _ = step(pb, fb, pts[which], m, gate)
        _, system, terms = step(pb, fb, pts[which], m, gate)
        return m.astype(np.float64), system, terms["dist2"]

    got = mesh_align.align(steps, pts["coarse"].astype(np.float64).mean(axis=0), centre_b, radius_b,
                           (len(pts["coarse"]), len(pts["fine"])), starts=starts, iterations=iterations, max_dist=max_dist,
                           min_overlap=min_overlap, init=init, seed=seed, **kw)
    return ops.MeshAlignment(*(got[k] for k in ops.MeshAlignment._fields))
