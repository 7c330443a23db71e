"""The numpy restatement of fp_icp_point_plane (include/fp_amd.h): the per-pixel float32 quantities op for op, the float64 sums (in
numpy's order, or exactly rounded with math.fsum as the reference the device's sums are bounded against), the LDL^T solve in the
header's order and the pose update.  `wrong` switches ONE piece to a neighbouring, wrong definition (tests/test_icp_host.py shows that
named cases tell each from the right one):
  r_sign         r = -(m.e)
  cross_swapped  the rotational half of J is m x a instead of a x m
  camera_origin  the rotation is taken about the camera origin (a = p) while t' = t + v is kept
  no_gate        no max_dist gate: every valid pixel is a pair
  floor          the texel is floor(ix), floor(iy) instead of nn_index (round half to even)
  no_diag        the damping adds damping * I instead of damping * diag(A)
Test infrastructure only."""
import math

import numpy as np

from raster_model import fmaf

F = np.float32
WRONG = ("r_sign", "cross_swapped", "camera_origin", "no_gate", "floor", "no_diag")
TRI = [(i, j) for i in range(6) for j in range(i, 6)]          # system[0..20]: A's upper triangle, row-major


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def texels(tf, H, W, oh, ow, wrong=None):
    """the frame texel every crop pixel reads (crop_inverse, crop_to_frame, nn_index of csrc/crop_map.h) -> qx, qy int64 (N,oh,ow)"""
    tf = np.asarray(tf, F).reshape(-1, 3, 3)
    sx, tx, sy, ty = (tf[:, a, b][:, None, None] for a, b in ((0, 0), (0, 2), (1, 1), (1, 2)))
    with np.errstate(all="ignore"):
        i00, i11 = F(1) / sx, F(1) / sy
        i02, i12 = (-tx) / sx, (-ty) / sy
        cW, cH = F(W) / F(W - 1), F(H) / F(H - 1)
        ii = np.arange(ow, dtype=F)[None, None, :]
        jj = np.arange(oh, dtype=F)[None, :, None]
        ix = fmaf(fmaf(ii, i00, i02), cW, F(-0.5)) + np.zeros((1, oh, 1), F)
        iy = fmaf(fmaf(jj, i11, i12), cH, F(-0.5)) + np.zeros((1, 1, ow), F)
        rx, ry = (np.floor(ix), np.floor(iy)) if wrong == "floor" else (np.rint(ix), np.rint(iy))
    lim = 2.0 ** 31 - 1                      # (int)rintf saturates; a NaN converts to 0
    qx = np.clip(np.nan_to_num(rx.astype(np.float64), nan=0.0), -lim - 1, lim).astype(np.int64)
    qy = np.clip(np.nan_to_num(ry.astype(np.float64), nan=0.0), -lim - 1, lim).astype(np.int64)
    return qx, qy


def pixel_terms(xyz_crops, normal_crops, xyz_map, tf, poses, max_dist, view=None, wrong=None):
    """-> pair (N,oh,ow) bool, J (N,oh,ow,6) float32, r (N,oh,ow) float32 (J and r are 0 where there is no pair)"""
    p = np.asarray(xyz_crops, F)
    m = np.asarray(normal_crops, F)
    N, oh, ow, _ = p.shape
    xm = np.asarray(xyz_map, F)
    if xm.ndim == 3:
        xm = xm[None]
    V, H, W, _ = xm.shape
    view = np.zeros(N, np.int64) if view is None else np.asarray(view, np.int64).reshape(N)
    P = np.asarray(poses, F).reshape(N, 16)
    qx, qy = texels(tf, H, W, oh, ow, wrong)
    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & ((view >= 0) & (view < V))[:, None, None]
    vv = np.clip(view, 0, V - 1)[:, None, None]
    q = np.where(inside[..., None], xm[vv, np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)], F(0))
    with np.errstate(all="ignore"):
        m0, m1, m2 = m[..., 0], m[..., 1], m[..., 2]
        model = (p[..., 2] > 0) & (_dot3(m0, m0, m1, m1, m2, m2) > 0)
        valid = model & (q[..., 2] >= F(0.001))
        e = q - p
        e0, e1, e2 = e[..., 0], e[..., 1], e[..., 2]
        md2 = F(max_dist) * F(max_dist)
        pair = valid if wrong == "no_gate" else valid & (_dot3(e0, e0, e1, e1, e2, e2) <= md2)
        r = _dot3(m0, e0, m1, e1, m2, e2)
        if wrong == "r_sign":
            r = -r
        c = np.zeros((N, 1, 1, 3), F) if wrong == "camera_origin" else P[:, None, None, [3, 7, 11]]
        a = p - c
        a0, a1, a2 = a[..., 0], a[..., 1], a[..., 2]
        J = np.stack([a1 * m2 - a2 * m1, a2 * m0 - a0 * m2, a0 * m1 - a1 * m0, m0, m1, m2], -1)
        if wrong == "cross_swapped":
            J[..., :3] = -J[..., :3]
    J = np.where(pair[..., None], J, F(0)).astype(F)
    r = np.where(pair, r, F(0)).astype(F)
    return pair, J, r


def sums(pair, J, r, exact=False):
    """-> S (N,29) float64: the 28 sums in system's order and the pair count; with exact=True each sum is math.fsum of its terms
    (the exactly rounded sum) and a second array holds sum |term| per column (the scale of the summation-error bound)"""
    N = pair.shape[0]
    S = np.zeros((N, 29))
    absS = np.zeros((N, 28))
    for n in range(N):
        k = pair[n].reshape(-1)
        Jn = J[n].reshape(-1, 6)[k].astype(np.float64)
        rn = r[n].reshape(-1)[k].astype(np.float64)
        cols = [Jn[:, i] * Jn[:, j] for i, j in TRI] + [Jn[:, i] * rn for i in range(6)] + [rn * rn]   # products of float32 pairs: exact
        for t, term in enumerate(cols):
            if exact:
                with np.errstate(all="ignore"):
                    S[n, t] = math.fsum(term.tolist()) if np.isfinite(term).all() else term.sum()
                    absS[n, t] = math.fsum(np.abs(term).tolist()) if np.isfinite(term).all() else np.inf
            else:
                with np.errstate(all="ignore"):
                    S[n, t] = term.sum()
        S[n, 28] = int(k.sum())
    return (S, absS) if exact else S


def damped(S, damping, wrong=None):
    """A_lambda (6,6) symmetric, from the 21 upper entries of one system row"""
    A = np.zeros((6, 6))
    for t, (i, j) in enumerate(TRI):
        A[i, j] = A[j, i] = S[t]
    for j in range(6):
        A[j, j] = A[j, j] + (damping if wrong == "no_diag" else damping * A[j, j])
    return A


def solve(S, damping, wrong=None):
    """LDL^T without pivoting in the header's order, on one row S of sums -> (x (6,), ok): ok False for a pivot <= 0 or not finite or
    a non-finite x (x is then 0)"""
    A = damped(S, damping, wrong).tolist()
    b = [float(v) for v in S[21:27]]
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            vk = [L[j][k] * d[k] for k in range(j)]
            s = A[j][j]
            for k in range(j):
                s = s - L[j][k] * vk[k]
            d[j] = s
            ok = ok and s > 0.0 and math.isfinite(s)
            for i in range(j + 1, 6):
                u = A[j][i]
                for k in range(j):
                    u = u - L[i][k] * vk[k]
                L[i][j] = float(np.float64(u) / np.float64(s))
        if not ok:
            return np.zeros(6), False
        y = [0.0] * 6
        for i in range(6):
            u = b[i]
            for k in range(i):
                u = u - L[i][k] * y[k]
            y[i] = u
        y = [float(np.float64(y[i]) / np.float64(d[i])) for i in range(6)]
        x = [0.0] * 6
        for i in range(5, -1, -1):
            u = y[i]
            for k in range(i + 1, 6):
                u = u - L[k][i] * x[k]
            x[i] = u
    if not all(math.isfinite(v) for v in x):
        return np.zeros(6), False
    return np.asarray(x), True


def rodrigues(w):
    w0, w1, w2 = (float(v) for v in w)
    th = math.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    if th < 1e-12:
        return np.array([[1.0, -w2, w1], [w2, 1.0, -w0], [-w1, w0, 1.0]])
    k0, k1, k2 = w0 / th, w1 / th, w2 / th
    c, s = math.cos(th), math.sin(th)
    c1 = 1.0 - c
    return np.array([[c + c1 * (k0 * k0), c1 * (k0 * k1) - s * k2, c1 * (k0 * k2) + s * k1],
                     [c1 * (k0 * k1) + s * k2, c + c1 * (k1 * k1), c1 * (k1 * k2) - s * k0],
                     [c1 * (k0 * k2) - s * k1, c1 * (k1 * k2) + s * k0, c + c1 * (k2 * k2)]])


def update64(pose_in, x):
    """the float64 pose update of one float32 pose by the step x, before the rounding to float32 -> (4,4) float64"""
    Pin = np.asarray(pose_in, F).astype(np.float64).reshape(4, 4)
    dR = rodrigues(x[:3])
    out = Pin.copy()
    for i in range(3):
        for j in range(3):
            out[i, j] = _dot3(dR[i, 0], Pin[0, j], dR[i, 1], Pin[1, j], dR[i, 2], Pin[2, j])
        out[i, 3] = Pin[i, 3] + float(x[3 + i])
    return out


def finish(S, poses, damping, min_pairs, wrong=None):
    """the finish kernel on the sums S (N,29) -> system (N,40) float64, poses_out (N,4,4) float32"""
    P = np.asarray(poses, F).reshape(-1, 4, 4)
    N = P.shape[0]
    system = np.zeros((N, 40))
    out = P.copy()
    for n in range(N):
        system[n, :29] = S[n]
        x = np.zeros(6)
        if not np.isfinite(P[n]).all():
            status = 2
        elif S[n, 28] < min_pairs:
            status = 1
        else:
            x, ok = solve(S[n], damping, wrong)
            status = 0 if ok else 2
        system[n, 29] = status
        system[n, 30:36] = x
        if status == 0:
            with np.errstate(all="ignore"):
                out[n] = update64(P[n], x).astype(F)
    return system, out


def step(xyz_crops, normal_crops, xyz_map, tf, poses, max_dist, damping=1e-3, min_pairs=64, view=None, wrong=None, exact=False):
    """one fp_icp_point_plane call -> (system (N,40), poses_out (N,4,4) float32)"""
    pair, J, r = pixel_terms(xyz_crops, normal_crops, xyz_map, tf, poses, max_dist, view, wrong)
    S = sums(pair, J, r, exact=exact)
    return finish(S[0] if exact else S, poses, damping, min_pairs, wrong)


def ldl_backward_bound(A_l, x):
    """|A_l x - b|_inf of a solve by LDL^T (Cholesky-like, no pivoting, A_l positive definite) with unit roundoff u = 2^-53:
    (A_l + dA) x = b with |dA| <= gamma_{3n+1} |L||D||L^T| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem
    10.4 for Cholesky; with R = D^(1/2) L^T, |L||D||L^T| = |R^T||R|).  Entry (i, j) of |R^T||R| is at most |r_i||r_j| =
    sqrt(a_ii a_jj) <= max_k a_kk <= ||A_l||_inf (Cauchy-Schwarz on the columns of R), so || |R^T||R| ||_inf <= n ||A_l||_inf and the
    residual is <= gamma_{3n+1} n ||A_l||_inf ||x||_inf = c n^2 2^-53 ||A_l||_inf ||x||_inf with c = (3n + 1) / n ~ 3.2 for n = 6;
    c = 4 is used."""
    n = 6
    return 4.0 * n * n * 2.0 ** -53 * np.abs(A_l).sum(1).max() * np.abs(x).max()


# ------------------------------------------------------------------------------------------------ the polish loop on the CPU oracle
CROP, CROP_RATIO = (160, 160), 1.2


def perturbations(gt, n=32, seed=0, max_trans=0.008, norm=(0.005, 0.011), rot_deg=(1.0, 4.0), axis=2):
    """n seeded perturbations of a pose: a rotation of rot_deg[0]..rot_deg[1] degrees (applied on the left, about the pose's origin)
    and a translation drawn uniformly from +-max_trans per camera axis.  Two rejections keep the set meaningful.  The translation is
    redrawn until its length lies in `norm`: at least 5 mm, so that a gate of about 1 mm is well below every start error, and at most
    11 mm, because one step of ICP with pairs gated at 20 mm is a local method (measured on the conftest scene: a 13.1 mm offset
    towards one corner of the +-8 mm cube with a 2 degree tilt locks onto the wrong pairs and walks away, with status 0 throughout).
    The rotation axis is redrawn until it is at least 30 degrees away from the object's own `axis` as the camera sees it (a turn about
    a solid of revolution's axis is no error of its pose), so every perturbation tilts that axis by at least sin(30 deg) of its angle.
    -> (n,4,4) float32"""
    rng = np.random.default_rng(seed + 4000)
    out = np.tile(np.asarray(gt, np.float64)[None], (n, 1, 1))
    own = np.asarray(gt, np.float64)[:3, axis]
    for i in range(n):
        while True:
            k = rng.normal(size=3)
            k /= np.linalg.norm(k)
            if abs(k @ own) <= np.cos(np.deg2rad(30.0)):
                break
        while True:
            t = rng.uniform(-max_trans, max_trans, size=3)
            if norm[0] <= np.linalg.norm(t) <= norm[1]:
                break
        out[i, :3, :3] = rodrigues(k * np.deg2rad(rng.uniform(*rot_deg))) @ out[i, :3, :3]
        out[i, :3, 3] += t
    return out.astype(F)


def pose_errors(P, gt, axis=2):
    """-> (translation error in metres, tilt of the object's `axis` in degrees) of poses (n,4,4) against gt (4,4)"""
    P = np.asarray(P, np.float64).reshape(-1, 4, 4)
    gt = np.asarray(gt, np.float64)
    dt = np.linalg.norm(P[:, :3, 3] - gt[:3, 3], axis=1)
    cosang = np.clip(P[:, :3, axis] @ gt[:3, axis] / np.linalg.norm(P[:, :3, axis], axis=1), -1, 1)
    return dt, np.rad2deg(np.arccos(cosang))


def oracle_xyz_map(depth, K):
    """the tracking ingest on the CPU oracle: erode, bilateral, back-projection in float32 -> (H,W,3)"""
    from oracle import ops as oo
    from oracle import pipeline as op
    return oo.depth2xyzmap(op.preprocess_depth(np.asarray(depth, F)), K, f64_internal=False)


def polish_oracle(mesh_np, diameter, K, H, W, xyz_map, poses, iterations=3, max_dist=0.02, damping=1e-3, min_pairs=64, wrong=None,
                  crop=CROP, crop_ratio=CROP_RATIO):
    """PoseRefinePredictor.depth_polish with the CPU oracle's crop windows and renders and this restatement's step
    -> (poses (n,4,4) float32, [system (n,40)] per iteration)"""
    from oracle import ops as oo
    P = np.asarray(poses, F).reshape(-1, 4, 4)
    oh, ow = crop
    systems = []
    for _ in range(iterations):
        tf, bb = oo.crop_windows(P, K, diameter, crop_ratio, (ow, oh))
        r = oo.render_crops(mesh_np, P, bb, K, H, W, (oh, ow), diameter, normalize_xyz=False, want=("xyz", "normal"))
        system, P = step(r["xyz"], r["normal"], xyz_map, tf, P, max_dist, damping, min_pairs, wrong=wrong)
        systems.append(system)
    return P, systems


# ------------------------------------------------------------------------------------------------ generated arrays (no renders)
def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def generated_case(N, oh, ow, V=1, H=24, W=32, seed=0, max_dist=0.02):
    """Arrays for fp_icp_point_plane that no renderer made: a random observed map (V,H,W,3) and, per crop pixel, a model point p at a
    random offset of up to 1.5 max_dist from the texel it reads (so the gate cuts some), random unit normals, random poses, and the
    edge cases of the definition sprinkled in -- windows partly and (every fifth hypothesis) wholly outside the frame, view indices
    outside 0..V-1 (for V > 1), texels without depth, with z exactly 0.001 and one ulp below, pairs whose e.e is exactly max_dist^2 and
    one ulp above, p.z of 0, negative and NaN, NaN normals and observed points, zero normals, one hypothesis (N >= 3) whose normals are
    all (0, 0, 1) (a singular system) and one (N >= 4) with a NaN pose.  -> dict of float32 / int32 arrays"""
    rng = np.random.default_rng(seed)
    md = F(max_dist)
    xm = np.empty((V, H, W, 3), F)
    xm[..., :2] = rng.uniform(-0.1, 0.1, (V, H, W, 2))
    xm[..., 2] = rng.uniform(0.4, 0.6, (V, H, W))
    flat = xm.reshape(-1, 3)
    k = rng.permutation(flat.shape[0])
    n8 = max(1, flat.shape[0] // 16)
    flat[k[:n8], 2] = 0                                                   # no depth
    flat[k[n8:2 * n8]] = (0.0, 0.0, 0.5)                                  # texels the exact-threshold pairs hang on
    flat[k[2 * n8:2 * n8 + n8 // 2], 2] = F(0.001)
    flat[k[2 * n8 + n8 // 2:3 * n8], 2] = np.nextafter(F(0.001), F(0))
    flat[k[3 * n8:3 * n8 + max(1, n8 // 4)], rng.integers(0, 3)] = np.nan
    # windows: crop = s * frame + t, the frame rectangle [x0, x0 + w) x [y0, y0 + h)
    tf = np.zeros((N, 3, 3), F)
    for n in range(N):
        w, h = rng.uniform(0.3, 1.2) * W, rng.uniform(0.3, 1.2) * H
        x0, y0 = rng.uniform(-0.3 * W, W - 0.5 * w), rng.uniform(-0.3 * H, H - 0.5 * h)
        if n % 5 == 4:
            x0 += 3.0 * W                                                 # wholly outside
        sx, sy = ow / w, oh / h
        tf[n] = [[sx, 0, -sx * x0], [0, sy, -sy * y0], [0, 0, 1]]
    view = rng.integers(0, V, N).astype(np.int32)
    if V > 1 and N >= 3:
        view[rng.integers(0, N)] = V
        view[rng.integers(0, N)] = -1
    poses = np.tile(np.eye(4, dtype=F), (N, 1, 1))
    for n in range(N):
        poses[n, :3, :3] = _rotation(rng)
        poses[n, :3, 3] = (rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(0.45, 0.55))
    qx, qy = texels(tf, H, W, oh, ow)
    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & ((view >= 0) & (view < V))[:, None, None]
    q = np.where(inside[..., None], xm[np.clip(view, 0, V - 1)[:, None, None], np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)], F(0))
    d = rng.normal(size=(N, oh, ow, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        p = (q - (d * rng.uniform(0, 1.5 * max_dist, (N, oh, ow, 1))).astype(F)).astype(F)
    p = np.where(np.isnan(p), F(0.5), p)                                  # (a NaN texel stays a NaN in q alone)
    m = rng.normal(size=(N, oh, ow, 3))
    m = (m / np.linalg.norm(m, axis=-1, keepdims=True)).astype(F)
    # exact thresholds on the (0, 0, 0.5) texels: e = (md, 0, 0) has e.e == md * md; e = (md, y, 0) with y * y one ulp of it is one above
    md2 = md * md
    y = F(np.sqrt(np.float64(np.nextafter(md2, F(1)) - md2)))
    assert _dot3(md, md, y, y, F(0), F(0)) == np.nextafter(md2, F(1)) and _dot3(md, md, F(0), F(0), F(0), F(0)) == md2
    hang = inside & (q[..., 0] == 0) & (q[..., 1] == 0) & (q[..., 2] == F(0.5))
    idx = np.argwhere(hang)
    for c, (n, j, i) in enumerate(idx):
        p[n, j, i] = (-md, -y if c % 2 else F(0), F(0.5))
    roll = rng.uniform(size=(N, oh, ow))
    roll[hang] = 1.0
    p[roll < 0.02, 2] = 0
    p[(roll >= 0.02) & (roll < 0.04), 2] *= -1
    p[(roll >= 0.04) & (roll < 0.05), 2] = np.nan
    p[(roll >= 0.05) & (roll < 0.06), 0] = np.nan
    m[(roll >= 0.06) & (roll < 0.08)] = 0
    m[(roll >= 0.08) & (roll < 0.09), 1] = np.nan
    if N >= 3:
        m[2] = (0, 0, 1)
    if N >= 4:
        poses[3, 1, 2] = np.nan
    return dict(xyz_crops=np.ascontiguousarray(p), normal_crops=np.ascontiguousarray(m), xyz_map=xm, tf=tf, view=view, poses=poses, V=V,
                max_dist=float(max_dist), thresholds=int(len(idx)))


# ------------------------------------------------------------------------------------------------ reference views on the CPU
def view_perturbations(poses, seed=0, max_trans=0.004, rot_deg=(0.5, 1.5)):
    """every view's pose with its own seeded error: a rotation of rot_deg about a random axis (on the left) and +-max_trans per axis"""
    rng = np.random.default_rng(seed + 7000)
    out = np.asarray(poses, np.float64).copy()
    for i in range(len(out)):
        k = rng.normal(size=3)
        k /= np.linalg.norm(k)
        out[i, :3, :3] = rodrigues(k * np.deg2rad(rng.uniform(*rot_deg))) @ out[i, :3, :3]
        out[i, :3, 3] += rng.uniform(-max_trans, max_trans, size=3)
    return out.astype(F)


def fuse_model(spec, views, poses):
    """tests/tsdf_model.py: fuse the views at `poses` into a fresh volume and extract -> (pos, col, nrm, faces)"""
    import tsdf_model as tm
    origin, dims, s, trunc = spec
    vol = tm.integrate(tm.Volume(dims, origin, s, trunc), views["depth"], views["rgb"], views["masks"], poses, views["Ks"])
    return tm.extract(vol)


def refine_views_model(mesh, views, poses, H, W, iterations=3, max_dist=0.01):
    """reconstruct.refine_view_poses with the CPU oracle's renders and this restatement: every view against its own masked,
    unfiltered depth, through windows around the sphere about the origin that holds the mesh -> (poses, [status])"""
    from oracle import ops as oo
    pos, col, nrm, faces = mesh
    mesh_np = dict(pos=np.asarray(pos, F), vnormals=np.asarray(nrm, F), faces=np.asarray(faces, np.int32),
                   vertex_color=(np.asarray(col, F) / F(255)))
    diam = 2.0 * float(np.linalg.norm(np.asarray(pos, np.float64), axis=1).max())
    out, status = [], []
    for v in range(len(poses)):
        d = np.where(views["masks"][v] != 0, views["depth"][v], F(0)).astype(F)
        xyz = oo.depth2xyzmap(d, views["Ks"][v], f64_internal=False)
        P, systems = polish_oracle(mesh_np, diam, views["Ks"][v], H, W, xyz, poses[v:v + 1], iterations, max_dist)
        out.append(P[0])
        status.append(int(systems[-1][0, 29]))
    return np.stack(out), status
