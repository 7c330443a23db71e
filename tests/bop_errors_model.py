"""The numpy restatement of fp_vsd_counts' and fp_mspd's definitions (include/fp_amd.h) that the BOP-error tests compare the kernels
with: every float32 value with one rounding per stated operation, in the stated order; and a float64 evaluation of both straight from
the formulas (BOP's arithmetic) for the cross-checks."""
import numpy as np

BOP_TAUS = tuple(0.05 * k for k in range(1, 11))
BOP_DELTA = 0.015


def dist_factor(K, H, W, dtype=np.float32):
    """fac[v,u] = sqrt(1 + ((u - cx)/fx)^2 + ((v - cy)/fy)^2) in float64 with integer u, v, rounded once to `dtype`"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    a = (np.arange(W, dtype=np.float64)[None, :] - K[0, 2]) / K[0, 0]
    b = (np.arange(H, dtype=np.float64)[:, None] - K[1, 2]) / K[1, 1]
    return np.sqrt(1.0 + a * a + b * b).astype(dtype)


def thresholds(taus, diameter):
    """thr[t] = float32(tau_t * diameter), the product in float64"""
    return (np.asarray(taus, np.float64) * float(diameter)).astype(np.float32)


def _gt_of(gt_index, G, n):
    g = int(gt_index[n]) if gt_index is not None else (0 if G == 1 else n)
    return g if 0 <= g < G else -1


def _pixel_terms(est, gt, obs, fac, delta, dtype):
    """the per-pixel values of the definition in `dtype` -> (vg, ve, inter, union, dist, and the four decided differences)"""
    with np.errstate(invalid="ignore", over="ignore"):
        Do, De, Dg = obs * fac, est * fac, gt * fac
        assert Do.dtype == De.dtype == Dg.dtype == dtype
        seen = Do > 0
        vg = (Dg > 0) & (~seen | ((Dg - Do) <= delta))
        ve = ((De > 0) & (~seen | ((De - Do) <= delta))) | (vg & (De > 0))
        dist = np.abs(Dg - De)
    return vg, ve, vg & ve, vg | ve, dist


def vsd_counts(est, gt, obs, fac, delta, thr, gt_index=None, origin=(0, 0)):
    """-> (N, 4 + T) int32 [n_gt_vis, n_est_vis, n_inter, n_union, c_0 .. c_{T-1}] in float32 exactly as defined; a row of -1 for a
    gt_index outside 0..G-1.  est (N,h,w), gt (G,h,w): the window at frame pixel origin = (x0, y0) of obs / fac (H,W)."""
    est, gt = np.asarray(est, np.float32), np.asarray(gt, np.float32)
    obs, fac = np.asarray(obs, np.float32), np.asarray(fac, np.float32)
    thr, delta = np.asarray(thr, np.float32).reshape(-1), np.float32(delta)
    N, h, w = est.shape
    x0, y0 = origin
    o, f = obs[y0:y0 + h, x0:x0 + w], fac[y0:y0 + h, x0:x0 + w]
    assert o.shape == (h, w) and gt.shape[1:] == (h, w)
    out = np.full((N, 4 + len(thr)), -1, np.int32)
    for n in range(N):
        g = _gt_of(gt_index, len(gt), n)
        if g < 0:
            continue
        vg, ve, inter, union, dist = _pixel_terms(est[n], gt[g], o, f, delta, np.float32)
        with np.errstate(invalid="ignore"):
            out[n] = [vg.sum(), ve.sum(), inter.sum(), union.sum()] + [int((inter & (dist >= t)).sum()) for t in thr]
    return out


def vsd_counts64(est, gt, obs, K, delta, taus, diameter):
    """the same counts for ONE ground truth over the full frame in float64 straight from the formulas (distance images from the float64
    factor, float64 delta and thresholds) -> (counts (N, 4+T) int64, undecided (N, 4+T) int64): undecided[n, c] is the number of pixels
    that can change column c between float32 and float64 -- pixels where a comparison that enters the column is decided by less than the
    float32 rounding error of its operands.  With u = 2^-24: the float32 factor is within u relative of the float64 one and the product
    is rounded once, so a float32 distance D is within e2 = 2u + u^2 relative of its float64 value; a difference of two of them is
    rounded once more, so it is within e2 (|Da| + |Db|) + u (|Da - Db| + e2 (|Da| + |Db|)) of the float64 difference; float32(delta)
    and float32(thr) are within u relative of delta and thr.  The signs of the products are exact, so `> 0` never differs."""
    est, gt, obs = (np.asarray(a, np.float32).astype(np.float64) for a in (est, gt, obs))
    H, W = obs.shape
    fac = dist_factor(K, H, W, np.float64)
    thr = np.asarray(taus, np.float64) * float(diameter)
    u = 2.0 ** -24
    e2 = 2 * u + u * u

    def slack(Da, Db, const):
        s = e2 * (np.abs(Da) + np.abs(Db))
        return s + u * (np.abs(Da - Db) + s) + u * const

    N = len(est)
    counts = np.zeros((N, 4 + len(thr)), np.int64)
    undecided = np.zeros_like(counts)
    with np.errstate(invalid="ignore"):
        Do_all, Dg_all = np.where(obs > 0, obs, 0.0) * fac, gt * fac
        for n in range(N):
            m = (est[n] > 0) | (gt > 0)                       # every other pixel counts nothing in either arithmetic
            Do, Dg, De = Do_all[m], Dg_all[m], (est[n] * fac)[m]
            seen = Do > 0
            vg = (Dg > 0) & (~seen | ((Dg - Do) <= delta))
            ve = ((De > 0) & (~seen | ((De - Do) <= delta))) | (vg & (De > 0))
            inter, union, dist = vg & ve, vg | ve, np.abs(Dg - De)
            counts[n] = [vg.sum(), ve.sum(), inter.sum(), union.sum()] + [int((inter & (dist >= t)).sum()) for t in thr]

            def close(Dm):      # the visibility test (Dm - Do) <= delta is undecided
                return seen & (Dm > 0) & (np.abs((Dm - Do) - delta) <= slack(Dm, Do, delta))

            cg, ce = close(Dg), close(De)
            vis_any = cg | ce
            undecided[n, 0] = cg.sum()
            undecided[n, 1:4] = vis_any.sum()
            for t, th in enumerate(thr):
                near = (Dg > 0) & (De > 0) & (np.abs(dist - th) <= slack(Dg, De, th))
                undecided[n, 4 + t] = (vis_any | near).sum()
    return counts, undecided


def vsd_from_counts(counts):
    """(N, 4+T) counts -> (N, T) float64 vsd_t = (c_t + n_union - n_inter) / n_union, 1 where n_union == 0"""
    c = np.asarray(counts, np.int64)
    out = np.ones((len(c), c.shape[1] - 4))
    ok = c[:, 3] > 0
    out[ok] = (c[ok, 4:] + (c[ok, 3] - c[ok, 2])[:, None]) / c[ok, 3][:, None].astype(np.float64)
    return out


# ------------------------------------------------------------------ MSPD
def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def gt_times_symmetry(G, S):
    """M = G * S in float64, term by term as the header writes it -> (4,4) float64"""
    G, S = np.asarray(G, np.float64), np.asarray(S, np.float64)
    M = np.eye(4)
    for i in range(3):
        for j in range(3):
            M[i, j] = _dot3(G[i, 0], S[0, j], G[i, 1], S[1, j], G[i, 2], S[2, j])
        M[i, 3] = _dot3(G[i, 0], S[0, 3], G[i, 1], S[1, 3], G[i, 2], S[2, 3]) + G[i, 3]
    return M


def project32(T, pts, K):
    """(u, v, Z) float32 of the model points under the float32 transform T, in the header's order"""
    T, p, K = np.asarray(T, np.float32), np.asarray(pts, np.float32), np.asarray(K, np.float64).reshape(3, 3).astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    X, Y, Z = (((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3))
    u = (K[0, 0] * X) / Z + K[0, 2]
    v = (K[1, 1] * Y) / Z + K[1, 2]
    assert u.dtype == v.dtype == Z.dtype == np.float32
    return u, v, Z


def mspd(pts, poses, gt, K, gt_index=None, sym=None):
    """-> (N,) float64: the float32 restatement (the float32 maximum widened); NaN as the header says"""
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    gt = np.asarray(gt, np.float64).reshape(-1, 4, 4)
    syms = None if sym is None else np.asarray(sym, np.float64).reshape(-1, 4, 4)
    out = np.full(len(poses), np.nan)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for n, A in enumerate(poses):
            g = _gt_of(gt_index, len(gt), n)
            if g < 0 or not np.isfinite(A[:3]).all():
                continue
            Ms = [gt[g].astype(np.float32)] if syms is None or len(syms) == 0 else [gt_times_symmetry(gt[g], S).astype(np.float32) for S in syms]
            if not all(np.isfinite(M[:3]).all() for M in Ms):
                continue
            ua, va, Za = project32(A, pts, K)
            best, bad = np.float32(np.inf), not (Za > 0).all()
            for M in Ms:
                ub, vb, Zb = project32(M, pts, K)
                bad = bad or not (Zb > 0).all()
                du, dv = ua - ub, va - vb
                d = np.sqrt(du * du + dv * dv)
                assert d.dtype == np.float32
                if not bad:
                    best = min(best, d.max())
            if not bad:
                out[n] = float(best)
    return out


def mspd64(pts, pose, gt, K, sym=None):
    """one pose in float64 straight from the formula: min over s of the max pixel distance"""
    p = np.asarray(pts, np.float64)
    K = np.asarray(K, np.float64).reshape(3, 3)

    def proj(T):
        c = p @ T[:3, :3].T + T[:3, 3]
        return np.stack([K[0, 0] * c[:, 0] / c[:, 2] + K[0, 2], K[1, 1] * c[:, 1] / c[:, 2] + K[1, 2]], 1)
    a = proj(np.asarray(pose, np.float64))
    syms = [np.eye(4)] if sym is None else np.asarray(sym, np.float64).reshape(-1, 4, 4)
    return min(float(np.linalg.norm(a - proj(np.asarray(gt, np.float64) @ S), axis=1).max()) for S in syms)


def mspd_bound(pts, pose, gt, K, sym=None):
    """the bound of the float32 restatement against mspd64, from u = 2^-24 and the magnitudes, all evaluated in float64.  Per
    transform (R, t) and point p: X, Y, Z are three rounded products and three rounded additions, so each is within g4 (|R_i| . |p| +
    |t_i|) of the exact value with g4 = 4u / (1 - 4u); M_s is rounded once from float64, one more u on the same magnitudes (counted
    for both sides).  u_px = (fx X) / Z + cx: fx, cx are float32 roundings (u each), the product, the quotient and the sum round
    once each, so |d u_px| <= (fx / Z) dX + (fx |X| / Z^2) dZ + 3u |fx X / Z| + u |cx| + u |u_px|.  The distance: du is one rounded
    difference (u |du|), d = sqrtf(du*du + dv*dv) has two squares, a sum and a square root: within 3u d.  A maximum moves by at most
    the largest per-point error and a minimum by at most the largest per-transform one.  Second-order terms (products of two relative
    errors of <= 1e-6) are covered by the factor 1.01."""
    u = 2.0 ** -24
    g5 = 4 * u / (1 - 4 * u) + u
    p = np.asarray(pts, np.float64)
    K = np.asarray(K, np.float64).reshape(3, 3)

    def proj_err(T):
        c = p @ T[:3, :3].T + T[:3, 3]
        mag = np.abs(p) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])
        out = []
        for f, cc, i in ((K[0, 0], K[0, 2], 0), (K[1, 1], K[1, 2], 1)):
            q = f * c[:, i] / c[:, 2]
            out.append((q + cc, f / c[:, 2] * g5 * mag[:, i] + np.abs(q) / c[:, 2] * g5 * mag[:, 2] + 3 * u * np.abs(q) + u * abs(cc)
                        + u * np.abs(q + cc)))
        return out

    (ua, eua), (va, eva) = proj_err(np.asarray(pose, np.float64))
    worst = 0.0
    for S in ([np.eye(4)] if sym is None else np.asarray(sym, np.float64).reshape(-1, 4, 4)):
        (ub, eub), (vb, evb) = proj_err(np.asarray(gt, np.float64) @ S)
        du, dv = ua - ub, va - vb
        worst = max(worst, float((eua + eub + eva + evb + u * (np.abs(du) + np.abs(dv)) + 3 * u * np.hypot(du, dv)).max()))
    return 1.01 * worst
