"""The numpy restatement of fp_pose_errors' definition (include/fp_amd.h) that the pose-error tests compare the kernel with: the relative
transform T = inv(pose) * gt term by term in float64 and rounded to float32, every per-point value in float32 in the order the header
writes it, the sums exactly rounded (math.fsum)."""
import math

import numpy as np

FLAG_ADD, FLAG_ADDS, FLAG_SYM = 1, 2, 4


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def relative_tf(pose, gt):
    """T = inv(pose) * gt in float64 -> (R (3,3), t (3,)) float64; pose as the float32 values the kernel reads"""
    A = np.asarray(pose, np.float32).astype(np.float64)
    B = np.asarray(gt, np.float64)
    d = [B[0, 3] - A[0, 3], B[1, 3] - A[1, 3], B[2, 3] - A[2, 3]]
    R, t = np.empty((3, 3)), np.empty(3)
    for i in range(3):
        for j in range(3):
            R[i, j] = _dot3(A[0, i], B[0, j], A[1, i], B[1, j], A[2, i], B[2, j])
        t[i] = _dot3(A[0, i], d[0], A[1, i], d[1], A[2, i], d[2])
    return R, t


def times_symmetry(R, t, S):
    """T * S in float64 -> (R, t)"""
    S = np.asarray(S, np.float64)
    Rs, ts = np.empty((3, 3)), np.empty(3)
    for i in range(3):
        for j in range(3):
            Rs[i, j] = _dot3(R[i, 0], S[0, j], R[i, 1], S[1, j], R[i, 2], S[2, j])
        ts[i] = _dot3(R[i, 0], S[0, 3], R[i, 1], S[1, 3], R[i, 2], S[2, 3]) + t[i]
    return Rs, ts


def transform_pts(R, t, pts):
    """q_j = ((R0*x + R1*y) + R2*z) + t in float32 -> (P,3) float32"""
    R, t, p = np.asarray(R, np.float64).astype(np.float32), np.asarray(t, np.float64).astype(np.float32), np.asarray(pts, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    q = np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)], 1)
    assert q.dtype == np.float32
    return q


def _dist2(q, p):
    dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
    r = (dx * dx + dy * dy) + dz * dz
    assert r.dtype == np.float32
    return r


def point_distances(R, t, pts):
    """d_j (P,) float32: distance of q_j to its own model point"""
    p = np.asarray(pts, np.float32)
    return np.sqrt(_dist2(transform_pts(R, t, p), p))


def nearest_distances(R, t, pts, block=256):
    """e_j (P,) float32: distance of q_j to the nearest model point, the squared distances computed directly"""
    p = np.asarray(pts, np.float32)
    q = transform_pts(R, t, p)
    best = np.empty(len(p), np.float32)
    for a in range(0, len(p), block):
        best[a:a + block] = _dist2(q[a:a + block, None, :], p[None, :, :]).min(1)
    return np.sqrt(best)


def _mean(v):
    return math.fsum(float(x) for x in v) / len(v)


def pose_errors(pts, poses, gt, gt_index=None, sym=None, flags=FLAG_ADD | FLAG_ADDS):
    """-> (N, 4) float64 [add, adds, add_sym, mssd]; NaN where a column is not selected, the ground-truth index is out of range or the
    transform is not finite"""
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    gt = np.asarray(gt, np.float64).reshape(-1, 4, 4)
    N, G = len(poses), len(gt)
    out = np.full((N, 4), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):         # non-finite input is part of the definition: NaN rows, no warning
        _fill(out, pts, poses, gt, gt_index, sym, flags)
    return out


def _fill(out, pts, poses, gt, gt_index, sym, flags):
    N, G = len(poses), len(gt)
    for n in range(N):
        g = int(gt_index[n]) if gt_index is not None else (0 if G == 1 else n)
        if not 0 <= g < G:
            continue
        R, t = relative_tf(poses[n], gt[g])
        if not (np.isfinite(R.astype(np.float32)).all() and np.isfinite(t.astype(np.float32)).all()):
            continue                                           # a T that is not finite in float32: NaN in every column
        if flags & FLAG_ADD:
            out[n, 0] = _mean(point_distances(R, t, pts))
        if flags & FLAG_ADDS:
            out[n, 1] = _mean(nearest_distances(R, t, pts))
        if flags & FLAG_SYM:
            tfs = [times_symmetry(R, t, S) for S in np.asarray(sym, np.float64).reshape(-1, 4, 4)]
            if all(np.isfinite(Rs.astype(np.float32)).all() and np.isfinite(ts.astype(np.float32)).all() for Rs, ts in tfs):
                ds = [point_distances(Rs, ts, pts) for Rs, ts in tfs]       # (a T_s that is not finite: add_sym and mssd stay NaN)
                out[n, 2] = min(_mean(d) for d in ds)
                out[n, 3] = min(float(d.max()) for d in ds)


def bound_vs_float64(pose, gt, pts, value):
    """the issue's bound of a float32-per-point metre value against the float64 metric `value` (vis.add_err / vis.adds_err):
    8 * 2^-24 * (|t_rel| + 2 r_max) + 2 * delta * value, delta = max |R^T R - I| of the predicted rotation, all in float64"""
    Rp = np.asarray(pose, np.float32).astype(np.float64)[:3, :3]
    _, t = relative_tf(pose, gt)
    r_max = float(np.linalg.norm(np.asarray(pts, np.float64), axis=1).max())
    delta = float(np.abs(Rp.T @ Rp - np.eye(3)).max())
    return 8 * 2.0 ** -24 * (float(np.linalg.norm(t)) + 2 * r_max) + 2 * delta * float(value)
