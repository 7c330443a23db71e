"""CPU: the pose-error metrics without a GPU -- fp_pose_errors' argument errors through ctypes, the host record ops.PoseErrors, the
checks ops.pose_errors makes before any device work, and the numpy restatement of the definition (tests/pose_errors_model.py) that the
GPU tests compare the kernel with: against the float64 metrics of vis.add_err / vis.adds_err, and its own properties."""
import ctypes as C
import math

import numpy as np
import pytest

import pose_errors_model as pm


def _rot(axis, angle):
    """Rodrigues, float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _tf(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _can_pts():
    from foundationpose_amd.mesh import make_can_mesh
    v = np.asarray(make_can_mesh().vertices, np.float64)
    return (v - (v.min(0) + v.max(0)) / 2).astype(np.float32)


HALF_TURN = np.diag([-1.0, -1.0, 1.0, 1.0])          # about the can's axis (tests/test_io.py uses the same)


def test_argument_errors_are_reported_without_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)
    big = 1 << 40

    def call(pts=p, P=100, sym=None, S=0, poses=p, gt=p, gi=None, G=1, N=4, flags=3, out=p, ws=p, wsb=big):
        return lib.fp_pose_errors(pts, P, sym, S, poses, gt, gi, G, N, flags, out, ws, wsb, None)

    bad = [dict(pts=None), dict(poses=None), dict(gt=None), dict(out=None), dict(P=0), dict(P=(1 << 22) + 1), dict(N=-1), dict(N=65536),
           dict(G=0), dict(S=-1), dict(S=4097, sym=p), dict(S=2), dict(flags=4), dict(flags=0), dict(flags=8), dict(flags=11),
           dict(G=3), dict(ws=None), dict(wsb=lib.fp_pose_errors_workspace_bytes(4, 100, 0) - 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.fp_last_error().startswith(b"fp_pose_errors"), (kw, lib.fp_last_error())
    assert b"gt_index is NULL" in (call(G=3), lib.fp_last_error())[1]
    assert b"workspace" in (call(wsb=16), lib.fp_last_error())[1]
    assert b"FP_ERR_SYM" in (call(flags=5), lib.fp_last_error())[1]
    # N == 0 does nothing, with NULL tensors and no workspace; the argument checks that do not depend on N still hold
    assert call(N=0, pts=None, poses=None, gt=None, out=None, ws=None, wsb=0) == 0
    assert call(N=0, G=0) == -1 and call(N=0, flags=0) == -1
    wb = lib.fp_pose_errors_workspace_bytes
    assert wb(0, 100, 3) == 0
    for S in (0, 1, 6):
        for P in (1, 63, 256, 257, 2501, 32767, 32768, 100000):
            sizes = [wb(N, P, S) for N in (1, 2, 3, 252, 65535)]
            assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (S, P, sizes)
        for N in (1, 252):
            sizes = [wb(N, P, S) for P in range(1, 70000, 97)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (S, N)
        assert wb(3, 1 << 22, S) > wb(3, 100000, S)


def test_pose_errors_record():
    from foundationpose_amd.ops import PoseErrors
    rows = PoseErrors.rows(np.asarray([[0.01, 0.005, np.nan, np.nan], [1.0, 2.0, 3.0, 4.0]]))
    assert rows[1] == PoseErrors(1.0, 2.0, 3.0, 4.0) and rows[1].mssd == 4.0
    assert rows[0].add == 0.01 and rows[0].adds == 0.005 and math.isnan(rows[0].add_sym) and math.isnan(rows[0].mssd)
    assert all(type(x) is float for x in rows[0]) and PoseErrors._fields == ("add", "adds", "add_sym", "mssd")
    import torch
    assert PoseErrors.rows(torch.zeros(3, 4, dtype=torch.float64)) == [PoseErrors(0.0, 0.0, 0.0, 0.0)] * 3


def test_wrapper_refuses_before_device_work():
    import torch
    from foundationpose_amd import _lib, ops
    pts, poses, gt = torch.zeros(5, 3), torch.eye(4)[None].repeat(2, 1, 1), np.eye(4)
    with pytest.raises(ValueError, match="unknown name"):
        ops.pose_errors(pts, poses, gt, want=("add", "mssd"))
    with pytest.raises(ValueError, match="empty"):
        ops.pose_errors(pts, poses, gt, want=())
    with pytest.raises(_lib.FpAmdError, match="CUDA"):
        ops.pose_errors(pts, poses, gt)
    with pytest.raises(_lib.FpAmdError, match="CUDA"):
        ops.pose_errors(pts, poses, gt, want="adds")
    # wrong shapes and tables are refused before the device check (CPU tensors throughout: none of these gets as far as "CUDA")
    eye = torch.eye(4)
    for kw, msg in ((dict(model_pts=torch.zeros(5, 4)), r"model_pts must be \(P,3\)"),
                    (dict(model_pts=torch.zeros(0, 3)), r"model_pts must be \(P,3\)"),
                    (dict(model_pts=torch.zeros(15)), r"model_pts must be \(P,3\)"),
                    (dict(model_pts=np.zeros((5, 3), np.float32)), "model_pts must be a tensor"),
                    (dict(poses=eye), r"poses must be \(N,4,4\)"),
                    (dict(poses=torch.zeros(2, 3, 4)), r"poses must be \(N,4,4\)"),
                    (dict(poses=np.eye(4)[None]), "poses must be a tensor"),
                    (dict(gt=np.eye(3)), r"gt must be \(4,4\) or \(n,4,4\)"),
                    (dict(gt=torch.zeros(2, 2, 4, 4)), r"gt must be \(4,4\) or \(n,4,4\)"),
                    (dict(gt=np.zeros((0, 4, 4))), "0 ground truths"),
                    (dict(gt=np.eye(4).astype(complex)), "gt must be of a float type"),
                    (dict(gt=torch.eye(4, dtype=torch.int64)), "gt must be of a float type"),
                    (dict(gt=np.stack([np.eye(4)] * 3)), "3 ground truths for 2 poses need a gt_index"),
                    (dict(gt_index=torch.zeros(3, dtype=torch.int32)), "gt_index tensor of 2 entries"),
                    (dict(gt_index=[0, 0]), "gt_index tensor of 2 entries"),
                    (dict(want=("add", "sym")), 'want "sym" needs symmetry_tfs'),
                    (dict(want="sym", symmetry_tfs=np.zeros((0, 4, 4))), 'want "sym" needs symmetry_tfs'),
                    (dict(symmetry_tfs=np.eye(4)[:3]), r"symmetry_tfs must be \(4,4\) or \(n,4,4\)"),
                    (dict(symmetry_tfs=torch.zeros(2, 4, 4, dtype=torch.int32)), "symmetry_tfs must be of a float type")):
        args = dict(model_pts=pts, poses=poses, gt=gt)
        args.update(kw)
        with pytest.raises(_lib.FpAmdError, match=msg):
            ops.pose_errors(**args)
    # three ground truths with an index of the right length, integer tables that are exact: past the shape checks, refused as CPU tensors
    with pytest.raises(_lib.FpAmdError, match="CUDA"):
        ops.pose_errors(pts, poses, np.stack([np.eye(4)] * 3), gt_index=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.FpAmdError, match="CUDA"):
        ops.pose_errors(pts, poses, np.eye(4, dtype=np.int64), symmetry_tfs=np.eye(4), want=("add", "sym"))
    from foundationpose_amd.estimater import FoundationPose
    est = object.__new__(FoundationPose)          # no state at all: no registration either
    with pytest.raises(RuntimeError, match="no registration"):
        est.pose_errors(np.eye(4))
    with pytest.raises(ValueError, match="unknown metric"):
        est.hypothesis_report(np.eye(4), metric="addx")
    assert "pose_errors" in FoundationPose.compute_add_err_to_gt_pose.__doc__


GRID_ROT = (0.0, 1e-4, 1e-2, 0.3, math.pi)
GRID_TRANS = (0.0, 1e-5, 1e-3, 0.05, 1.0)


def _grid_cases(pts):
    """(pose float32, gt float64) over the issue's grid: ground truths 0.4-1.5 m from the camera, the predicted pose = the ground truth
    turned by the rotation offset about a seeded axis and moved by the translation offset along a seeded direction, rounded to
    float32"""
    rng = np.random.default_rng(7)
    for ir, ang in enumerate(GRID_ROT):
        for it, off in enumerate(GRID_TRANS):
            k = ir * len(GRID_TRANS) + it
            dist = 0.4 + 1.1 * k / (len(GRID_ROT) * len(GRID_TRANS) - 1)
            direction = np.array([0.2 * math.cos(k), 0.15 * math.sin(k), 1.0])
            gt = _tf(_rot(rng.normal(size=3), rng.uniform(0, math.pi)), dist * direction / np.linalg.norm(direction))
            u = rng.normal(size=3)
            pred = _tf(_rot(rng.normal(size=3), ang) @ gt[:3, :3], gt[:3, 3] + off * u / np.linalg.norm(u)).astype(np.float32)
            yield (ang, off), pred, gt


def test_restatement_against_float64_metrics():
    """the restatement's add / adds against vis.add_err / vis.adds_err (float64, KD-tree) within the bound
    8 * 2^-24 * (|t_rel| + 2 r_max) + 2 * delta * vis over the 5 x 5 grid"""
    from foundationpose_amd import vis
    pts = _can_pts()
    assert pts.shape == (2501, 3)
    worst = 0.0
    for key, pred, gt in _grid_cases(pts):
        got = pm.pose_errors(pts, pred[None], gt[None])[0]
        for col, ref in ((0, vis.add_err(pred.astype(np.float64), gt, pts.astype(np.float64))),
                         (1, vis.adds_err(pred.astype(np.float64), gt, pts.astype(np.float64)))):
            bound = pm.bound_vs_float64(pred, gt, pts, ref)
            err = abs(got[col] - ref)
            _, t = pm.relative_tf(pred, gt)
            unit = 2.0 ** -24 * (np.linalg.norm(t) + 2 * np.linalg.norm(pts.astype(np.float64), axis=1).max())
            worst = max(worst, err / unit)
            print(f"rot {key[0]:g} trans {key[1]:g} col {col}: model {got[col]:.9e} vis {ref:.9e} |diff| {err:.2e} bound {bound:.2e}")
            assert err <= bound, (key, col, got[col], ref, bound)
    print(f"worst |diff| / (2^-24 (|t_rel| + 2 r_max)) = {worst:.3f}")


def test_restatement_properties():
    pts = _can_pts()
    ident = np.eye(4)[None]
    sym = np.stack([np.eye(4), HALF_TURN])
    for key, pred, gt in list(_grid_cases(pts))[::3]:
        r1 = pm.pose_errors(pts, pred[None], gt[None], sym=ident, flags=7)[0]
        assert r1[2] == r1[0], (key, r1)                      # identity-only symmetry: add_sym == add exactly
        r = pm.pose_errors(pts, pred[None], gt[None], sym=sym, flags=7)[0]
        assert r[0] == r1[0] and r[1] == r1[1]
        assert r[1] <= r[0] and r[2] <= r[0], (key, r)          # i = j and the identity are in the sets the minima run over
        assert r[3] >= r[2] * (1 - 1e-12), (key, r)
    # a half-turned pose of the can: invisible to add_sym with the half turn in the set, centimetres to add
    gt = _tf(_rot([0.3, -0.5, 0.8], 0.9), [0.05, -0.02, 0.7])
    flipped = (gt @ HALF_TURN).astype(np.float32)
    r = pm.pose_errors(pts, flipped[None], gt[None], sym=sym, flags=7)[0]
    assert r[2] < 1e-6 and r[0] > 0.01 and r[3] < 1e-6 and r[1] < 1e-6, r
    # equal poses: ~1e-8 m (float32 per-point arithmetic), not 0; an index out of range: NaN in every column
    same = pm.pose_errors(pts, gt.astype(np.float32)[None], gt.astype(np.float32).astype(np.float64)[None])[0]
    assert 0 <= same[0] < 1e-7 and 0 <= same[1] <= same[0]
    rows = pm.pose_errors(pts[:50], np.stack([flipped] * 3), gt[None], gt_index=[0, 1, -1], sym=sym, flags=7)
    assert np.isfinite(rows[0]).all() and np.isnan(rows[1:]).all()
