"""CPU: BOP's pose errors without a GPU -- the numpy restatement of fp_vsd_counts and fp_mspd (tests/bop_errors_model.py) that the GPU
tests compare the kernels with: its properties on the scene (depth maps from the CPU oracle's full-frame render), the float32
restatement against a float64 evaluation of the formulas within bounds derived from the float32 rounding of the operands, the recalls of
vis.bop_recall / bop_average_recall on hand-made lists, the host record ops.VsdCounts, every refusal of the wrappers that needs no
device, and the C entry points' argument errors."""
import ctypes as C
import math

import numpy as np
import pytest

import bop_errors_model as bm
from test_pose_errors_host import HALF_TURN, _can_pts, _grid_cases, _rot, _tf

H, W = 480, 640


def _render(scene, poses):
    """full-frame depth maps (n,H,W) float32 of the scene's mesh at float32 poses, by the CPU oracle"""
    from oracle import ops as oo
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    return oo.render_crops(scene["mesh_np"], poses, None, scene["K"], H, W, (H, W), normalize_xyz=False, want=("depth",))["depth"]


@pytest.fixture(scope="module")
def maps(scene):
    """the scene's observed depth, the render of its ground truth and of the 252 grid poses, the factor and BOP's thresholds"""
    gt = _render(scene, scene["gt"])
    return dict(obs=np.asarray(scene["depth"], np.float32), gt=gt, est=_render(scene, scene["poses"]),
                fac=bm.dist_factor(scene["K"], H, W), thr=bm.thresholds(bm.BOP_TAUS, scene["diameter"]))


def _counts(maps, est, obs=None, gt=None):
    return bm.vsd_counts(est, maps["gt"] if gt is None else gt, maps["obs"] if obs is None else obs, maps["fac"], bm.BOP_DELTA, maps["thr"])


# ------------------------------------------------------------------ 1. properties of the restatement on the scene
def test_ground_truth_against_itself(maps):
    c = _counts(maps, maps["gt"])[0]
    print("gt against itself:", c.tolist())
    assert c[0] == c[1] == c[2] == c[3] > 20000 and (c[4:] == 0).all()
    assert (bm.vsd_from_counts(c[None]) == 0).all()
    assert len(c) == 4 + 10 and maps["thr"].dtype == np.float32 and maps["fac"].dtype == np.float32
    assert maps["fac"].min() >= 1.0 and maps["fac"][240, 320] < 1.001 and maps["fac"][0, 0] > maps["fac"][0, 1]


def test_sideways_shift_has_no_intersection(scene, maps):
    T = np.asarray(scene["gt"], np.float64).copy()
    T[0, 3] += 0.2
    c = _counts(maps, _render(scene, T))[0]
    print("0.2 m sideways:", c.tolist())
    assert c[2] == 0 and c[3] == c[0] + c[1] and c[1] > 0 and (c[4:] == 0).all()
    assert (bm.vsd_from_counts(c[None]) == 1.0).all()
    # nothing rendered at all, and nothing visible at all: VSD is 1 by definition
    empty = np.zeros((1, H, W), np.float32)
    c = _counts(maps, empty)[0]
    assert c[1] == 0 and c[2] == 0 and c[3] == c[0] and (bm.vsd_from_counts(c[None]) == 1.0).all()
    c = bm.vsd_counts(empty, empty, maps["obs"], maps["fac"], bm.BOP_DELTA, maps["thr"])[0]
    assert (c == 0).all() and (bm.vsd_from_counts(c[None]) == 1.0).all()


def test_estimate_beyond_delta_is_kept_by_the_ground_truth(scene, maps):
    """+0.03 m along z puts the estimate more than delta behind the observed surface: its own visibility test fails wherever the
    sensor measured, and it stays visible only where the ground truth is (ve = vis(De) or (vg and De > 0))"""
    T = np.asarray(scene["gt"], np.float64).copy()
    T[2, 3] += 0.03
    est = _render(scene, T)
    c = _counts(maps, est)[0]
    print("+0.03 m along z:", c.tolist())
    assert 0 < c[1] < c[0] and c[4] == c[2] > 0
    # without the ground truth's help nothing of it is visible where the object was observed
    alone = bm.vsd_counts(est, np.zeros((1, H, W), np.float32), maps["obs"], maps["fac"], bm.BOP_DELTA, maps["thr"])[0]
    print("the same estimate against an empty ground truth:", alone.tolist())
    assert alone[0] == 0 and alone[1] < c[1]


def test_vsd_does_not_increase_with_tau(maps):
    c = _counts(maps, maps["est"])
    v = bm.vsd_from_counts(c)
    print("vsd of the 252 grid poses: tau 0.05 min/mean/max", v[:, 0].min(), v[:, 0].mean(), v[:, 0].max(), "tau 0.5", v[:, -1].min(), v[:, -1].max())
    assert v.shape == (252, 10) and (np.diff(v, axis=1) <= 0).all() and (v >= 0).all() and (v <= 1).all()
    assert (np.diff(c[:, 4:], axis=1) <= 0).all() and (c[:, 4] <= c[:, 2]).all() and (c[:, 2] <= np.minimum(c[:, 0], c[:, 1])).all()
    assert (c[:, 3] == c[:, 0] + c[:, 1] - c[:, 2]).all()


def test_holes_occluders_and_invalid_measurements(maps):
    base = _counts(maps, maps["gt"])[0]
    ys, xs = np.nonzero(maps["gt"][0] > 0)
    cy, cx = int(ys.mean()), int(xs.mean())
    blk = (slice(cy - 10, cy + 10), slice(cx - 8, cx + 8))
    covered = int((maps["gt"][0][blk] > 0).sum())
    assert covered > 100
    for hole in (0.0, -1.0, np.nan, -np.inf):                 # no measurement: the surface under it stays visible
        obs = maps["obs"].copy()
        obs[blk] = hole
        assert np.array_equal(_counts(maps, maps["gt"], obs=obs)[0], base), hole
    obs = maps["obs"].copy()                                  # something 0.1 m in front: exactly its pixels leave
    obs[blk] = maps["obs"][blk] - np.float32(0.1)
    covered = int(((maps["gt"][0][blk] > 0) & (obs[blk] > 0)).sum())      # (the frame's own holes in the block stay holes)
    occ = _counts(maps, maps["gt"], obs=obs)[0]
    print("occluder over", covered, "object pixels:", base.tolist()[:4], "->", occ.tolist()[:4])
    assert (occ[:4] == base[:4] - covered).all() and (occ[4:] == 0).all()
    # the whole map negative / NaN is the whole map 0
    none = _counts(maps, maps["est"][:3], obs=np.zeros_like(maps["obs"]))
    for bad in (-1.0, np.nan):
        assert np.array_equal(_counts(maps, maps["est"][:3], obs=np.full_like(maps["obs"], bad)), none)
    assert (none[:, 0] == int((maps["gt"][0] > 0).sum())).all()


def test_window_index_and_out_of_range_rows(maps):
    """a window of the frame at an origin counts what the full frame counts when it holds the object; gt_index picks the ground truth"""
    ys, xs = np.nonzero((maps["gt"][0] > 0) | (maps["est"][:4] > 0).any(0))
    y0, y1, x0, x1 = ys.min() - 1, ys.max() + 2, xs.min() - 3, xs.max() + 2
    full = _counts(maps, maps["est"][:4])
    win = bm.vsd_counts(maps["est"][:4, y0:y1, x0:x1], maps["gt"][:, y0:y1, x0:x1], maps["obs"], maps["fac"], bm.BOP_DELTA, maps["thr"],
                        origin=(x0, y0))
    assert np.array_equal(full, win)
    two = np.concatenate([maps["gt"], maps["est"][:1]])
    rows = bm.vsd_counts(maps["est"][:4], two, maps["obs"], maps["fac"], bm.BOP_DELTA, maps["thr"], gt_index=[0, 1, 2, -1])
    assert np.array_equal(rows[0], full[0]) and (rows[2:] == -1).all() and rows[1, 0] != full[1, 0]


# ------------------------------------------------------------------ 2. float32 against float64
def test_vsd_float32_against_float64_on_the_grid(scene, maps):
    """the counts of the float32 restatement against BOP's float64 arithmetic: they may differ only at pixels where a comparison is
    decided by less than the float32 rounding of its operands (bop_errors_model.vsd_counts64 counts them per column)"""
    c32 = _counts(maps, maps["est"]).astype(np.int64)
    c64, undecided = bm.vsd_counts64(maps["est"], maps["gt"][0], maps["obs"], scene["K"], bm.BOP_DELTA, bm.BOP_TAUS, scene["diameter"])
    diff = np.abs(c32 - c64)
    print("columns: largest |count32 - count64|", diff.max(0).tolist(), "largest number of undecided pixels", undecided.max(0).tolist())
    print("poses with a difference:", int((diff > 0).any(1).sum()), "of 252; undecided pixels in all:", int(undecided.sum()))
    assert (diff <= undecided).all(), np.argwhere(diff > undecided)


def test_mspd_float32_against_float64():
    from foundationpose_amd import synthetic as syn
    from foundationpose_amd import vis
    pts, K = _can_pts(), syn.YCBV_K
    sym = np.stack([np.eye(4), HALF_TURN, _tf(_rot([0, 0, 1], 0.5), [0, 0, 0.001])])
    worst = 0.0
    for key, pred, gt in _grid_cases(pts):
        for s in (None, sym):
            got = bm.mspd(pts, pred[None], gt[None], K, sym=s)[0]
            zmin = min((pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3])[:, 2].min()
                       for T in [pred.astype(np.float64)] + [gt @ S for S in ([np.eye(4)] if s is None else s)])
            if zmin <= 0.05:        # at or near the camera plane: NaN by definition once a point is behind it, no bound in front of it
                assert zmin > -1e-6 or math.isnan(got), (key, zmin, got)
                continue
            ref, bound = bm.mspd64(pts, pred.astype(np.float64), gt, K, s), bm.mspd_bound(pts, pred.astype(np.float64), gt, K, s)
            worst = max(worst, abs(got - ref) / bound)
            print(f"rot {key[0]:g} trans {key[1]:g} sym {s is not None}: model {got:.6f} px float64 {ref:.6f} px |diff| {abs(got - ref):.2e} bound {bound:.2e}")
            assert abs(got - ref) <= bound, (key, got, ref, bound)
            if s is not None:
                assert got <= bm.mspd(pts, pred[None], gt[None], K)[0]          # the identity is in the set
    print(f"worst |diff| / bound = {worst:.3f}")
    # the float64 formula is vis.project_3d_to_2d's before it rounds to whole pixels: one point, directly
    _, pred, gt = list(_grid_cases(pts))[7]
    p = np.append(pts[17].astype(np.float64), 1.0)
    a, b = vis.project_3d_to_2d(p, K, pred.astype(np.float64)), vis.project_3d_to_2d(p, K, gt)
    one = bm.mspd64(pts[17:18], pred.astype(np.float64), gt, K)
    assert abs(one - np.linalg.norm(a - b)) <= math.sqrt(2) + 1e-9      # each coordinate rounds by at most half a pixel
    # a half-turned can is invisible to MSPD with the half turn in the set
    gt = _tf(_rot([0.3, -0.5, 0.8], 0.9), [0.05, -0.02, 0.7])
    flipped = (gt @ HALF_TURN).astype(np.float32)
    assert bm.mspd(pts, flipped[None], gt[None], K, sym=sym)[0] < 1e-2 < 10 < bm.mspd(pts, flipped[None], gt[None], K)[0]


def test_mspd_nan_rows():
    from foundationpose_amd import synthetic as syn
    pts, K = _can_pts()[:200], syn.YCBV_K
    gt = _tf(_rot([0.3, -0.5, 0.8], 0.9), [0.05, -0.02, 0.7])
    good = gt.astype(np.float32)
    behind, nan_pose, inf_pose = good.copy(), good.copy(), good.copy()
    behind[2, 3] = 0.01            # the camera plane cuts the object
    nan_pose[0, 0], inf_pose[1, 3] = np.nan, np.inf
    rows = bm.mspd(pts, np.stack([good, behind, nan_pose, inf_pose, good, good]), np.stack([gt, gt]), K, gt_index=[0, 0, 0, 0, 2, -1])
    assert rows[0] < 1e-3 and np.isnan(rows[1:]).all(), rows
    bad_gt = gt.copy()
    bad_gt[2, 3] = -0.7
    assert np.isnan(bm.mspd(pts, good[None], bad_gt[None], K)[0])
    sym = np.stack([np.eye(4), _tf(np.eye(3), [0, 0, np.nan])])
    assert np.isnan(bm.mspd(pts, good[None], gt[None], K, sym=sym)[0])


# ------------------------------------------------------------------ 3. recall
def test_bop_recall_on_hand_made_lists():
    from foundationpose_amd import vis
    thetas = vis.BOP_THETAS
    assert len(thetas) == 10 and abs(thetas[0] - 0.05) < 1e-15 and abs(thetas[-1] - 0.5) < 1e-15
    assert vis.bop_recall([0.0, 0.01, 0.049], thetas) == 1.0                    # all correct under every threshold
    assert vis.bop_recall([0.5, 0.7, 1.0, np.inf], thetas) == 0.0               # none: e < theta is strict
    assert vis.bop_recall([0.07], thetas) == pytest.approx(0.9)                 # fails theta = 0.05 only
    assert vis.bop_recall([0.07, 0.12], thetas) == pytest.approx((0.9 + 0.8) / 2)
    assert vis.bop_recall([0.0, np.nan], thetas) == 0.5                         # NaN is an incorrect pose
    assert vis.bop_recall(np.zeros((3, 10)), thetas) == 1.0 and math.isnan(vis.bop_recall([], thetas))
    ar = vis.bop_average_recall(np.zeros((2, 10)), [0.0, 0.31], [4.9, 1000.0], 640)
    assert ar["AR_VSD"] == 1.0 and ar["AR_MSSD"] == pytest.approx((1.0 + 0.4) / 2) and ar["AR_MSPD"] == 0.5
    assert ar["AR"] == pytest.approx((1.0 + 0.7 + 0.5) / 3) and sorted(ar) == ["AR", "AR_MSPD", "AR_MSSD", "AR_VSD"]
    # the pixel thresholds scale with the image width: 9 px is under 5r only for r = 2
    assert vis.bop_average_recall(np.zeros((1, 10)), [0.0], [9.0], 640)["AR_MSPD"] == pytest.approx(0.9)
    assert vis.bop_average_recall(np.zeros((1, 10)), [0.0], [9.0], 1280)["AR_MSPD"] == 1.0
    # VSD pools poses and taus: one pose, half of its taus beyond every theta
    v = np.array([[0.0] * 5 + [1.0] * 5])
    assert vis.bop_average_recall(v, [0.0], [0.0], 640)["AR_VSD"] == 0.5


# ------------------------------------------------------------------ 4. the host record and the refusals
def test_vsd_counts_record():
    import torch
    from foundationpose_amd.ops import VsdCounts
    rows = VsdCounts.rows(np.asarray([[10, 8, 6, 12, 6, 3, 0], [0, 0, 0, 0, 0, 0, 0]], np.int32))
    assert rows[0] == VsdCounts(10, 8, 6, 12, (6, 3, 0)) and rows[0].n_union == 12 and VsdCounts._fields[:4] == ("n_gt_vis", "n_est_vis", "n_inter", "n_union")
    assert np.array_equal(rows[0].errors(), [1.0, 0.75, 0.5]) and rows[0].errors().dtype == np.float64
    assert np.array_equal(rows[1].errors(), [1.0, 1.0, 1.0])
    assert np.array_equal(np.stack([r.errors() for r in rows]), bm.vsd_from_counts([[10, 8, 6, 12, 6, 3, 0], [0] * 7]))
    assert VsdCounts.rows(torch.zeros(3, 5, dtype=torch.int32)) == [VsdCounts(0, 0, 0, 0, (0,))] * 3


def test_wrappers_refuse_before_device_work():
    import torch
    from foundationpose_amd import _lib, ops
    from foundationpose_amd import synthetic as syn
    K = syn.YCBV_K
    est, gt, obs = torch.zeros(3, 8, 12), torch.zeros(1, 8, 12), torch.zeros(8, 12)
    skew = K.copy()
    skew[0, 1] = 0.5
    for kw, exc, msg in ((dict(est_depth=np.zeros((3, 8, 12), np.float32)), _lib.FpAmdError, "est_depth must be a tensor"),
                         (dict(est_depth=torch.zeros(8, 12)), _lib.FpAmdError, r"est_depth must be \(n,h,w\)"),
                         (dict(gt_depth=torch.zeros(8, 12)), _lib.FpAmdError, r"gt_depth must be \(n,h,w\)"),
                         (dict(obs_depth=torch.zeros(1, 8, 12)), _lib.FpAmdError, r"obs_depth must be \(H,W\)"),
                         (dict(est_depth=torch.zeros(3, 0, 12), gt_depth=torch.zeros(1, 0, 12)), _lib.FpAmdError, "empty images"),
                         (dict(gt_depth=torch.zeros(1, 8, 11)), _lib.FpAmdError, r"gt_depth must be \(G,8,12\)"),
                         (dict(obs_depth=torch.zeros(8, 11)), _lib.FpAmdError, "not inside the 8 x 11 frame"),
                         (dict(origin=(1, 0)), _lib.FpAmdError, "not inside"),
                         (dict(origin=(0, -1)), _lib.FpAmdError, "not inside"),
                         (dict(origin=3), _lib.FpAmdError, "origin must be"),
                         (dict(gt_depth=torch.zeros(2, 8, 12)), _lib.FpAmdError, "2 ground truths for 3 maps need a gt_index"),
                         (dict(gt_depth=torch.zeros(0, 8, 12)), _lib.FpAmdError, "0 ground truths"),
                         (dict(gt_index=[0, 0, 0]), _lib.FpAmdError, "gt_index tensor of 3 entries"),
                         (dict(gt_index=torch.zeros(2, dtype=torch.int32)), _lib.FpAmdError, "gt_index tensor of 3 entries"),
                         (dict(taus=()), ValueError, "0 taus"),
                         (dict(taus=[0.1] * 17), ValueError, "17 taus"),
                         (dict(taus=[0.1, np.nan]), ValueError, "taus must be finite"),
                         (dict(taus=[0.1, -0.1]), ValueError, "taus must be finite"),
                         (dict(taus=[np.inf]), ValueError, "taus must be finite"),
                         (dict(delta=-0.01), ValueError, "delta must be finite"),
                         (dict(delta=np.nan), ValueError, "delta must be finite"),
                         (dict(delta=np.inf), ValueError, "delta must be finite"),
                         (dict(diameter=0.0), ValueError, "diameter must be finite"),
                         (dict(diameter=np.nan), ValueError, "diameter must be finite"),
                         (dict(diameter=1e39, taus=[1.0]), ValueError, "beyond float32"),
                         (dict(K=skew), ValueError, "skew"),
                         (dict(K=np.eye(2)), ValueError, "9 entries"),
                         (dict(K=np.diag([0.0, 1.0, 1.0])), ValueError, "positive focal"),
                         (dict(), _lib.FpAmdError, "CUDA"),                                   # everything right but the device
                         (dict(taus=[0.1] * 16, gt_depth=torch.zeros(3, 8, 12)), _lib.FpAmdError, "CUDA"),
                         (dict(est_depth=torch.zeros(3, 4, 4), gt_depth=torch.zeros(1, 4, 4), origin=(8, 4)), _lib.FpAmdError, "CUDA")):
        args = dict(est_depth=est, gt_depth=gt, obs_depth=obs, K=K, diameter=0.2)
        args.update(kw)
        with pytest.raises(exc, match=msg):
            ops.vsd_counts(**args)
    pts, poses, g = torch.zeros(5, 3), torch.eye(4)[None].repeat(2, 1, 1), np.eye(4)
    for kw, exc, msg in ((dict(model_pts=torch.zeros(5, 4)), _lib.FpAmdError, r"mspd: model_pts must be \(P,3\)"),
                         (dict(model_pts=np.zeros((5, 3), np.float32)), _lib.FpAmdError, "model_pts must be a tensor"),
                         (dict(poses=torch.eye(4)), _lib.FpAmdError, r"mspd: poses must be \(N,4,4\)"),
                         (dict(gt=np.eye(3)), _lib.FpAmdError, r"mspd: gt must be \(4,4\) or \(n,4,4\)"),
                         (dict(gt=np.zeros((0, 4, 4))), _lib.FpAmdError, "0 ground truths"),
                         (dict(gt=np.stack([np.eye(4)] * 3)), _lib.FpAmdError, "3 ground truths for 2 poses need a gt_index"),
                         (dict(gt_index=[0, 0]), _lib.FpAmdError, "gt_index tensor of 2 entries"),
                         (dict(symmetry_tfs=np.eye(4)[:3]), _lib.FpAmdError, r"mspd: symmetry_tfs must be \(4,4\) or \(n,4,4\)"),
                         (dict(symmetry_tfs=torch.zeros(2, 4, 4, dtype=torch.int32)), _lib.FpAmdError, "symmetry_tfs must be of a float type"),
                         (dict(K=skew), ValueError, "mspd: K has a skew"),
                         (dict(K=np.zeros(8)), ValueError, "9 entries"),
                         (dict(), _lib.FpAmdError, "CUDA"),
                         (dict(symmetry_tfs=np.stack([np.eye(4)] * 2), gt_index=torch.zeros(2, dtype=torch.int32)), _lib.FpAmdError, "CUDA")):
        args = dict(model_pts=pts, poses=poses, gt=g, K=K)
        args.update(kw)
        with pytest.raises(exc, match=msg):
            ops.mspd(**args)
    # pose_errors' own messages keep its name
    with pytest.raises(_lib.FpAmdError, match=r"pose_errors: gt must be \(4,4\)"):
        ops.pose_errors(pts, poses, np.eye(3))
    from foundationpose_amd.estimater import FoundationPose
    e = object.__new__(FoundationPose)          # no state at all: no registration either
    with pytest.raises(RuntimeError, match="no registration"):
        e.bop_errors(np.eye(4), np.zeros((8, 12), np.float32), K)
    with pytest.raises(ValueError, match="needs the frame's depth and K"):
        e.hypothesis_report(np.eye(4), metric="vsd", K=K)
    with pytest.raises(ValueError, match="needs the frame's K"):
        e.hypothesis_report(np.eye(4), metric="mspd")
    with pytest.raises(RuntimeError, match="no registration"):
        e.hypothesis_report(np.eye(4), metric="mspd", K=K)
    with pytest.raises(ValueError, match="unknown metric"):
        e.hypothesis_report(np.eye(4), metric="vsdx", depth=np.zeros((8, 12)), K=K)
    # the factor the wrapper uploads is the restatement's
    assert np.array_equal(ops.vsd_dist_factor(K, 48, 64), bm.dist_factor(K, 48, 64))
    assert ops.BOP_TAUS == bm.BOP_TAUS and ops.VSD_MAX_T == 16


def test_argument_errors_are_reported_without_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)
    thr3 = (C.c_float * 16)(*([0.01, 0.02, 0.03] + [0.0] * 13))

    def vsd(est=p, gt=p, gi=None, G=1, N=4, h=8, w=12, obs=p, fac=p, H=8, W=12, x0=0, y0=0, delta=0.015, thr=thr3, T=3, out=p):
        return lib.fp_vsd_counts(est, gt, gi, G, N, h, w, obs, fac, H, W, x0, y0, delta, thr, T, out, None)

    neg, nan = (C.c_float * 16)(0.01, -0.02), (C.c_float * 16)(0.01, float("nan"))
    bad = [dict(est=None), dict(gt=None), dict(obs=None), dict(fac=None), dict(out=None), dict(thr=None), dict(T=0), dict(T=17), dict(N=-1),
           dict(N=65536), dict(G=0), dict(G=3), dict(h=0), dict(w=0), dict(H=0, h=0), dict(W=0), dict(h=1 << 15, w=1 << 14, H=1 << 15, W=1 << 14),
           dict(x0=1), dict(y0=1), dict(x0=-1), dict(y0=-4, h=4), dict(h=9), dict(w=13), dict(delta=-1.0), dict(delta=float("nan")),
           dict(delta=float("inf")), dict(thr=neg, T=2), dict(thr=nan, T=2)]
    for kw in bad:
        assert vsd(**kw) == -1, kw
        assert lib.fp_last_error().startswith(b"fp_vsd_counts"), (kw, lib.fp_last_error())
    assert b"gt_index is NULL" in (vsd(G=3), lib.fp_last_error())[1]
    assert b"not inside" in (vsd(x0=1), lib.fp_last_error())[1]
    assert b"T=17" in (vsd(T=17), lib.fp_last_error())[1]
    # N == 0 does nothing, with NULL tensors; the argument checks that do not depend on N still hold; a threshold beyond T is not read as one
    assert vsd(N=0, est=None, gt=None, obs=None, fac=None, out=None) == 0
    assert vsd(N=0, T=0) == -1 and vsd(N=0, G=0) == -1 and vsd(N=0, thr=None) == -1 and vsd(N=0, x0=1) == -1
    assert vsd(N=0, thr=neg, T=1) == 0 and vsd(N=0, G=3, gi=p) == 0 and vsd(N=0, h=4, w=4, x0=8, y0=4) == 0

    K = (C.c_float * 9)(1066.778, 0, 312.9869, 0, 1067.487, 241.3109, 0, 0, 1)
    Ks = (C.c_float * 9)(1066.778, 0.1, 312.9869, 0, 1067.487, 241.3109, 0, 0, 1)

    def mspd(pts=p, P=100, sym=None, S=0, poses=p, gt=p, gi=None, G=1, N=4, K=K, out=p):
        return lib.fp_mspd(pts, P, sym, S, poses, gt, gi, G, N, K, out, None)

    for kw in (dict(pts=None), dict(poses=None), dict(gt=None), dict(out=None), dict(K=None), dict(K=Ks), dict(P=0), dict(P=(1 << 22) + 1),
               dict(N=-1), dict(N=(1 << 20) + 1), dict(G=0), dict(G=3), dict(S=-1), dict(S=2), dict(S=4097, sym=p)):
        assert mspd(**kw) == -1, kw
        assert lib.fp_last_error().startswith(b"fp_mspd"), (kw, lib.fp_last_error())
    assert b"skew" in (mspd(K=Ks), lib.fp_last_error())[1]
    assert mspd(N=0, pts=None, poses=None, gt=None, out=None) == 0 and mspd(N=0, K=Ks) == -1 and mspd(N=0, G=0) == -1
