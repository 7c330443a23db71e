"""GPU: fp_pose_errors (ADD, ADD-S, symmetry-aware errors of pose batches) against the numpy restatement of its definition
(tests/pose_errors_model.py: mssd bit-equal, the means within P * 2^-53 relative -- the bound of any float64 summation order against the
exactly rounded sum, the per-point terms being equal by construction), what it may write, its replay stability, the float64 metrics of
vis.*, and the layers above it (FoundationPose.pose_errors / hypothesis_report, scripts/run_ycb_video.py --hypothesis_errors).

Measured on an MI355X: the worst |value - vis| / (2^-24 (|t_rel| + 2 r_max)) is 0.156 over the scene's 252 poses
(test_against_float64_metrics_on_the_scene) and 0.101 for the estimator's returned pose (test_estimator_pose_errors, the shifted mesh;
0.041 centred) where the bound allows 8; the means came out bit-equal to the exactly rounded sums in every case of section 1 (a float64
sum of a few thousand float32 values of one magnitude is usually exact), where the bound allows P x 2^-53.  Each test prints its figure
before it asserts."""
import math

import numpy as np
import pytest
import torch

import pose_errors_model as pm
from test_gpu_multi_object import dev  # noqa: F401
from test_pose_errors_host import HALF_TURN, _rot, _tf

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _points(P, seed):
    """P points of an object of ~0.1 m (float32)"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (P, 3)) * [0.05, 0.04, 0.07]).astype(np.float32)


def _pose_sets(N, G, seed):
    """G ground truths 0.4-1.5 m from the camera (float64) and N float32 poses around them, from exact to far off"""
    rng = np.random.default_rng(seed)
    gts = np.stack([_tf(_rot(rng.normal(size=3), rng.uniform(0, math.pi)), [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.4, 1.5)])
                    for _ in range(G)])
    poses = []
    for n in range(N):
        g = gts[n % G]
        ang, off = (0.0, 1e-4, 1e-2, 0.3, math.pi)[n % 5], (0.0, 1e-5, 1e-3, 0.05, 1.0)[(n // 5) % 5]
        u = rng.normal(size=3)
        poses.append(_tf(_rot(rng.normal(size=3), ang) @ g[:3, :3], g[:3, 3] + off * u / np.linalg.norm(u)))
    return np.stack(poses).astype(np.float32), gts


def _symmetries(S, seed):
    """identity first, then turns about z and one general rigid transform with a translation"""
    rng = np.random.default_rng(seed)
    out = [np.eye(4)] + [_tf(_rot([0, 0, 1], 2 * math.pi * k / max(S - 1, 1)), [0, 0, 0]) for k in range(1, max(S - 1, 1))]
    out.append(_tf(_rot(rng.normal(size=3), 0.7), [0.002, -0.001, 0.003]))
    return np.stack(out[:S]) if S else None


def _call(dev, pts, poses, gts, gt_index, sym, flags, out=None):
    """through the C ABI (ops.pose_errors adds only the buffers)"""
    from foundationpose_amd import ops
    want = tuple(n for n, f in (("add", 1), ("adds", 2), ("sym", 4)) if flags & f)
    gi = None if gt_index is None else torch.as_tensor(np.asarray(gt_index, np.int32), device=dev)
    return ops.pose_errors(torch.as_tensor(pts, device=dev), torch.as_tensor(poses, device=dev), gts, gt_index=gi, symmetry_tfs=sym,
                           want=want, out=out)


def _check(got, ref, P, flags, what):
    """mssd bit-equal; add, adds, add_sym within P * 2^-53 relative; NaN exactly where the restatement has NaN"""
    assert got.shape == ref.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    ok = ~np.isnan(ref)
    assert np.array_equal(got[:, 3][ok[:, 3]].view(np.uint64), ref[:, 3][ok[:, 3]].view(np.uint64)), (what, "mssd", got[:, 3], ref[:, 3])
    worst = 0.0
    for c in range(3):
        g, r = got[:, c][ok[:, c]], ref[:, c][ok[:, c]]
        rel = np.abs(g - r) / np.maximum(np.abs(r), np.finfo(np.float64).tiny)
        rel[(g == r)] = 0.0
        if len(rel):
            worst = max(worst, float(rel.max()))
        assert (np.abs(g - r) <= P * U * np.abs(r)).all(), (what, "column", c, g, r, rel.max() / U)
    print(f"{what}: worst relative difference of a mean {worst / U:.2f} x 2^-53 (bound {P})")
    for c, f in enumerate((1, 2, 4, 4)):
        if not flags & f:
            assert np.isnan(got[:, c]).all(), (what, c)


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 2501, 10007])
def test_every_point_count_with_an_explicit_index(dev, P):
    """N = 3, S = 6, every column, an explicit gt_index with a repeat and one out-of-range entry: that row NaN, its neighbours right"""
    pts, sym = _points(P, P), _symmetries(6, P)
    poses, gts = _pose_sets(3, 2, 100 + P)
    for bad in (2, -1):
        gi = [1, bad, 1]
        got = _call(dev, pts, poses, gts, gi, sym, 7).cpu().numpy()
        assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()
        _check(got, pm.pose_errors(pts, poses, gts, gi, sym, 7), P, 7, f"P={P} index {gi}")


@pytest.mark.parametrize("S", [0, 1, 6])
def test_every_combination_of_flags(dev, S):
    P, N = 257, 3
    pts, sym = _points(P, 5), _symmetries(S, 9)
    poses, gts = _pose_sets(N, N, 11 + S)
    for flags in range(1, 8):
        if flags & 4 and S == 0:
            continue
        got = _call(dev, pts, poses, gts, None, sym, flags).cpu().numpy()       # G == N, no index: pose n against gt n
        _check(got, pm.pose_errors(pts, poses, gts, None, sym, flags), P, flags, f"S={S} flags={flags}")
    if S == 1:      # S_0 = I: add_sym == add bit for bit
        got = _call(dev, pts, poses, gts, None, sym, 7).cpu().numpy()
        assert np.array_equal(got[:, 2].view(np.uint64), got[:, 0].view(np.uint64)), got


@pytest.mark.parametrize("N,P,S,G", [(1, 1, 1, 1), (1, 63, 0, 1), (1, 64, 6, 1), (1, 65, 1, 1), (1, 2501, 6, 1), (1, 10007, 0, 1),
                                     (252, 65, 6, 1), (252, 257, 1, 252), (252, 2501, 6, 252), (3, 10007, 1, 1)])
def test_batch_sizes_and_index_forms(dev, N, P, S, G):
    """gt_index NULL with G = 1 (all against one) and G = N (pairwise), at both ends of the batch sizes"""
    pts, sym = _points(P, 3 * P + N), _symmetries(S, N)
    poses, gts = _pose_sets(N, G, 1000 + N + P)
    flags = 7 if S else 3
    got = _call(dev, pts, poses, gts, None, sym, flags).cpu().numpy()
    _check(got, pm.pose_errors(pts, poses, gts, None, sym, flags), P, flags, f"N={N} P={P} S={S} G={G}")


def test_odd_chunk_count_with_two_queries_per_lane(dev):
    """N * ceil(P / 256) >= 1024 takes two queries per lane; P = 2305 is 9 chunks, so every pose's last workgroup has a second query
    of dead lanes only (no partial may be written for it, and its lanes read no point beyond P)"""
    N, P = 252, 2305
    pts, sym = _points(P, 77), _symmetries(6, 78)
    poses, gts = _pose_sets(N, 1, 79)
    for flags in (5, 7):
        got = _call(dev, pts, poses, gts, None, sym, flags).cpu().numpy()
        _check(got, pm.pose_errors(pts, poses, gts, None, sym, flags), P, flags, f"N={N} P={P} flags={flags}")
    # and a row of it is the call on that pose alone, which takes one query per lane
    for k in (0, 100, 251):
        one = _call(dev, pts, poses[k:k + 1], gts, None, sym, 7).cpu().numpy()
        assert np.array_equal(one.view(np.uint64), got[k:k + 1].view(np.uint64)), k


def test_non_finite_transforms_give_nan(dev):
    """a NaN or an infinity in a pose or its ground truth: that row NaN in every column (not +inf or a zero mssd), its neighbours right;
    a non-finite symmetry: add_sym and mssd NaN, add and adds right"""
    P = 300
    pts, sym = _points(P, 31), _symmetries(3, 32)
    poses, gts = _pose_sets(4, 4, 33)
    poses[1, 0, 3] = np.nan
    poses[2, 1, 1] = np.inf
    gts[3, 2, 3] = np.nan
    got = _call(dev, pts, poses, gts, None, sym, 7).cpu().numpy()
    assert np.isfinite(got[0]).all() and np.isnan(got[1:]).all(), got
    _check(got, pm.pose_errors(pts, poses, gts, None, sym, 7), P, 7, "non-finite poses")
    poses, gts = _pose_sets(4, 4, 33)
    sym[2, 0, 0] = np.nan
    got = _call(dev, pts, poses, gts, None, sym, 7).cpu().numpy()
    assert np.isfinite(got[:, :2]).all() and np.isnan(got[:, 2:]).all(), got
    _check(got, pm.pose_errors(pts, poses, gts, None, sym, 7), P, 7, "non-finite symmetry")


def test_wrapper_refusals_on_device_tensors(dev):
    """the checks of ops.pose_errors that only device tensors reach: dtype and layout, the index, the caller's buffers"""
    from foundationpose_amd import _lib, ops
    P, N = 50, 3
    pts, poses = torch.as_tensor(_points(P, 1), device=dev), torch.as_tensor(_pose_sets(N, 1, 2)[0], device=dev)
    gt = np.eye(4)
    good = ops.pose_errors(pts, poses, gt).cpu().numpy()
    assert np.isfinite(good[:, :2]).all()
    ws = ops.pose_errors_workspace(N, P, 0, dev)
    for kw, msg in ((dict(model_pts=pts.double()), "model_pts: expected dtype"),
                    (dict(poses=poses.half()), "poses: expected dtype"),
                    (dict(model_pts=torch.as_tensor(_points(2 * P, 1), device=dev)[::2]), "model_pts: tensor must be contiguous"),
                    (dict(poses=poses.transpose(1, 2)), "poses: tensor must be contiguous"),
                    (dict(gt_index=torch.zeros(N, dtype=torch.int64, device=dev)), "gt_index: expected dtype"),
                    (dict(gt_index=torch.zeros(N, dtype=torch.int32)), "gt_index: expected a CUDA"),
                    (dict(gt_index=torch.zeros(N + 1, dtype=torch.int32, device=dev)), f"gt_index tensor of {N} entries"),
                    (dict(gt=np.stack([gt] * 2)), f"2 ground truths for {N} poses need a gt_index"),
                    (dict(want=("sym",)), 'want "sym" needs symmetry_tfs'),
                    (dict(gt=torch.zeros(5, 4, device=dev)), r"gt must be \(4,4\) or \(n,4,4\)"),
                    (dict(symmetry_tfs=torch.zeros(2, 3, 3, device=dev)), r"symmetry_tfs must be \(4,4\) or \(n,4,4\)"),
                    (dict(out=torch.zeros(N, 4, device=dev)), "out: expected dtype"),
                    (dict(out=torch.zeros(N, 4, dtype=torch.float64)), "out: expected a CUDA"),
                    (dict(out=torch.zeros(N + 1, 4, dtype=torch.float64, device=dev)), rf"out must be \({N}, 4\)"),
                    (dict(out=torch.zeros(4, N, dtype=torch.float64, device=dev)), rf"out must be \({N}, 4\)"),
                    (dict(workspace=ws[:-1]), "bytes, .* needed"),
                    (dict(workspace=ws.cpu()), "workspace must be a contiguous CUDA"),
                    (dict(workspace=torch.zeros(2 * ws.numel(), dtype=torch.float64, device=dev)[::2]), "workspace must be a contiguous CUDA"),
                    (dict(workspace=ws, symmetry_tfs=np.eye(4)[None]), "bytes, .* needed")):        # S = 1 needs more room
        args = dict(model_pts=pts, poses=poses, gt=gt)
        args.update(kw)
        with pytest.raises(_lib.FpAmdError, match=msg):
            ops.pose_errors(**args)
    # the exact workspace and a device index are accepted and change nothing
    again = ops.pose_errors(pts, poses, gt, gt_index=torch.zeros(N, dtype=torch.int32, device=dev), workspace=ws).cpu().numpy()
    assert np.array_equal(again.view(np.uint64), good.view(np.uint64))


# ------------------------------------------------------------------ 2. what it writes
def test_writes_nothing_outside_out(dev):
    P, N = 300, 5
    pts, sym = _points(P, 1), _symmetries(2, 2)
    poses, gts = _pose_sets(N, 1, 3)
    sentinel = -1.2345678901234567e+300
    for flags in (1, 2, 4, 3, 7):
        arena = torch.full((64 + N * 4 + 64,), sentinel, dtype=torch.float64, device=dev)
        out = arena[64:64 + N * 4].view(N, 4)
        r = _call(dev, pts, poses, gts, None, sym, flags, out=out)
        assert r.data_ptr() == out.data_ptr()
        a = arena.cpu().numpy()
        assert (a[:64] == sentinel).all() and (a[64 + N * 4:] == sentinel).all()
        got = a[64:64 + N * 4].reshape(N, 4)
        for c, f in enumerate((1, 2, 4, 4)):
            assert (np.isnan(got[:, c]).all() if not flags & f else np.isfinite(got[:, c]).all()), (flags, c, got)


# ------------------------------------------------------------------ 3. the same bits every time
def test_rows_replays_and_graph_have_equal_bits(dev):
    from foundationpose_amd import ops
    P, N, S = 2501, 7, 3
    pts, sym = _points(P, 21), _symmetries(S, 22)
    poses, gts = _pose_sets(N, N, 23)
    batch = _call(dev, pts, poses, gts, None, sym, 7).cpu().numpy()
    again = _call(dev, pts, poses, gts, None, sym, 7).cpu().numpy()
    assert np.array_equal(batch.view(np.uint64), again.view(np.uint64))
    for k in range(N):
        one = _call(dev, pts, poses[k:k + 1], gts[k:k + 1], None, sym, 7).cpu().numpy()
        assert np.array_equal(one.view(np.uint64), batch[k:k + 1].view(np.uint64)), (k, one, batch[k])
    # a captured graph owns its buffers: out= and workspace=, every input already a device tensor of the C ABI's type
    pts_t, poses_t = torch.as_tensor(pts, device=dev), torch.as_tensor(poses, device=dev)
    gt_t, sym_t = torch.as_tensor(gts, device=dev), torch.as_tensor(sym, device=dev)
    out = torch.zeros((N, 4), dtype=torch.float64, device=dev)
    ws = ops.pose_errors_workspace(N, P, S, dev)
    want = ("add", "adds", "sym")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.pose_errors(pts_t, poses_t, gt_t, symmetry_tfs=sym_t, want=want, out=out, workspace=ws)     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.pose_errors(pts_t, poses_t, gt_t, symmetry_tfs=sym_t, want=want, out=out, workspace=ws)
    for _ in range(3):
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), batch.view(np.uint64))
    # new poses in the graph's input buffer: the replay computes them
    poses_t.copy_(torch.as_tensor(poses[::-1].copy(), device=dev))
    g.replay()
    torch.cuda.synchronize()
    ref = _call(dev, pts, poses[::-1].copy(), gts, None, sym, 7).cpu().numpy()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), ref.view(np.uint64))


# ------------------------------------------------------------------ 4. against the float64 metrics
def _vs_vis(rows, poses64, gts64, pts64, poses_for_bound, what):
    """rows' add / adds against vis.add_err / vis.adds_err within 8 * 2^-24 * (|t_rel| + 2 r_max) + 2 * delta * vis"""
    from foundationpose_amd import vis
    worst = 0.0
    for n, (pose, gt) in enumerate(zip(poses64, gts64)):
        for col, ref in ((0, vis.add_err(pose, gt, pts64)), (1, vis.adds_err(pose, gt, pts64))):
            bound = pm.bound_vs_float64(poses_for_bound[n], gt, pts64, ref)
            _, t = pm.relative_tf(poses_for_bound[n], gt)
            ratio = abs(rows[n, col] - ref) / (2.0 ** -24 * (np.linalg.norm(t) + 2 * np.linalg.norm(pts64, axis=1).max()))
            worst = max(worst, ratio)
            assert abs(rows[n, col] - ref) <= bound, (what, n, col, rows[n, col], ref, bound, ratio)
    print(f"{what}: worst |value - vis| / (2^-24 (|t_rel| + 2 r_max)) = {worst:.3f} (the bound allows 8)")


def test_against_float64_metrics_on_the_scene(scene, dev):
    pts = np.asarray(scene["mesh"].vertices, np.float64)
    poses, gt = scene["poses"], np.asarray(scene["gt"], np.float64)
    rows = _call(dev, pts.astype(np.float32), poses, gt[None], None, None, 3).cpu().numpy()
    assert rows.shape == (252, 4) and np.isnan(rows[:, 2:]).all()
    _vs_vis(rows, poses.astype(np.float64), [gt] * len(poses), pts.astype(np.float32).astype(np.float64), poses, "scene grid")
    assert (rows[:, 1] <= rows[:, 0]).all()


# ------------------------------------------------------------------ 5. the estimator
def _estimator(mesh, dev, symmetry_tfs=None):
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    from foundationpose_amd.predict_score import ScorePredictor
    from foundationpose_amd.weights import DEFAULT_REFINE_CFG, DEFAULT_SCORE_CFG, random_state_dict, trained_refiner_state_dict
    refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
    scorer = ScorePredictor(cfg=dict(DEFAULT_SCORE_CFG), state_dict=random_state_dict("score", seed=0), device=dev)
    return FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, symmetry_tfs=symmetry_tfs, mesh=mesh, scorer=scorer,
                          refiner=refiner, device=dev)


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (0.03, -0.02, 0.05)], ids=["centred", "shifted"])
def test_estimator_pose_errors(scene, dev, shift):
    from foundationpose_amd import ops
    mesh = scene["mesh"].copy()
    mesh.vertices = np.asarray(mesh.vertices) + np.asarray(shift)           # a mesh whose model_center is not 0
    gt = np.asarray(scene["gt"], np.float64) @ _tf(np.eye(3), -np.asarray(shift))   # the same object in the camera, in the shifted mesh's frame
    est = _estimator(mesh, dev)          # no symmetry: the rotation grid keeps its 252 hypotheses, and add_sym is add
    assert np.allclose(est.model_center, shift, atol=1e-6)
    with pytest.raises(RuntimeError, match="no registration"):
        est.pose_errors(gt)
    pose = est.register(scene["K"], scene["rgb"], scene["depth"], scene["mask"], iteration=2)
    table = est.pose_errors(gt)
    assert tuple(table.shape) == (252, 4) and table.dtype == torch.float64 and table.is_cuda
    rows = table.cpu().numpy()
    assert np.isfinite(rows).all() and (rows[:, 1] <= rows[:, 0]).all() and np.array_equal(rows[:, 2], rows[:, 0])
    assert (rows[:, 3] >= rows[:, 2]).all()
    # the rows are in the order of est.poses: row k is the call on hypothesis k alone
    for k in (0, 1, 100, 251):
        one = est.pose_errors(gt, poses=est.poses[k:k + 1]).cpu().numpy()
        assert np.array_equal(one.view(np.uint64), rows[k:k + 1].view(np.uint64))
    # row 0 is the returned pose: vis.* on it, in the frame of the mesh as it was handed over
    pts_ori = np.asarray(mesh.vertices, np.float64)
    centred32 = est.pts.cpu().numpy()
    gt_c = gt @ _tf(np.eye(3), est.model_center)
    from foundationpose_amd import vis
    worst = 0.0
    for col, ref in ((0, vis.add_err(np.asarray(pose, np.float64), gt, pts_ori)), (1, vis.adds_err(np.asarray(pose, np.float64), gt, pts_ori))):
        bound = pm.bound_vs_float64(est.poses[0].cpu().numpy(), gt_c, centred32, ref)
        _, t = pm.relative_tf(est.poses[0].cpu().numpy(), gt_c)
        ratio = abs(rows[0, col] - ref) / (2.0 ** -24 * (np.linalg.norm(t) + 2 * np.linalg.norm(centred32.astype(np.float64), axis=1).max()))
        worst = max(worst, ratio)
        print(f"shift {shift} col {col}: table {rows[0, col]:.9e} vis {ref:.9e} bound {bound:.2e} ratio {ratio:.3f}")
        assert abs(rows[0, col] - ref) <= bound, (col, rows[0, col], ref, bound, ratio)
    # the report: best rank = argmin of the column, scores of both ranks
    for metric, col in (("adds", 1), ("add", 0), ("add_sym", 2), ("mssd", 3)):
        rep = est.hypothesis_report(gt, metric=metric)
        k = int(np.argmin(rows[:, col]))
        assert rep["best_rank"] == k and rep["best_err"] == rows[k, col] and rep["top_err"] == rows[0, col] and rep["n"] == 252
        assert rep["top_score"] == float(est.scores[0]) and rep["best_score"] == float(est.scores[k]) and rep["metric"] == metric
    # a new object has no hypotheses: the last object's are not evaluated on its points
    keep, keep_scores = est.poses, est.scores
    est.reset_object(mesh.vertices, mesh.vertex_normals, mesh=mesh)
    assert est.poses is None and est.scores is None
    with pytest.raises(RuntimeError, match="no registration"):
        est.pose_errors(gt)
    with pytest.raises(RuntimeError, match="no registration"):
        est.hypothesis_report(gt)
    est.poses, est.scores = keep, keep_scores
    # a tracked sequence: N poses against N ground truths, pairwise
    seq = est.poses[:5]
    gts = np.stack([gt @ _tf(_rot([0, 0, 1], 0.01 * i), [0.001 * i, 0, 0]) for i in range(5)])
    pair = est.pose_errors(gts, poses=seq).cpu().numpy()
    for i in range(5):
        one = est.pose_errors(gts[i], poses=seq[i:i + 1]).cpu().numpy()
        assert np.array_equal(one.view(np.uint64), pair[i:i + 1].view(np.uint64))
    assert ops.PoseErrors.rows(table)[0] == ops.PoseErrors(*rows[0])


def test_half_turn_is_invisible_to_the_symmetry_aware_errors(scene, dev):
    """the can turned half-way about its axis: centimetres to ADD, nothing to add_sym / mssd with the half turn in the symmetry set"""
    est = _estimator(scene["mesh"], dev, symmetry_tfs=np.stack([np.eye(4), HALF_TURN]))
    gt = np.asarray(scene["gt"], np.float64)
    flipped = torch.as_tensor((gt @ HALF_TURN @ _tf(np.eye(3), est.model_center)).astype(np.float32), device=dev)[None]
    r = ops_rows(est.pose_errors(gt, poses=flipped))[0]
    assert r.add > 0.01 and r.add_sym < 1e-6 and r.mssd < 1e-6 and r.adds < 1e-6, r


def ops_rows(table):
    from foundationpose_amd import ops
    return ops.PoseErrors.rows(table)


# ------------------------------------------------------------------ 6. the script
def test_run_ycb_video_hypothesis_errors(tmp_path, dev):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_ycb_video", os.path.join(root, "scripts", "run_ycb_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    plain = mod.main(["--synthetic", "2", "--est_refine_iter", "1", "--debug_dir", str(tmp_path / "a")])
    full = mod.main(["--synthetic", "2", "--est_refine_iter", "1", "--hypothesis_errors", "--debug_dir", str(tmp_path / "b")])
    assert sorted(plain) == ["ADDS_AUC", "ADDS_mean_m", "ADD_AUC", "ADD_mean_m", "n"]
    assert {k: full[k] for k in plain} == plain
    assert sorted(set(full) - set(plain)) == ["ADDS_oracle_mean_m", "ADDsym_AUC", "best_rank_hist", "hypothesis_reports"]
    assert sum(full["best_rank_hist"].values()) == full["n"] == 2 and sorted(full["best_rank_hist"]) == ["0", "1-4", "5+"]
    assert len(full["hypothesis_reports"]) == 2 and 0.0 <= full["ADDsym_AUC"] <= 1.0
    assert 0.0 <= full["ADDS_oracle_mean_m"] <= full["ADDS_mean_m"] + 1e-6
