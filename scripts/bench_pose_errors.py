"""Cost of the pose-error table (ops.pose_errors / fp_pose_errors) against the host metrics it replaces.

Case "ranked_252": the 252 ranked hypotheses of one registration on the bench scene (bench.build_scene's can, 2 501 vertices) against
the ground truth -- the device table (HIP events around the call with caller-owned out / workspace and device-resident inputs, warm,
median of --reps) for ("add", "adds") and for ("add", "adds", "sym"), against the only way to get the same numbers before: a loop
over vis.add_err / vis.adds_err (numpy + a scipy KD-tree per pose) on the host, including the copy of the poses to the host.
Case "one_pose": the same with N = 1.  Case "points_100k": a 100 000-point set, N = 1 and N = 16.

Prints one JSON line; times in milliseconds."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from foundationpose_amd import ops, vis
from foundationpose_amd.estimater import FoundationPose
from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
from foundationpose_amd.predict_score import ScorePredictor
from foundationpose_amd.weights import DEFAULT_REFINE_CFG, DEFAULT_SCORE_CFG, random_state_dict, trained_refiner_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--host_reps", type=int, default=3)
ap.add_argument("--iteration", type=int, default=5)
args = ap.parse_args()
assert args.reps >= 20
dev = torch.device("cuda:0")
sc = bench.build_scene(dev, 0, 252)
refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
scorer = ScorePredictor(cfg=dict(DEFAULT_SCORE_CFG), state_dict=random_state_dict("score", seed=0), device=dev)
half_turn = np.diag([-1.0, -1.0, 1.0, 1.0])
# registered without a symmetry set (the rotation grid keeps its 252 hypotheses); the half turn only enters the "sym" columns below
est = FoundationPose(model_pts=sc["mesh"].vertices, model_normals=sc["mesh"].vertex_normals, mesh=sc["mesh"], scorer=scorer,
                     refiner=refiner, device=dev)
est.register(sc["K"], sc["rgb"], sc["depth"], sc["mask"], iteration=args.iteration)
c = np.asarray(est.model_center, np.float64)
to_c, from_c = np.eye(4), np.eye(4)
to_c[:3, 3], from_c[:3, 3] = -c, c
gt_c = np.asarray(sc["T"], np.float64) @ from_c
sym_c = to_c @ np.stack([np.eye(4), half_turn]) @ from_c


def device_ms(pts, poses, gt, sym, want):
    """median ms of the call alone: inputs on the device, buffers owned by the caller"""
    gt_t = torch.as_tensor(gt, device=dev).reshape(-1, 4, 4)
    sym_t = None if sym is None else torch.as_tensor(sym, device=dev)
    N, P, S = len(poses), len(pts), 0 if sym is None else len(sym)
    out = torch.empty((N, 4), dtype=torch.float64, device=dev)
    ws = ops.pose_errors_workspace(N, P, S, dev)
    ts = []
    for r in range(args.reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.pose_errors(pts, poses, gt_t, symmetry_tfs=sym_t, want=want, out=out, workspace=ws)
        e1.record()
        torch.cuda.synchronize()
        if r >= 5:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), out.cpu().numpy()


def host_ms(pts_t, poses_t, gt):
    """the host metrics over the same poses, the copy of the poses included; best of --host_reps"""
    best, vals = None, None
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = poses_t.cpu().numpy().astype(np.float64)
        pts = pts_t.cpu().numpy().astype(np.float64)
        vals = [(vis.add_err(p, gt, pts), vis.adds_err(p, gt, pts)) for p in P]
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, np.asarray(vals)


out = {"metric": "ms per pose-error table: device (HIP events, median of %d warm calls) vs the host loop over vis.add_err / "
       "vis.adds_err (best of %d, poses copied to the host)" % (args.reps, args.host_reps), "cases": {}}
with torch.inference_mode():
    poses = est.poses.contiguous()
    assert len(poses) == 252
    for name, ps in (("ranked_252", poses), ("one_pose", poses[:1].contiguous())):
        med, lo, tab = device_ms(est.pts, ps, gt_c, None, ("add", "adds"))
        med_s, lo_s, _ = device_ms(est.pts, ps, gt_c, sym_c, ("add", "adds", "sym"))
        med_a, lo_a, _ = device_ms(est.pts, ps, gt_c, None, ("add",))
        h, vals = host_ms(est.pts, ps, gt_c)
        out["cases"][name] = dict(N=len(ps), P=int(est.pts.shape[0]), device_add_adds_ms=med, device_add_adds_min_ms=lo,
                                  device_add_adds_sym_ms=med_s, device_add_only_ms=med_a, host_add_adds_ms=h, host_over_device=h / med,
                                  pairs_per_s=len(ps) * float(est.pts.shape[0]) ** 2 / (med * 1e-3),
                                  max_abs_diff_to_host_m=float(np.abs(tab[:, :2] - vals).max()))
    rng = np.random.default_rng(0)
    big = torch.as_tensor((rng.uniform(-1, 1, (100000, 3)) * [0.05, 0.04, 0.07]).astype(np.float32), device=dev)
    for n in (1, 16):
        ps = poses[:n].contiguous()
        med, lo, tab = device_ms(big, ps, gt_c, None, ("add", "adds"))
        case = dict(N=n, P=100000, device_add_adds_ms=med, device_add_adds_min_ms=lo, pairs_per_s=n * 1e10 / (med * 1e-3))
        if n == 1:
            h, vals = host_ms(big, ps, gt_c)
            case.update(host_add_adds_ms=h, host_over_device=h / med, max_abs_diff_to_host_m=float(np.abs(tab[:, :2] - vals).max()))
        out["cases"]["points_100k_N%d" % n] = case
print(json.dumps(out))
