"""Cost of BOP's pose errors on the device (fp_vsd_counts, fp_mspd, the full-frame renders that feed VSD) against the host.

On the bench scene (bench.build_scene's can, 2 501 vertices, 480 x 640), for two sets of 252 poses against the ground truth -- "grid":
the scene's rotation grid at the ground truth's translation plus (4, -3, 10) mm, far-off poses as the tests' scene has them;
"ranked": the ranked hypotheses of one registration, most of them close to the object:
  (a) ops.vsd_counts at N = 252, T = 10 on the renders (HIP events around the call with a caller-owned table, warm, median of --reps),
      the bytes the algorithm must move (N * H * W * 4 for est plus the three shared maps once) over the achievable HBM bandwidth
      (MI355X: 6.3e12 B/s) as the floor, and the float32 numpy restatement (tests/bop_errors_model.py) of the same pairs on the host,
      with and without the copy of the renders to the host;
  (b) the 253 full-frame renders, at once and in the chunks FoundationPose.bop_errors uses, and bop_errors as a whole;
  (c) ops.mspd at 252 poses x the vertices.
Prints one JSON line; times in milliseconds."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import bench
import bop_errors_model as bm
from foundationpose_amd import ops
from foundationpose_amd.estimater import FoundationPose
from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
from foundationpose_amd.predict_score import ScorePredictor
from foundationpose_amd.Utils import get_mesh_handle
from foundationpose_amd.weights import DEFAULT_REFINE_CFG, DEFAULT_SCORE_CFG, random_state_dict, trained_refiner_state_dict

HBM_ACHIEVABLE = 6.3e12      # bytes / s (MI355X: 8 TB/s peak, about 6.3 TB/s measured for a streaming copy)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--host_reps", type=int, default=2)
ap.add_argument("--iteration", type=int, default=5)
args = ap.parse_args()
assert args.reps >= 20
dev = torch.device("cuda:0")
sc = bench.build_scene(dev, 0, 252)
refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
scorer = ScorePredictor(cfg=dict(DEFAULT_SCORE_CFG), state_dict=random_state_dict("score", seed=0), device=dev)
est = FoundationPose(model_pts=sc["mesh"].vertices, model_normals=sc["mesh"].vertex_normals, mesh=sc["mesh"], scorer=scorer,
                     refiner=refiner, device=dev)
K = np.asarray(sc["K"], np.float64)
raw = torch.as_tensor(np.asarray(sc["depth"]), device=dev, dtype=torch.float).contiguous()
H, W = (int(x) for x in raw.shape)
est.register(sc["K"], sc["rgb"], sc["depth"], sc["mask"], iteration=args.iteration)
from_c = np.eye(4)
from_c[:3, 3] = np.asarray(est.model_center, np.float64)
gt_c = np.asarray(sc["T"], np.float64) @ from_c
gt32 = torch.as_tensor(gt_c.astype(np.float32), device=dev)[None]
grid = torch.as_tensor((sc["poses"].astype(np.float64) @ from_c).astype(np.float32), device=dev)
handle = get_mesh_handle(est.mesh_tensors)


def render(p):
    return ops.render_crops(handle, p.contiguous(), None, K, H, W, (H, W), mesh_diameter=est.diameter, normalize_xyz=False, want=("depth",))["depth"]


def timed(fn, reps=args.reps):
    """median and minimum ms of fn() between HIP events, after 5 warm calls"""
    ts = []
    for r in range(reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 5:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


out = {"metric": "ms: device = HIP events around warm calls (median of %d); host = numpy float32 restatement, best of %d" % (args.reps, args.host_reps),
       "H": H, "W": W, "P": int(est.pts.shape[0]), "cases": {}}
with torch.inference_mode():
    gt_map = render(gt32)
    for name, poses in (("grid", grid.contiguous()), ("ranked", est.poses.contiguous())):
        N = len(poses)
        assert N == 252
        maps = render(poses)
        table = torch.empty((N, 14), dtype=torch.int32, device=dev)
        vsd_med, vsd_min = timed(lambda: ops.vsd_counts(maps, gt_map, raw, K, est.diameter, out=table))
        one_med, _ = timed(lambda: ops.vsd_counts(maps[:1], gt_map, raw, K, est.diameter, out=table[:1]))
        must = N * H * W * 4 + 3 * H * W * 4
        floor_ms = must / HBM_ACHIEVABLE * 1e3
        counts = table.cpu().numpy()
        # the host: the same pairs in numpy, the renders already there / copied from the device first
        fac, thr, obs = bm.dist_factor(K, H, W), bm.thresholds(bm.BOP_TAUS, est.diameter), raw.cpu().numpy()
        host, copy = None, None
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e_h, g_h = maps.cpu().numpy(), gt_map.cpu().numpy()
            t1 = time.perf_counter()
            ref = bm.vsd_counts(e_h, g_h, obs, fac, bm.BOP_DELTA, thr)
            t2 = time.perf_counter()
            host = (t2 - t1) * 1e3 if host is None else min(host, (t2 - t1) * 1e3)
            copy = (t1 - t0) * 1e3 if copy is None else min(copy, (t1 - t0) * 1e3)
        assert np.array_equal(counts, ref), "the device table differs from the restatement"
        ren_med, ren_min = timed(lambda: (render(poses), render(gt32)), reps=20)
        chunk = est.BOP_DEPTH_BUDGET // (H * W * 4)
        chk_med, _ = timed(lambda: [render(poses[a:a + chunk]) for a in range(0, N, chunk)] + [render(gt32)], reps=20)
        all_med, _ = timed(lambda: est.bop_errors(sc["T"], raw, K, poses=poses), reps=20)
        mspd_med, mspd_min = timed(lambda: ops.mspd(est.pts, poses, gt_c, K))
        mspd_out = torch.empty(N, dtype=torch.float64, device=dev)
        gt_t = torch.as_tensor(gt_c, device=dev)[None]
        mspd_dev_med, _ = timed(lambda: ops.mspd(est.pts, poses, gt_t, K, out=mspd_out))
        covered = float((maps > 0).float().mean())
        out["cases"][name] = dict(
            N=N, T=10, vsd_counts_ms=vsd_med, vsd_counts_min_ms=vsd_min, vsd_counts_one_pose_ms=one_med, bytes_must_move=must,
            floor_ms_at_6p3TBps=floor_ms, share_of_floor=floor_ms / vsd_med, achieved_TBps=must / (vsd_med * 1e-3) / 1e12,
            pixels_rendered_fraction=covered, host_numpy_ms=host, host_copy_of_renders_ms=copy, host_over_device=host / vsd_med,
            renders_253_at_once_ms=ren_med, renders_253_at_once_min_ms=ren_min, renders_253_in_chunks_ms=chk_med, chunk=chunk,
            bop_errors_whole_ms=all_med, mspd_ms=mspd_med, mspd_min_ms=mspd_min, mspd_device_inputs_ms=mspd_dev_med,
            vsd_row0=counts[0].tolist())
print(json.dumps(out))
