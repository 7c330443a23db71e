"""Objects registered in several camera streams: ONE estimater.register_views call against one register() per (camera, object), each
on its own frame, one after the other.  V in {1, 2, 4} cameras x {1, 2} objects per camera, in two regimes:
  * "asymmetric": identity symmetry, 252 hypotheses per object;
  * "symmetric":  a continuous symmetry about z (symmetry_tfs every 5 degrees), which the rotation grid's clustering cuts to 20
                  hypotheses per object.
Every camera gets its own frame (bench.build_scene's, with a per-camera rgb perturbation and depth offset) and its own K (focal length
and principal point shifted per camera); every object uses the scene's mask.  Timing: synchronised host clock per call, median of
--reps calls after --warmup calls, both sides alternated.  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from foundationpose_amd.estimater import FoundationPose, register_views
from foundationpose_amd.mesh import make_can_mesh
from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
from foundationpose_amd.predict_score import ScorePredictor
from foundationpose_amd.Utils import symmetry_tfs_from_info
from foundationpose_amd.weights import DEFAULT_REFINE_CFG, DEFAULT_SCORE_CFG, random_state_dict, trained_refiner_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--views", default="1,2,4")
ap.add_argument("--objects", default="1,2")
ap.add_argument("--iters", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
vs = [int(v) for v in args.views.split(",")]
ks = [int(k) for k in args.objects.split(",")]
sc = bench.build_scene(dev, 0, 1)
rng = np.random.default_rng(0)
rgbs, depths, Ks = [], [], []
for v in range(max(vs)):
    rgbs.append(np.clip(np.asarray(sc["rgb"]).astype(np.float32) + (rng.normal(0, 4, np.asarray(sc["rgb"]).shape) if v else 0), 0, 255)
                .astype(np.uint8))
    depths.append((np.asarray(sc["depth"]) + 0.002 * v).astype(np.float32))
    K = np.asarray(sc["K"], dtype=np.float64).copy()
    K[0, 0] *= 1.0 + 0.03 * v
    K[1, 1] *= 1.0 + 0.03 * v
    K[0, 2] += 3.5 * v
    Ks.append(K)
mask = np.asarray(sc["mask"])
refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
scorer = ScorePredictor(cfg=dict(DEFAULT_SCORE_CFG), state_dict=random_state_dict("score", seed=0), device=dev)
meshes = [make_can_mesh(radius=0.03 + 0.004 * k, height=0.08 + 0.01 * k, n_ang=30 + 6 * k, n_axial=16 + 4 * k, textured=k % 2 == 0,
                        tex_size=256, seed=k) for k in range(max(ks))]
REGIMES = {"asymmetric": None,
           "symmetric": symmetry_tfs_from_info({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


out = {"metric": "ms per frame set to register K objects in each of V cameras (%d refine iterations + 1 score pass): one register_views "
       "call vs V x K sequential register() calls on their own frames" % args.iters, "reps": args.reps, "warmup": args.warmup,
       "regimes": {}}
for regime, sym in REGIMES.items():
    res = {"K": {}}
    for V in vs:
        for Kn in ks:
            views = [v for v in range(V) for _ in range(Kn)]
            ests = [FoundationPose(model_pts=meshes[k].vertices, model_normals=meshes[k].vertex_normals, mesh=meshes[k], symmetry_tfs=sym,
                                   scorer=scorer, refiner=refiner, device=dev) for _ in range(V) for k in range(Kn)]
            res["hypotheses_per_object"] = int(ests[0].rot_grid.shape[0])

            def sequential():
                for e, v in zip(ests, views):
                    e.register(K=Ks[v], rgb=rgbs[v], depth=depths[v], ob_mask=mask, iteration=args.iters)

            def batched():
                register_views(ests, views, rgbs[:V], depths[:V], Ks[:V], [mask] * len(ests), iteration=args.iters)
            b, s = [], []
            for i in range(args.warmup + args.reps):
                tb, ts = timed(batched), timed(sequential)
                if i >= args.warmup:
                    b.append(tb)
                    s.append(ts)
            bm, sm = float(np.median(b)), float(np.median(s))
            res["K"][f"V{V}xK{Kn}"] = dict(batched_ms=bm, sequential_ms=sm, batched_over_sequential=bm / sm,
                                           batched_spread_ms=[float(min(b)), float(max(b))],
                                           sequential_spread_ms=[float(min(s)), float(max(s))])
            print(f"{regime} V={V} K={Kn}: batched {bm:.2f} ms, sequential {sm:.2f} ms", file=sys.stderr, flush=True)
            del ests
    out["regimes"][regime] = res
print(json.dumps(out))
