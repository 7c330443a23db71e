"""Several objects registered in one frame: ONE estimater.register_objects call over K distinct meshes against K register() calls one
after the other, on the same frame and masks.  K in {1, 2, 4, 8}, in two regimes:
  * "asymmetric": identity symmetry, 252 hypotheses per object (BASELINE configs[3]: 8 novel objects x 252 hypotheses);
  * "symmetric":  a continuous symmetry about z (symmetry_tfs every 5 degrees), which the rotation grid's clustering cuts to 20
                  hypotheses per object -- the calls that leave most of the chip idle one object at a time.
The meshes are K cans of different size, tessellation and shading; the frame is bench.build_scene's, every object uses its mask
(the comparison is about the launch shapes, not about where the objects are).  Timing: synchronised host clock per call, median of
--reps calls after --warmup calls, both sides alternated.  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from foundationpose_amd.estimater import FoundationPose, register_objects
from foundationpose_amd.mesh import make_can_mesh
from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
from foundationpose_amd.predict_score import ScorePredictor
from foundationpose_amd.Utils import symmetry_tfs_from_info
from foundationpose_amd.weights import DEFAULT_REFINE_CFG, DEFAULT_SCORE_CFG, random_state_dict, trained_refiner_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--ks", default="1,2,4,8")
ap.add_argument("--iters", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
ks = [int(k) for k in args.ks.split(",")]
sc = bench.build_scene(dev, 0, 1)
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


out = {"metric": "ms per frame to register K objects (%d refine iterations + 1 score pass): one register_objects call vs K "
       "sequential register() calls" % args.iters, "reps": args.reps, "warmup": args.warmup, "regimes": {}}
for regime, sym in REGIMES.items():
    ests = [FoundationPose(model_pts=m.vertices, model_normals=m.vertex_normals, mesh=m, symmetry_tfs=sym, scorer=scorer, refiner=refiner,
                           device=dev) for m in meshes]
    res = {"hypotheses_per_object": int(ests[0].rot_grid.shape[0]), "K": {}}
    for K in ks:
        sub = ests[:K]

        def sequential():
            for e in sub:
                e.register(K=sc["K"], rgb=sc["rgb"], depth=sc["depth"], ob_mask=sc["mask"], iteration=args.iters)

        def batched():
            register_objects(sub, sc["K"], sc["rgb"], sc["depth"], [sc["mask"]] * K, iteration=args.iters)
        b, s = [], []
        for i in range(args.warmup + args.reps):
            tb, ts = timed(batched), timed(sequential)
            if i >= args.warmup:
                b.append(tb)
                s.append(ts)
        bm, sm = float(np.median(b)), float(np.median(s))
        res["K"][str(K)] = dict(batched_ms=bm, sequential_ms=sm, batched_over_sequential=bm / sm,
                                batched_spread_ms=[float(min(b)), float(max(b))], sequential_spread_ms=[float(min(s)), float(max(s))])
        print(f"{regime} K={K}: batched {bm:.2f} ms, sequential {sm:.2f} ms", file=sys.stderr, flush=True)
    out["regimes"][regime] = res
    del ests
print(json.dumps(out))
