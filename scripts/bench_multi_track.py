"""Several objects per frame: ONE batched graphed tracker over K distinct meshes (graphs.GraphedTracker with a list of meshes,
1 hypothesis per object, 2 refine iterations -- what estimater.track_objects replays) against K single-object graphed trackers run
one after the other on the same frames (K x track_one with track_graph=True).  K in {1, 2, 4, 8}.

Per frame both sides upload the uint8 colour image and the float depth map from pinned host memory (every single-object tracker
ingests the frame itself, as K separate track_one calls do; the batched tracker once) and track from their previous output.  The
frames are bench.make_sequence's synthetic sequence; the meshes are K cans of different size, tessellation and shading.  Timing:
synchronised host clock over --frames frames after --warmup frames.  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from foundationpose_amd import synthetic as syn
from foundationpose_amd.graphs import GraphedTracker
from foundationpose_amd.mesh import make_can_mesh
from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
from foundationpose_amd.Utils import make_mesh_tensors
from foundationpose_amd.weights import DEFAULT_REFINE_CFG, trained_refiner_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=500)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--ks", default="1,2,4,8")
ap.add_argument("--iters", type=int, default=2)
args = ap.parse_args()
dev = torch.device("cuda:0")
ks = [int(k) for k in args.ks.split(",")]
sc = bench.build_scene(dev, 0, 1)
gt, rgb_h, depth_h, _ = bench.make_sequence(dev, sc, args.frames + args.warmup)
refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
meshes = [make_can_mesh(radius=0.03 + 0.004 * k, height=0.08 + 0.01 * k, n_ang=30 + 6 * k, n_axial=16 + 4 * k, textured=k % 2 == 0,
                        tex_size=256, seed=k) for k in range(max(ks))]
gms = [make_mesh_tensors(m, device=dev) for m in meshes]
diams = [float(np.linalg.norm(m.vertices.max(0) - m.vertices.min(0))) for m in meshes]
start = torch.as_tensor(gt[0], device=dev, dtype=torch.float32)


def run(trackers, n):
    """n frames through `trackers` (each uploads and ingests the frame itself, then replays) -> ms per frame"""
    rgb_u8 = torch.empty((syn.H, syn.W, 3), dtype=torch.uint8, device=dev)
    for t in trackers:
        t.poses_in.copy_(start.expand(t.N, 4, 4))
    torch.cuda.synchronize()
    t0 = None
    for f in range(n + args.warmup):
        if f == args.warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for t in trackers:
            rgb_u8.copy_(rgb_h[f], non_blocking=True)
            t.rgb.copy_(rgb_u8)
            t.depth.copy_(depth_h[f], non_blocking=True)
            if f:
                t.poses_in.copy_(t.poses_out)
            t.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


out = {"metric": "ms per frame, K objects x 1 hypothesis x %d iterations: one batched graphed tracker vs K single-object graphed trackers"
       % args.iters, "frames": args.frames, "warmup": args.warmup, "K": {}}
with torch.inference_mode():
    for K in ks:
        batched = GraphedTracker(refiner, gms[:K], diams[:K], sc["K"], syn.H, syn.W, n_hyp=1, iteration=args.iters, device=dev).capture()
        singles = [GraphedTracker(refiner, gms[k], diams[k], sc["K"], syn.H, syn.W, n_hyp=1, iteration=args.iters, device=dev).capture()
                   for k in range(K)]
        r = {}
        for rep in range(2):          # alternated, twice: the run-to-run spread is part of the record
            r.setdefault("batched_ms", []).append(run([batched], args.frames))
            r.setdefault("sequential_ms", []).append(run(singles, args.frames))
        b, s = min(r["batched_ms"]), min(r["sequential_ms"])
        out["K"][str(K)] = dict(batched_ms_per_frame=b, sequential_ms_per_frame=s, batched_over_sequential=b / s, runs=r)
        del batched, singles
if "8" in out["K"]:
    out["k8_batched_over_sequential"] = out["K"]["8"]["batched_over_sequential"]
    out["k8_bound_0.4_met"] = out["k8_batched_over_sequential"] <= 0.4
print(json.dumps(out))
