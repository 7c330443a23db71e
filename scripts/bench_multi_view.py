"""Several camera streams: ONE batched graphed tracker over V views (graphs.GraphedTracker with views, one object per view, 1 hypothesis,
2 refine iterations -- what estimater.track_views replays) against V single-object graphed trackers run one after the other, each on
its own view's frame (V x track_one with track_graph=True).  V in {1, 2, 4, 8}, plus a mixed case of 4 views x 2 objects (8 single
trackers against one batched tracker).

Per frame both sides upload every view's uint8 colour image and float depth map from pinned host memory (the batched tracker into its
frame stack, then one 3-launch ingest of all views; every single tracker its own frame and its own ingest) and track from their previous
output.  View v plays bench.make_sequence's synthetic sequence shifted by v frames, seen through its own K (focal length and principal
point varied per view).  Timing: synchronised host clock over --frames frames after --warmup frames, both sides alternated, twice.
Prints one JSON line."""
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
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--vs", default="1,2,4,8")
ap.add_argument("--iters", type=int, default=2)
ap.add_argument("--no-mixed", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
vs = [int(v) for v in args.vs.split(",")]
sc = bench.build_scene(dev, 0, 1)
F = args.frames + args.warmup
gt, rgb_h, depth_h, _ = bench.make_sequence(dev, sc, F + max(vs + [4]))
refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
meshes = [make_can_mesh(radius=0.03 + 0.004 * k, height=0.08 + 0.01 * k, n_ang=30 + 6 * k, n_axial=16 + 4 * k, textured=k % 2 == 0,
                        tex_size=256, seed=k) for k in range(2)]
gms = [make_mesh_tensors(m, device=dev) for m in meshes]
diams = [float(np.linalg.norm(m.vertices.max(0) - m.vertices.min(0))) for m in meshes]
K0 = np.asarray(sc["K"], dtype=np.float64)


def K_of(v):
    K = K0.copy()
    K[0, 0] *= 1.0 + 0.02 * v
    K[1, 1] *= 1.0 + 0.02 * v
    K[0, 2] += 1.5 * v
    K[1, 2] -= 1.25 * v
    return K


start = torch.as_tensor(gt[0], device=dev, dtype=torch.float32)


def run(trackers, n):
    """n frames through `trackers` = [(tracker, [view of each frame slot])]: each uploads its views' frames itself, then replays
    -> ms per frame"""
    rgb_u8 = torch.empty((syn.H, syn.W, 3), dtype=torch.uint8, device=dev)
    for t, _ in trackers:
        t.poses_in.copy_(start.expand(t.N, 4, 4))
    torch.cuda.synchronize()
    t0 = None
    for f in range(n + args.warmup):
        if f == args.warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for t, views in trackers:
            stacked = t.views is not None
            for s, v in enumerate(views):
                rgb_u8.copy_(rgb_h[f + v], non_blocking=True)
                (t.rgb[s] if stacked else t.rgb).copy_(rgb_u8)
                (t.depth[s] if stacked else t.depth).copy_(depth_h[f + v], non_blocking=True)
            if f:
                t.poses_in.copy_(t.poses_out)
            t.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def case(V, per_view):
    """V views x per_view objects: one batched tracker against V * per_view single trackers"""
    objs = [k % 2 for _ in range(V) for k in range(per_view)]
    views = [v for v in range(V) for _ in range(per_view)]
    batched = GraphedTracker(refiner, [gms[o] for o in objs], [diams[o] for o in objs], [K_of(v) for v in range(V)], syn.H, syn.W,
                             n_hyp=1, iteration=args.iters, device=dev, views=views).capture()
    singles = [(GraphedTracker(refiner, gms[o], diams[o], K_of(v), syn.H, syn.W, n_hyp=1, iteration=args.iters, device=dev).capture(), [v])
               for o, v in zip(objs, views)]
    r = {}
    for _ in range(2):          # alternated, twice: the run-to-run spread is part of the record
        r.setdefault("batched_ms", []).append(run([(batched, list(range(V)))], args.frames))
        r.setdefault("sequential_ms", []).append(run(singles, args.frames))
    b, s = min(r["batched_ms"]), min(r["sequential_ms"])
    return dict(batched_ms_per_frame=b, sequential_ms_per_frame=s, batched_over_sequential=b / s, runs=r)


out = {"metric": "ms per frame, V views x 1 object x 1 hypothesis x %d iterations: one batched graphed tracker vs V single-object "
       "graphed trackers" % args.iters, "frames": args.frames, "warmup": args.warmup, "V": {}}
with torch.inference_mode():
    for V in vs:
        out["V"][str(V)] = case(V, 1)
    if not args.no_mixed:
        out["mixed_4views_x_2objects"] = case(4, 2)
if "1" in out["V"]:
    out["v1_within_5pct"] = out["V"]["1"]["batched_over_sequential"] <= 1.05
if "8" in out["V"]:
    out["v8_batched_over_sequential"] = out["V"]["8"]["batched_over_sequential"]
    out["v8_at_most_half"] = out["v8_batched_over_sequential"] <= 0.5
print(json.dumps(out))
