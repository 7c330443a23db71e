"""Cost of the depth-agreement check in the graphed trackers: ms per frame of a GraphedTracker built without and with agreement_tol
(the check runs inside each part's graph after the last refine iteration: crop windows, the depth render, the zeroing of the table and
fp_depth_agreement), both replaying the same frames, alternated, twice.  Three shapes, 1 hypothesis per object, 2 refine iterations:
track_one (one object), track_objects with K = 8 objects, track_views with 4 views x 2 objects.

Per frame both sides upload every view's uint8 colour image and float depth map from pinned host memory and track from their previous
output (bench.make_sequence's synthetic sequence; view v plays it shifted by v frames through its own K).  Timing: synchronised host
clock over --frames frames after --warmup frames.  Prints one JSON line."""
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
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--iters", type=int, default=2)
ap.add_argument("--tol", type=float, default=0.01)
ap.add_argument("--cases", default="track_one,track_objects_8,track_views_4x2")
args = ap.parse_args()
dev = torch.device("cuda:0")
sc = bench.build_scene(dev, 0, 1)
F = args.frames + args.warmup
gt, rgb_h, depth_h, _ = bench.make_sequence(dev, sc, F + 4)
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


def run(t, n):
    """n frames through tracker t (uploads its views' frames itself, then replays) -> ms per frame"""
    rgb_u8 = torch.empty((syn.H, syn.W, 3), dtype=torch.uint8, device=dev)
    t.poses_in.copy_(start.expand(t.N, 4, 4))
    stacked = t.views is not None
    V = t.V if stacked else 1
    torch.cuda.synchronize()
    t0 = None
    for f in range(n + args.warmup):
        if f == args.warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for v in range(V):
            rgb_u8.copy_(rgb_h[f + v], non_blocking=True)
            (t.rgb[v] if stacked else t.rgb).copy_(rgb_u8)
            (t.depth[v] if stacked else t.depth).copy_(depth_h[f + v], non_blocking=True)
        if f:
            t.poses_in.copy_(t.poses_out)
        t.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def trackers(name, tol):
    kw = dict(n_hyp=1, iteration=args.iters, device=dev, agreement_tol=tol)
    if name == "track_one":
        return GraphedTracker(refiner, gms[0], diams[0], K0, syn.H, syn.W, **kw).capture()
    if name == "track_objects_8":
        objs = [k % 2 for k in range(8)]
        return GraphedTracker(refiner, [gms[o] for o in objs], [diams[o] for o in objs], K0, syn.H, syn.W, **kw).capture()
    if name == "track_views_4x2":
        views = [v for v in range(4) for _ in range(2)]
        objs = [k % 2 for k in range(8)]
        return GraphedTracker(refiner, [gms[o] for o in objs], [diams[o] for o in objs], [K_of(v) for v in range(4)], syn.H, syn.W,
                              views=views, **kw).capture()
    raise ValueError(name)


out = {"metric": "graphed ms per frame without / with the depth-agreement check (agreement_tol=%g), 1 hypothesis per object, %d "
       "iterations" % (args.tol, args.iters), "frames": args.frames, "warmup": args.warmup, "cases": {}}
with torch.inference_mode():
    for name in args.cases.split(","):
        off, on = trackers(name, None), trackers(name, args.tol)
        r = {}
        for _ in range(2):          # alternated, twice: the run-to-run spread is part of the record
            r.setdefault("off_ms", []).append(run(off, args.frames))
            r.setdefault("on_ms", []).append(run(on, args.frames))
        a, b = min(r["off_ms"]), min(r["on_ms"])
        out["cases"][name] = dict(off_ms_per_frame=a, on_ms_per_frame=b, added_ms=b - a, added_frac=(b - a) / a, runs=r,
                                  last_agreement=on.agreement.cpu().numpy().tolist())
print(json.dumps(out))
