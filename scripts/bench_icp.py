"""Cost of one point-to-plane ICP step (ops.icp_point_plane: fp_icp_point_plane's two launches) next to the render it follows
(ops.render_crops of the camera-frame xyz and normals), at N = 1, 64 and 252 hypotheses with 160 x 160 crops: perturbations of the
bench scene's pose against the frame's ingested depth.  Timing: HIP events around --reps back-to-back calls after --warmup calls, the
two ops alternated, twice.  Prints one JSON line (profiles/icp_polish.json keeps a run)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from foundationpose_amd import ops, synthetic as syn
from foundationpose_amd.crops import Scene
from foundationpose_amd.Utils import get_mesh_handle

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--sizes", default="1,64,252")
args = ap.parse_args()
dev = torch.device("cuda:0")
sc = bench.build_scene(dev, 0, 1)
gt, rgb_h, depth_h, _ = bench.make_sequence(dev, sc, 2)
xyz = ops.ingest_frame(torch.as_tensor(np.asarray(depth_h[0]), device=dev, dtype=torch.float).contiguous(), sc["K"])


def timed(fn):
    for _ in range(args.warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


out = {"metric": "ms per call, 160x160 crops: render_crops(want=xyz, normal) and the icp_point_plane that follows it", "reps": args.reps,
       "sizes": {}}
with torch.inference_mode():
    for N in (int(s) for s in args.sizes.split(",")):
        P = torch.as_tensor(syn.perturbed_poses(gt[0], N, seed=N, max_trans=0.008, max_rot_deg=4.0).astype(np.float32), device=dev)
        scene = Scene(get_mesh_handle(sc["gm"]), sc["diameter"], sc["K"], syn.H, syn.W, N)
        tf, bb = scene.crop_windows(P, 1.2, (160, 160))
        ws = scene.workspace(N, 160, 160, dev)
        r = scene.render_crops(P, bb, (160, 160), xyz_thr=0.001, normalize_xyz=False, want=("xyz", "normal"), workspace=ws)
        system = torch.empty((N, 40), dtype=torch.float64, device=dev)
        pout = torch.empty((N, 4, 4), dtype=torch.float32, device=dev)
        iws = ops.icp_workspace(N, 160, 160, dev)
        render = lambda: scene.render_crops(P, bb, (160, 160), xyz_thr=0.001, normalize_xyz=False, want=("xyz", "normal"), workspace=ws)
        icp = lambda: scene.icp_point_plane(r["xyz"], r["normal"], xyz, tf, P, 0.02, system=system, poses_out=pout, workspace=iws)
        runs = {"render_ms": [], "icp_ms": []}
        for _ in range(2):
            runs["render_ms"].append(timed(render))
            runs["icp_ms"].append(timed(icp))
        steps = ops.IcpStep.rows(system)
        out["sizes"][str(N)] = dict(render_ms=min(runs["render_ms"]), icp_ms=min(runs["icp_ms"]), runs=runs,
                                    pairs=[min(s.pairs for s in steps), max(s.pairs for s in steps)],
                                    solved=sum(s.status == 0 for s in steps))
print(json.dumps(out))
