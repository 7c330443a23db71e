"""Cost of the ray-to-mesh query (ops.mesh_ray_cast: fp_mesh_ray_cast's three launches) and of the coverage report built on it:
--rays rays from the eyes of a ring of views towards surface samples of the true can, against the true can (4 900 faces) and against
the can fused from 16 device renders at 2.5 mm (about 86 k faces: the meshes of profiles/mesh_distance.json).  Beside each, in the same
process, ops.mesh_point_distance at the same Q x F: the sibling scan on the same LDS tile is the yardstick, there being no earlier ray
query to compare with.  HIP events around warm back-to-back calls that fill at least --window seconds, the smaller of two runs and
both runs.  Then reconstruct.view_coverage for the --views views x --rays samples against the fused can (a setup call that
synchronises: wall clock around it, the smaller of two).  Every figure is the time of a call through the Python wrapper.  Prints one
JSON line; --out FILE also writes it there (profiles/mesh_ray.json keeps a run)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from foundationpose_amd import ops, synthetic as syn
from foundationpose_amd.reconstruct import reconstruct_object, sample_surface, view_coverage
from foundationpose_amd.Utils import get_mesh_handle

# v_* instructions of the compiled inner loops per pair.  Not measured and not derived by this script: counted by hand in a hipcc -S
# listing (the Makefile's flags) of k_ray_scan (mesh_ray.hip) and k_scan (mesh_scan.hip) at the commit that added this script, the
# two-pair loop bodies halved; count again when either loop changes
VALU_INSTR_PER_PAIR = {"mesh_ray_cast": 81.5, "mesh_point_distance": 135.5}
VALU_INSTR_SOURCE = "counted by hand in a hipcc -S listing of k_ray_scan and k_scan at the commit that added bench_mesh_ray.py; not measured"

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=100_000)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--views", type=int, default=16)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
sc = bench.build_scene(dev, 0, 1)
V, H, W = args.views, syn.H, syn.W
poses = syn.reference_view_poses(V, 0.5)
P = torch.as_tensor(poses.astype(np.float32), device=dev)
r = ops.render_crops(get_mesh_handle(sc["gm"]), P, None, sc["K"], H, W, (H, W), sc["diameter"], normalize_xyz=False, want=("color", "depth"))
depth, rgb = r["depth"], (r["color"].clamp(0, 1) * 255).contiguous()
masks = (depth > 0).to(torch.uint8)
Ks = np.tile(np.asarray(sc["K"], np.float64)[None], (V, 1, 1))
true = dict(pos=sc["gm"]["pos"], faces=sc["gm"]["faces"])
points, _ = sample_surface(true, args.rays)
P64 = poses.astype(np.float64)
eyes = torch.as_tensor((-np.einsum("vji,vj->vi", P64[:, :3, :3], P64[:, :3, 3])).astype(np.float32), device=dev)
origins = eyes[torch.arange(args.rays, device=dev) % V].contiguous()          # ray i leaves the eye of view i mod V
dirs = (points - origins).contiguous()


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(3, int(np.ceil(args.window * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


out = {"metric": f"ms per call of ops.mesh_ray_cast (t, face, bary, hit) for {args.rays} rays from {V} eyes towards surface samples of the "
                 f"true can, and of ops.mesh_point_distance (dist2, face, closest) for those samples, against the same mesh",
       "valu_instr_per_pair": VALU_INSTR_PER_PAIR, "valu_instr_per_pair_source": VALU_INSTR_SOURCE, "sizes": {}}
with torch.inference_mode():
    mesh, fused = reconstruct_object(rgb, depth, masks, P, Ks, voxel=0.0025, device=dev)
    for name, t in (("can_true", true), ("can_2.5mm", fused)):
        F, R = int(t["faces"].shape[0]), args.rays
        rb = dict(t=torch.empty(R, device=dev), face=torch.empty(R, dtype=torch.int32, device=dev), bary=torch.empty((R, 2), device=dev),
                  hit=torch.empty((R, 3), device=dev))
        db = dict(dist2=torch.empty(R, device=dev), face=torch.empty(R, dtype=torch.int32, device=dev), closest=torch.empty((R, 3), device=dev))
        ray_runs = [timed(lambda: ops.mesh_ray_cast(origins, dirs, t, out=rb)) for _ in range(2)]
        dist_runs = [timed(lambda: ops.mesh_point_distance(points, t, out=db)) for _ in range(2)]
        ray_ms, dist_ms = min(x[0] for x in ray_runs), min(x[0] for x in dist_runs)
        out["sizes"][name] = dict(
            R=R, F=F, ray_ms=ray_ms, ray_runs_ms=[x[0] for x in ray_runs], ray_reps=ray_runs[0][1],
            ray_spread=abs(ray_runs[0][0] - ray_runs[1][0]) / ray_ms, ray_ns_per_pair=ray_ms * 1e6 / (R * F),
            distance_ms=dist_ms, distance_runs_ms=[x[0] for x in dist_runs], distance_reps=dist_runs[0][1],
            distance_spread=abs(dist_runs[0][0] - dist_runs[1][0]) / dist_ms, distance_ns_per_pair=dist_ms * 1e6 / (R * F),
            ray_over_distance=ray_ms / dist_ms, rays_that_hit=float((rb["face"] >= 0).float().mean()))
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cov = view_coverage(fused, P64, Ks, (H, W), samples=args.rays)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    F = int(fused["faces"].shape[0])
    out["view_coverage"] = dict(views=V, samples=args.rays, F=F, ms=min(walls), runs_ms=walls, spread=abs(walls[0] - walls[1]) / min(walls),
                                ns_per_pair=min(walls) * 1e6 / (V * args.rays * F), report=cov.as_dict(), describe=cov.describe())
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
