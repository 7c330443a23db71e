"""Cost of looking at a TSDF volume without extracting it (ops.tsdf_raycast: fp_tsdf_raycast's one launch), on the can fused at 2.5 mm
from 16 device renders: one align_views_to_volume iteration for the 16 views at ICP_CROP (crop windows, raycast of xyz and normals,
one ICP step); the same iteration the way refine_view_poses makes it possible (TsdfVolume.extract with its host read, weld and mesh
handle, then crop windows, render_crops and the ICP step; and without the extraction, which a round pays once); the raycast alone; and
a full-frame 480 x 640 raycast of all four outputs.  Every figure is the time of a call through the Python wrapper (launches and their enqueue included), not a kernel
time from a trace: HIP events around --reps back-to-back calls after --warmup calls (windows of 0.5 s and more; the extraction
synchronises: wall clock over a tenth of the calls there), the smaller of two runs.  Prints one JSON line (profiles/tsdf_raycast.json
keeps a run under "bench")."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from foundationpose_amd import ops, synthetic as syn
from foundationpose_amd.reconstruct import ICP_CROP, ICP_CROP_RATIO, PAD_VOXELS, TsdfVolume, _AlignSide, bounds_from_views
from foundationpose_amd.Utils import get_mesh_handle

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10000)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--views", type=int, default=16)
ap.add_argument("--voxel", type=float, default=0.0025)
args = ap.parse_args()
dev = torch.device("cuda:0")
sc = bench.build_scene(dev, 0, 1)
V, H, W = args.views, syn.H, syn.W
poses = syn.reference_view_poses(V, 0.5).astype(np.float32)
P = torch.as_tensor(poses, device=dev)
r = ops.render_crops(get_mesh_handle(sc["gm"]), P, None, sc["K"], H, W, (H, W), sc["diameter"], normalize_xyz=False, want=("color", "depth"))
depth, rgb = r["depth"], (r["color"].clamp(0, 1) * 255).contiguous()
masks = (depth > 0).to(torch.uint8)
Ks = np.tile(np.asarray(sc["K"], np.float64)[None], (V, 1, 1))
lo, hi = bounds_from_views(depth, masks, P, Ks, PAD_VOXELS * args.voxel, device=dev)
nx, ny, nz = (int(np.ceil(e / args.voxel - 1e-9)) + 1 for e in (hi - lo))
vol = TsdfVolume(lo, (nz, ny, nx), args.voxel, device=dev)
vol.integrate(rgb, depth, masks, P, Ks)
side = _AlignSide(vol, depth, masks, Ks)
oh, ow = ICP_CROP


def timed(fn, wall=False):
    reps = max(args.reps // 10, 1) if wall else args.reps          # the extraction takes ten times as long a call: the same window
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps if wall else e0.elapsed_time(e1) / reps


with torch.inference_mode():
    tf, bb = ops.crop_windows(P, None, side.diam, ICP_CROP_RATIO, (ow, oh), views=side.vt)
    bufs = dict(xyz=torch.empty((V, oh, ow, 3), device=dev), normal=torch.empty((V, oh, ow, 3), device=dev))
    full = {k: torch.empty((1, H, W) + ((3,) if k != "depth" else ()), device=dev) for k in ops.RAYCAST_OUTPUTS}
    system, pout, iws = torch.empty((V, 40), dtype=torch.float64, device=dev), torch.empty((V, 4, 4), device=dev), ops.icp_workspace(V, oh, ow, dev)
    mesh, t = vol.extract()
    mset = ops.MeshSet([get_mesh_handle(t)])

    def raycast():
        return ops.tsdf_raycast(*vol.arrays(), vol.origin, vol.voxel, P, None, H, W, (oh, ow), bb, want=("xyz", "normal"), out=bufs, views=side.vt)

    def volume_iteration():
        tf, bb = ops.crop_windows(P, None, side.diam, ICP_CROP_RATIO, (ow, oh), views=side.vt)
        r = ops.tsdf_raycast(*vol.arrays(), vol.origin, vol.voxel, P, None, H, W, (oh, ow), bb, want=("xyz", "normal"), out=bufs, views=side.vt)
        ops.icp_point_plane(r["xyz"], r["normal"], side.xyz, tf, P, 0.01, views=side.vt, system=system, poses_out=pout, workspace=iws)

    def mesh_iteration(ms=mset):
        tf, bb = ops.crop_windows(P, None, side.diam, ICP_CROP_RATIO, (ow, oh), views=side.vt)
        r = ops.render_crops(ms, P, bb, None, H, W, (oh, ow), side.diam, normalize_xyz=False, want=("xyz", "normal"), views=side.vt)
        ops.icp_point_plane(r["xyz"], r["normal"], side.xyz, tf, P, 0.01, views=side.vt, system=system, poses_out=pout, workspace=iws)

    def extract_and_mesh_iteration():
        _, t2 = vol.extract()
        mesh_iteration(ops.MeshSet([get_mesh_handle(t2)]))

    def full_frame():
        return ops.tsdf_raycast(*vol.arrays(), vol.origin, vol.voxel, P[:1], sc["K"], H, W, out=full)

    runs = {k: [] for k in ("raycast_ms", "volume_iteration_ms", "mesh_iteration_ms", "extract_and_mesh_iteration_ms", "full_frame_ms")}
    for _ in range(2):
        runs["raycast_ms"].append(timed(raycast))
        runs["volume_iteration_ms"].append(timed(volume_iteration))
        runs["mesh_iteration_ms"].append(timed(mesh_iteration))
        runs["extract_and_mesh_iteration_ms"].append(timed(extract_and_mesh_iteration, wall=True))
        runs["full_frame_ms"].append(timed(full_frame))
    hits = int((raycast()["xyz"][..., 2] > 0).sum())
out = {"metric": f"ms per call: {V} views of the can at {oh}x{ow} crops against its {nz}x{ny}x{nx} volume at {args.voxel * 1e3:g} mm "
                 f"({len(mesh.faces)} faces extracted); full frame {H}x{W}, one pose, four outputs", "reps": args.reps, "hit_pixels": hits}
out.update({k: min(v) for k, v in runs.items()})
out["runs"] = runs
print(json.dumps(out))
