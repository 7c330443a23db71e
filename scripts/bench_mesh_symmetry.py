"""Cost of the symmetry detector's kernel (ops.mesh_transform_residuals: fp_mesh_transform_residuals' three launches) at the size of
the detector's coarse scan: --transforms rotations (800: one per candidate axis) of --samples surface samples (64) against the true can
(4 900 faces) and against the can fused from 16 device renders at 2.5 mm (about 84 k faces; --fused_faces 0 leaves it out).  Beside it
the same residuals the way they could be had without the kernel: the T x Q transformed points materialised in torch, one
ops.mesh_point_distance call over all of them, and amax over each transform's row; `same_bits` says whether the two routes gave the
same maxima (torch may contract the transform into fused multiply-adds, the kernel does not).  Then the whole detection of the true
can (reconstruct.detect_symmetries, wall clock, it synchronises at every step of its policy).  HIP events around warm back-to-back
calls that fill at least --window seconds (or --iters calls), the smaller of two runs.  Every figure is the time of a call through the
Python wrapper.  Prints one JSON line.

--accel grid adds, per mesh, the same call answered through a uniform grid (ops.mesh_grid_build, then mesh_transform_residuals(grid=))
in the same run: under "grid" the time of a build (the smallest of three, wall clock around a synchronised call), the time of a query
measured as above, the brute-force time of this run over it, the grid's shape and whether the maxima equal the brute force's bit for
bit; it also adds the can fused at the default pitch (128 voxels, about 400 k faces) to the meshes, and --out FILE writes the JSON
there too.  Without the flag the output is what it was."""
import argparse, json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from foundationpose_amd import ops, symmetry, synthetic as syn
from foundationpose_amd.reconstruct import detect_symmetries, reconstruct_object, sample_surface
from foundationpose_amd.Utils import get_mesh_handle

ap = argparse.ArgumentParser()
ap.add_argument("--transforms", type=int, default=800)
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--iters", type=int, default=0, help="time exactly this many calls instead of filling --window")
ap.add_argument("--views", type=int, default=16)
ap.add_argument("--fused_faces", type=int, default=1, help="0: leave the fused can out")
ap.add_argument("--skip_detection", action="store_true")
ap.add_argument("--accel", choices=("grid",), default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
sc = bench.build_scene(dev, 0, 1)
true = dict(pos=sc["gm"]["pos"], faces=sc["gm"]["faces"])


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = args.iters if args.iters > 0 else max(3, int(np.ceil(args.window * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def built(mesh):
    """-> (the grid of a mesh, the wall-clock ms of three builds)"""
    builds = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid = ops.mesh_grid_build(pos=mesh["pos"], faces=mesh["faces"])
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)
    return grid, builds


def case(name, mesh):
    """the coarse scan's call at order 2: half turns about --transforms axes through the surface's centroid"""
    T, Q, F = args.transforms, args.samples, int(mesh["faces"].shape[0])
    centre, _ = symmetry.surface_centre(mesh["pos"].cpu().numpy(), mesh["faces"].cpu().numpy())
    tfs = symmetry.about(centre, np.stack([symmetry.axis_rotation(a, math.pi) for a in symmetry.hemisphere_axes(T)]))
    tfs = torch.as_tensor(tfs.astype(np.float32), device=dev)
    pts, _ = sample_surface(mesh, Q, seed=1)
    out = dict(max_d2=torch.empty(T, device=dev))
    d2 = torch.empty(T * Q, device=dev)

    def fused():
        return ops.mesh_transform_residuals(pts, tfs, mesh, want=("max_d2",), out=out)["max_d2"]

    def materialised():
        moved = (pts[None] @ tfs[:, :3, :3].transpose(1, 2) + tfs[:, None, :3, 3]).reshape(T * Q, 3).contiguous()
        return ops.mesh_point_distance(moved, mesh, want=("dist2",), out=dict(dist2=d2))["dist2"].view(T, Q).amax(dim=1)

    a, b = fused().clone(), materialised().clone()
    runs_f = [timed(fused) for _ in range(2)]
    runs_m = [timed(materialised) for _ in range(2)]
    f_ms, m_ms = min(x[0] for x in runs_f), min(x[0] for x in runs_m)
    row = dict(name=name, faces=F, fused_ms=f_ms, materialised_ms=m_ms, ratio=m_ms / f_ms, reps=[runs_f[0][1], runs_m[0][1]],
               runs_ms=dict(fused=[x[0] for x in runs_f], materialised=[x[0] for x in runs_m]), pairs_per_s=T * Q * F / (f_ms * 1e-3),
               same_bits=bool(torch.equal(a, b)), largest_difference_m=float((a.double().sqrt() - b.double().sqrt()).abs().max()))
    if args.accel == "grid":
        grid, builds = built(mesh)
        through = lambda: ops.mesh_transform_residuals(pts, tfs, mesh, want=("max_d2",), out=out, grid=grid)["max_d2"]   # noqa: E731
        g = through().clone()
        runs_g = [timed(through) for _ in range(2)]
        g_ms = float(np.median([x[0] for x in runs_g]))
        row["grid"] = dict(build_ms=min(builds), builds_ms=builds, query_ms=g_ms, runs_ms=[x[0] for x in runs_g], reps=runs_g[0][1],
                           brute_ms=float(np.median([x[0] for x in runs_f])), brute_over_grid=float(np.median([x[0] for x in runs_f])) / g_ms,
                           cell_m=float(grid.h), cells=[int(x) for x in grid.n], n_entries=grid.n_entries, n_overflow=grid.n_overflow,
                           equal_bits=bool((g.view(torch.int32) == a.view(torch.int32)).all()))
    return row


out = {"metric": f"ms per call: the largest surface distance under each of {args.transforms} transforms of {args.samples} samples, fused kernel "
                 f"against transformed points in torch + ops.mesh_point_distance + amax", "transforms": args.transforms, "samples": args.samples,
       "cases": []}
with torch.inference_mode():
    out["cases"].append(case("true can", true))
    if args.fused_faces:
        V, H, W = args.views, syn.H, syn.W
        P = torch.as_tensor(syn.reference_view_poses(V, 0.5).astype(np.float32), device=dev)
        r = ops.render_crops(get_mesh_handle(sc["gm"]), P, None, sc["K"], H, W, (H, W), sc["diameter"], normalize_xyz=False, want=("color", "depth"))
        depth, rgb = r["depth"], (r["color"].clamp(0, 1) * 255).contiguous()
        Ks = np.tile(np.asarray(sc["K"], np.float64)[None], (V, 1, 1))
        mesh, t = reconstruct_object(rgb, depth, (depth > 0).to(torch.uint8), P, Ks, voxel=0.0025, device=dev)
        out["cases"].append(case("can fused at 2.5 mm", dict(pos=t["pos"], faces=t["faces"])))
        if args.accel == "grid":
            mesh, t = reconstruct_object(rgb, depth, (depth > 0).to(torch.uint8), P, Ks, voxel=None, device=dev)
            out["cases"].append(case("can fused at 128 voxels", dict(pos=t["pos"], faces=t["faces"])))
    if not args.skip_detection:
        detect_symmetries(true)                                      # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = detect_symmetries(true)
        torch.cuda.synchronize()
        out["detection"] = dict(mesh="true can", seconds=time.perf_counter() - t0, transforms=len(rec.tfs),
                                axes=["continuous" if k == math.inf else int(k) for _, k in rec.axes], tol_m=rec.tol,
                                largest_residual_m=float(rec.residuals.max()))
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
