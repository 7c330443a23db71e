"""Cost of the mesh registration's kernel (ops.mesh_icp_step: fp_mesh_icp_step's four launches) at the size of the coarse stage of
reconstruct.align_meshes: --transforms start rotations (300) of --samples surface samples (128) of the true can against the true can
(4 900 faces) and against the can fused from 16 device renders at 2.5 mm (about 84 k faces; --fused_faces 0 leaves it out).  Beside it
the same step the way it could be had without the kernel (the materialised route): the T x Q transformed points in torch, one
ops.mesh_point_distance call over all of them with `face` and `closest`, the face normals, the rows and the 6 x 6 normal equations
in torch (float64 sums), solved with torch.linalg.solve; `largest_step_difference` is how far the two steps differ.  Then the whole
align_meshes of the displaced true can onto itself (wall clock; it synchronises once per stage and per gate).  HIP events around warm
back-to-back calls that fill at least --window seconds (or --iters calls), the smaller of two runs.  Every figure is the time of a call
through the Python wrapper.  Report only: nothing is gated on a time.  Prints one JSON line.

--accel grid adds, per mesh, the same step answered through a uniform grid (ops.mesh_grid_build, then mesh_icp_step(grid=)) in the
same run: under "grid" the time of a build (the smallest of three, wall clock around a synchronised call), the time of a step measured
as above, this run's brute-force time over it, the grid's shape, whether system and tfs_out equal the brute force's bit for bit, and
the same two steps on the samples sorted along a Morton curve by this script (`morton`: a rigid motion keeps neighbours neighbours,
so the lanes of a wave then walk nearby cells; recorded only, nothing in the package sorts), and under `near` the call of the fine
stage, 8 transforms of 2 048 samples, moved off the surface by a small rigid motion (0.5 degrees and 0.5 mm, 5 degrees and 5 mm): where
the grid is meant to pay.  It also adds the can fused at the default
pitch (128 voxels, about 400 k faces) to the meshes and align_meshes(accel="grid") to the alignment, and --out FILE writes the JSON
there too.  Without the flag the output is what it was."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from foundationpose_amd import mesh_align, ops, symmetry, synthetic as syn
from foundationpose_amd.reconstruct import align_meshes, reconstruct_object, sample_surface
from foundationpose_amd.Utils import get_mesh_handle

ap = argparse.ArgumentParser()
ap.add_argument("--transforms", type=int, default=300)
ap.add_argument("--samples", type=int, default=128)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--iters", type=int, default=0, help="time exactly this many calls instead of filling --window")
ap.add_argument("--views", type=int, default=16)
ap.add_argument("--fused_faces", type=int, default=1, help="0: leave the fused can out")
ap.add_argument("--skip_alignment", action="store_true")
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


def morton_order(pts):
    """the order of the points along a Morton curve of 10 bits an axis over their bounding box"""
    p = pts.cpu().numpy().astype(np.float64)
    q = np.minimum(((p - p.min(0)) / max(float((p.max(0) - p.min(0)).max()), 1e-30) * 1024).astype(np.int64), 1023)
    key = np.zeros(len(p), np.int64)
    for bit in range(10):
        for k in range(3):
            key |= ((q[:, k] >> bit) & 1) << (3 * bit + k)
    return torch.as_tensor(np.argsort(key, kind="stable"), device=pts.device)


def case(name, mesh):
    """one step of the coarse stage: the start rotations about the samples' centroid, put on the mesh's area centroid"""
    T, Q, F = args.transforms, args.samples, int(mesh["faces"].shape[0])
    pts, _ = sample_surface(true, Q, seed=1)
    centre, _ = symmetry.surface_centre(mesh["pos"].cpu().numpy(), mesh["faces"].cpu().numpy())
    tfs = mesh_align.start_transforms(mesh_align.start_rotations(T - 1, 0), pts.double().mean(dim=0).cpu().numpy(), centre)
    tfs = torch.as_tensor(tfs.astype(np.float32), device=dev)
    out = dict(tfs_out=torch.empty_like(tfs), system=torch.empty((T, 40), dtype=torch.float64, device=dev))
    ws = ops.mesh_icp_workspace(T, Q, dev)
    gate, damping = mesh_align.NO_GATE, 1e-3
    pos, faces = mesh["pos"], mesh["faces"].long()

    def fused():
        return ops.mesh_icp_step(pts, tfs, mesh, max_dist=gate, damping=damping, out=out, workspace=ws)[1]

    def materialised():
        p = (pts[None] @ tfs[:, :3, :3].transpose(1, 2) + tfs[:, None, :3, 3]).reshape(T * Q, 3).contiguous()
        near = ops.mesh_point_distance(p, mesh, want=("face", "closest"))
        tri = pos[faces[near["face"].long().clamp_(min=0)]]
        n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).double()
        m = n / n.norm(dim=1, keepdim=True)
        pair = (near["face"] >= 0) & torch.isfinite(m).all(dim=1)
        p64 = p.double()
        r = (m * (near["closest"].double() - p64)).sum(dim=1)
        J = torch.cat([torch.linalg.cross(p64 - tfs[:, None, :3, 3].expand(T, Q, 3).reshape(T * Q, 3).double(), m), m], dim=1)
        J = torch.where(pair[:, None], J, torch.zeros_like(J)).view(T, Q, 6)
        r = torch.where(pair, r, torch.zeros_like(r)).view(T, Q)
        A = J.transpose(1, 2) @ J
        b = (J * r[:, :, None]).sum(dim=1)
        A = A + damping * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
        return torch.linalg.solve(A, b)

    a, b = fused()[:, 30:36].clone(), materialised().clone()
    runs_f = [timed(fused) for _ in range(2)]
    runs_m = [timed(materialised) for _ in range(2)]
    f_ms, m_ms = min(x[0] for x in runs_f), min(x[0] for x in runs_m)
    row = dict(name=name, faces=F, fused_ms=f_ms, materialised_ms=m_ms, ratio=m_ms / f_ms, reps=[runs_f[0][1], runs_m[0][1]],
               runs_ms=dict(fused=[x[0] for x in runs_f], materialised=[x[0] for x in runs_m]), pairs_per_s=T * Q * F / (f_ms * 1e-3),
               largest_step_difference=float((a - b).abs().max()))
    if args.accel == "grid":
        grid, builds = built(mesh)
        step = lambda p, g: ops.mesh_icp_step(p, tfs, mesh, max_dist=gate, damping=damping, out=out, workspace=ws, grid=g)   # noqa: E731
        brute = [x.clone() for x in step(pts, None)]
        got = [x.clone() for x in step(pts, grid)]
        runs_g = [timed(lambda: step(pts, grid)) for _ in range(2)]
        b_ms, g_ms = float(np.median([x[0] for x in runs_f])), float(np.median([x[0] for x in runs_g]))
        sorted_pts = pts[morton_order(pts)].contiguous()
        m_brute, m_grid = [timed(lambda: step(sorted_pts, None)) for _ in range(2)], [timed(lambda: step(sorted_pts, grid)) for _ in range(2)]
        row["grid"] = dict(build_ms=min(builds), builds_ms=builds, query_ms=g_ms, runs_ms=[x[0] for x in runs_g], reps=runs_g[0][1],
                           brute_ms=b_ms, brute_over_grid=b_ms / g_ms, cell_m=float(grid.h), cells=[int(x) for x in grid.n],
                           n_entries=grid.n_entries, n_overflow=grid.n_overflow,
                           equal_bits=bool(torch.equal(got[0].view(torch.int32), brute[0].view(torch.int32))
                                           and torch.equal(got[1].view(torch.int64), brute[1].view(torch.int64))),
                           morton=dict(brute_ms=float(np.median([x[0] for x in m_brute])), query_ms=float(np.median([x[0] for x in m_grid]))),
                           near=[])
        fine, _ = sample_surface(true, 2048, seed=0)
        n_out = dict(tfs_out=torch.empty((8, 4, 4), device=dev), system=torch.empty((8, 40), dtype=torch.float64, device=dev))
        n_ws = ops.mesh_icp_workspace(8, 2048, dev)
        for deg, shift in ((0.5, 0.0005), (5.0, 0.005)):
            rng = np.random.default_rng(8)
            m = symmetry.about(centre, np.stack([symmetry.axis_rotation(rng.normal(size=3), np.radians(deg)) for _ in range(8)]))
            u = rng.normal(size=(8, 3))
            m[:, :3, 3] += shift * u / np.linalg.norm(u, axis=1, keepdims=True)
            m = torch.as_tensor(m.astype(np.float32), device=dev)
            near = lambda g: ops.mesh_icp_step(fine, m, mesh, max_dist=gate, damping=damping, out=n_out, workspace=n_ws, grid=g)   # noqa: E731
            n_brute = [x.clone() for x in near(None)]
            n_got = [x.clone() for x in near(grid)]
            t_b, t_g = [timed(lambda: near(None))[0] for _ in range(2)], [timed(lambda: near(grid))[0] for _ in range(2)]
            row["grid"]["near"].append(dict(degrees=deg, shift_m=shift, transforms=8, samples=2048, brute_ms=float(np.median(t_b)),
                                            query_ms=float(np.median(t_g)), brute_over_grid=float(np.median(t_b) / np.median(t_g)),
                                            equal_bits=bool(torch.equal(n_got[1].view(torch.int64), n_brute[1].view(torch.int64)))))
    return row


out = {"metric": f"ms per call: one point-to-plane step of {args.transforms} transforms of {args.samples} samples, fused kernel against "
                 f"transformed points in torch + ops.mesh_point_distance + normal equations in torch", "transforms": args.transforms,
       "samples": args.samples, "cases": []}
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
    if not args.skip_alignment:
        D = symmetry.about(np.array([0.01, -0.02, 0.03]), symmetry.axis_rotation((1.0, 2.0, 3.0), 2.0))
        D[:3, 3] += (0.2, -0.1, 0.3)
        moved = dict(pos=(true["pos"].double() @ torch.as_tensor(D[:3, :3].T, device=dev) + torch.as_tensor(D[:3, 3], device=dev)).float().contiguous(),
                     faces=true["faces"])
        align_meshes(moved, true)                                    # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = align_meshes(moved, true)
        torch.cuda.synchronize()
        out["alignment"] = dict(mesh="true can, displaced, onto itself", seconds=time.perf_counter() - t0, rmse_m=got.rmse, overlap=got.overlap,
                                mean_distance_m=got.mean_distance, status=got.status,
                                runner_up=None if got.runner_up is None else dict(cost_ratio=got.runner_up["cost"] / max(got.rmse ** 2, 1e-300),
                                                                                  angle_deg=got.runner_up["angle_deg"]))
        if args.accel == "grid":
            target = dict(true)                                          # the grid is kept in it
            fast = align_meshes(moved, target, accel="grid")             # warm, and the build
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fast = align_meshes(moved, target, accel="grid")
            torch.cuda.synchronize()
            out["alignment"]["grid"] = dict(seconds=time.perf_counter() - t0, faces=int(true["faces"].shape[0]),
                                            equal=bool(np.array_equal(fast.tf, got.tf) and repr(fast.rmse) == repr(got.rmse)))
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
