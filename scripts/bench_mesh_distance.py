"""Cost of the exact point-to-mesh distance (ops.mesh_point_distance: fp_mesh_point_distance's three launches): --queries surface
samples of the true can against the can fused from 16 device renders at 2.5 mm (about 84 k faces) and at the default pitch of 128 voxels
on the longest side (about 371 k faces).  HIP events around warm back-to-back calls that fill at least --window seconds, the smaller of
two runs; beside it the time Q x F x OPS_PER_PAIR float32 operations take at half the datasheet's 157.3 TFLOP/s.  That figure is the
rate of unpacked fused multiply-adds (a SIMD is 32 lanes wide, a wave's instruction issues in 2 cycles: 64 FLOP a cycle and SIMD), so
one unfused operation per lane and instruction runs at half of it, 78.65e12 a second; and the ratio of the two.  The same rate times
VALU_INSTR_PER_PAIR, the vector instructions the compiled inner loop holds per pair (271 in its two-pair body: the counted
operations, 16 comparisons, 23 selects and the expansion of the one division), gives the time the issue of those instructions
alone would take.  Every figure is the time of a call through the Python wrapper.  --host Q F also times the numpy restatement at
a size it can finish.  Prints one JSON line (profiles/mesh_distance.json keeps a run under "bench").

--accel grid adds, per size, the same call answered through a uniform grid (ops.mesh_grid_build, then mesh_point_distance(grid=)):
under "grid" the time of a build (the smaller of three, wall clock around a synchronised call: it reads the header back), the time of
a query measured as above, the grid's shape and list lengths, and whether the three outputs equal the brute force's bit for bit;
--out FILE also writes the JSON there (profiles/mesh_grid.json keeps a run)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from foundationpose_amd import ops, synthetic as syn
from foundationpose_amd.reconstruct import reconstruct_object, sample_surface
from foundationpose_amd.Utils import get_mesh_handle

OPS_PER_PAIR = 81             # the float32 operations of the definition (include/fp_amd.h), a division counted as one
VALU_INSTR_PER_PAIR = 135.5   # v_* instructions of k_scan's inner loop (mesh_scan.hip) per pair (hipcc -S with the Makefile's flags)
VALU_OPS_PER_S = 157.3e12 / 2   # one unfused float32 operation a lane and instruction

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=100_000)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--views", type=int, default=16)
ap.add_argument("--host", type=int, nargs=2, default=(1000, 4900), metavar=("Q", "F"))
ap.add_argument("--accel", choices=("grid",), default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
sc = bench.build_scene(dev, 0, 1)
V, H, W = args.views, syn.H, syn.W
P = torch.as_tensor(syn.reference_view_poses(V, 0.5).astype(np.float32), device=dev)
r = ops.render_crops(get_mesh_handle(sc["gm"]), P, None, sc["K"], H, W, (H, W), sc["diameter"], normalize_xyz=False, want=("color", "depth"))
depth, rgb = r["depth"], (r["color"].clamp(0, 1) * 255).contiguous()
masks = (depth > 0).to(torch.uint8)
Ks = np.tile(np.asarray(sc["K"], np.float64)[None], (V, 1, 1))
queries, _ = sample_surface(dict(pos=sc["gm"]["pos"], faces=sc["gm"]["faces"]), args.queries)


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


out = {"metric": f"ms per call of ops.mesh_point_distance (dist2, face, closest): {args.queries} samples of the true can against the can "
                 f"fused from {V} views", "ops_per_pair": OPS_PER_PAIR, "valu_instr_per_pair": VALU_INSTR_PER_PAIR, "valu_ops_per_s": VALU_OPS_PER_S,
       "sizes": {}}
with torch.inference_mode():
    for name, voxel in (("can_2.5mm", 0.0025), ("can_128", None)):
        mesh, t = reconstruct_object(rgb, depth, masks, P, Ks, voxel=voxel, device=dev)
        F = int(t["faces"].shape[0])
        bufs = dict(dist2=torch.empty(args.queries, device=dev), face=torch.empty(args.queries, dtype=torch.int32, device=dev),
                    closest=torch.empty((args.queries, 3), device=dev))
        runs = [timed(lambda: ops.mesh_point_distance(queries, t, out=bufs)) for _ in range(2)]
        only_d2 = timed(lambda: ops.mesh_point_distance(queries, t, want=("dist2",), out=dict(dist2=bufs["dist2"])))[0]
        ms = min(x[0] for x in runs)
        valu_ms = args.queries * F * OPS_PER_PAIR / VALU_OPS_PER_S * 1e3
        out["sizes"][name] = dict(Q=args.queries, F=F, voxel_m=mesh.voxel, ms=ms, runs_ms=[x[0] for x in runs], reps=runs[0][1],
                                  dist2_only_ms=only_d2, valu_ms_at_datasheet_rate=valu_ms, ratio=ms / valu_ms,
                                  valu_issue_ms=valu_ms * VALU_INSTR_PER_PAIR / OPS_PER_PAIR,
                                  valu_issue_fraction=valu_ms * VALU_INSTR_PER_PAIR / OPS_PER_PAIR / ms,
                                  pairs_per_s=args.queries * F / (ms * 1e-3),
                                  median_distance_m=float(bufs["dist2"].sqrt().median()))
        if args.accel == "grid":
            brute = {k: v.clone() for k, v in ops.mesh_point_distance(queries, t, out=bufs).items()}
            builds = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                grid = ops.mesh_grid_build(pos=t["pos"], faces=t["faces"])
                torch.cuda.synchronize()
                builds.append((time.perf_counter() - t0) * 1e3)
            g_runs = [timed(lambda: ops.mesh_point_distance(queries, t, out=bufs, grid=grid)) for _ in range(2)]
            g_d2 = timed(lambda: ops.mesh_point_distance(queries, t, want=("dist2",), out=dict(dist2=bufs["dist2"]), grid=grid))[0]
            got = ops.mesh_point_distance(queries, t, out=bufs, grid=grid)
            g_ms = min(x[0] for x in g_runs)
            out["sizes"][name]["grid"] = dict(
                build_ms=min(builds), builds_ms=builds, query_ms=g_ms, runs_ms=[x[0] for x in g_runs], reps=g_runs[0][1], dist2_only_ms=g_d2,
                brute_over_grid=ms / g_ms, cell_m=float(grid.h), cells=[int(x) for x in grid.n], pad_m=float(grid.pad),
                n_entries=grid.n_entries, n_overflow=grid.n_overflow, entries_per_face=grid.n_entries / max(F, 1),
                equal_bits=all(bool((got[k].view(torch.int32) == brute[k].view(torch.int32)).all()) for k in brute))
# the restatement on the host, at a size it can finish
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_distance_model as mm
Qh, Fh = args.host
pos, faces = sc["gm"]["pos"].cpu().numpy(), sc["gm"]["faces"].cpu().numpy()[:Fh]
t0 = time.perf_counter()
mm.mesh_point_distance(pos, faces, queries[:Qh].cpu().numpy())
dt = time.perf_counter() - t0
out["host_restatement"] = dict(Q=Qh, F=len(faces), seconds=dt, pairs_per_s=Qh * len(faces) / dt)
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
