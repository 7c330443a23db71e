"""Cost of the sign: ops.mesh_signed_distance against ops.mesh_point_distance at --queries points (100 000), and ops.mesh_penetration
against ops.mesh_transform_residuals at --transforms x --samples pairs (300 x 128), each against the true can (4 900 faces) and against
the can fused from 16 device renders at 2.5 mm (about 85 k faces; --fused_faces 0 leaves it out).  The scan is one copy of the code
(csrc/mesh_closest.h), so what the signed call may cost over its sibling is its finish launch: the walk of the winning face again,
the table read and one dot product a pair -- and, for the penetration, 64-bit keys in the place of mesh_transform_residuals' 32-bit
cells.  The two of a pair are timed in turns (--rounds of signed, sibling, signed, sibling, ...), each turn HIP events around warm
back-to-back calls that fill --window seconds; the figure is the median of the turns, the spread their (max - min) / median.  Every
figure is the time of a call through the Python wrapper.  Prints one JSON line and writes it into --out (profiles/mesh_signed.json)
under "bench", keeping what else the file holds.

--accel grid adds, per mesh, the same penetration call answered through a uniform grid (ops.mesh_grid_build, then
mesh_penetration(grid=)) in the same run: under "grid" the time of a build (the smallest of three, wall clock around a synchronised
call), the time of a call (the median of --rounds turns), this run's brute-force time over it, the grid's shape and whether inside,
depth2 and deepest equal the brute force's bit for bit; and under "far" the same call with every placement moved three extents of the
mesh away from it, where each lane walks the whole grid and tests every stored triangle: the brute-force time, and the grid's unless
its time, estimated from the first four placements, is above --far_limit times the brute force's (then `skipped` says so).  It also
adds the can fused at the default pitch (128 voxels, about 400 k faces) to the meshes.  Without the flag the output is what it was."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from foundationpose_amd import ops, synthetic as syn
from foundationpose_amd.reconstruct import reconstruct_object, sample_surface
from foundationpose_amd.Utils import get_mesh_handle

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=100_000)
ap.add_argument("--transforms", type=int, default=300)
ap.add_argument("--samples", type=int, default=128)
ap.add_argument("--window", type=float, default=0.3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--views", type=int, default=16)
ap.add_argument("--fused_faces", type=int, default=1, help="0: leave the fused can out")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mesh_signed.json"), help="'' writes no file")
ap.add_argument("--accel", choices=("grid",), default=None)
ap.add_argument("--far_limit", type=float, default=2000.0, help="the far placements through the grid may take this many brute-force calls")
args = ap.parse_args()
dev = torch.device("cuda:0")
sc = bench.build_scene(dev, 0, 1)


def timed(fn):
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
    return e0.elapsed_time(e1) / reps


def in_turns(signed, sibling):
    for fn in (signed, sibling):
        for _ in range(3):
            fn()
    runs = {"signed": [], "sibling": []}
    for _ in range(args.rounds):
        runs["signed"].append(timed(signed))
        runs["sibling"].append(timed(sibling))
    med = {k: float(np.median(v)) for k, v in runs.items()}
    return dict(signed_ms=med["signed"], sibling_ms=med["sibling"], ratio=med["signed"] / med["sibling"], runs_ms=runs,
                spread={k: (max(v) - min(v)) / med[k] for k, v in runs.items()})


def case(name, mesh):
    mesh = dict(pos=mesh["pos"], faces=mesh["faces"])
    tables = ops.mesh_pseudonormals(mesh)                                         # kept in the dict: not part of a timed call
    F = int(mesh["faces"].shape[0])
    lo, hi = mesh["pos"].amin(dim=0), mesh["pos"].amax(dim=0)
    g = torch.Generator(device="cpu").manual_seed(0)
    q = ((lo + hi) / 2 + (torch.rand((args.queries, 3), generator=g).to(dev) - 0.5) * 1.5 * (hi - lo)).contiguous()
    names = ("dist2", "face", "closest", "feature", "sign")
    o_s = {k: torch.empty((args.queries, 3) if k == "closest" else (args.queries,), dtype=ops._MESH_SIGNED_DTYPES[k], device=dev) for k in names}
    o_u = {k: torch.empty_like(o_s[k]) for k in names[:3]}
    dist = in_turns(lambda: ops.mesh_signed_distance(q, mesh, want=names, out=o_s, allow_open=True),
                    lambda: ops.mesh_point_distance(q, mesh, want=names[:3], out=o_u))
    dist.update(Q=args.queries, same_bits=bool(all(torch.equal(o_s[k], o_u[k]) for k in names[:3])),
                inside=float((o_s["sign"] < 0).float().mean()))
    # placements of the mesh's own samples: small seeded rigid motions, so that a part of every sample set is inside
    T, Q = args.transforms, args.samples
    pts, _ = sample_surface(mesh, Q, seed=1)
    rng = np.random.default_rng(0)
    tfs = np.tile(np.eye(4), (T, 1, 1))
    for t in range(T):
        w = rng.normal(size=3) * 0.2
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        tfs[t, :3, :3] = np.eye(3) + K + K @ K / 2
        u, _, vt = np.linalg.svd(tfs[t, :3, :3])
        tfs[t, :3, :3] = u @ vt
        tfs[t, :3, 3] = rng.normal(size=3) * 0.01
    tfs = torch.as_tensor(tfs.astype(np.float32), device=dev)
    o_p = dict(inside=torch.empty(T, dtype=torch.int32, device=dev), depth2=torch.empty(T, device=dev),
               deepest=torch.empty(T, dtype=torch.int32, device=dev))
    o_r = dict(max_d2=torch.empty(T, device=dev))
    ws = ops.mesh_penetration_workspace(T, Q, dev)
    pen = in_turns(lambda: ops.mesh_penetration(pts, tfs, mesh, out=o_p, workspace=ws, allow_open=True),
                   lambda: ops.mesh_transform_residuals(pts, tfs, mesh, want=("max_d2",), out=o_r))
    pen.update(T=T, Q=Q, inside_share=float(o_p["inside"].float().mean() / Q))
    row = dict(name=name, faces=F, closed=tables.closed, distance=dist, penetration=pen)
    if args.accel == "grid":
        builds = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grid = ops.mesh_grid_build(pos=mesh["pos"], faces=mesh["faces"])
            torch.cuda.synchronize()
            builds.append((time.perf_counter() - t0) * 1e3)
        call = lambda m, g, o=o_p, w=ws: ops.mesh_penetration(pts, m, mesh, out=o, workspace=w, allow_open=True, grid=g)   # noqa: E731
        brute = {k: v.clone() for k, v in call(tfs, None).items()}
        got = {k: v.clone() for k, v in call(tfs, grid).items()}
        for _ in range(3):
            call(tfs, grid)
        runs = [timed(lambda: call(tfs, grid)) for _ in range(args.rounds)]
        g_ms = float(np.median(runs))
        row["grid"] = dict(build_ms=min(builds), builds_ms=builds, query_ms=g_ms, runs_ms=runs, brute_ms=pen["signed_ms"],
                           brute_over_grid=pen["signed_ms"] / g_ms, cell_m=float(grid.h), cells=[int(x) for x in grid.n],
                           n_entries=grid.n_entries, n_overflow=grid.n_overflow,
                           equal_bits=all(bool((got[k].view(torch.int32) == brute[k].view(torch.int32)).all()) for k in brute))
        # every placement three extents away along x: each lane walks every shell and tests every stored triangle from global memory
        far = tfs.clone()
        far[:, 0, 3] += 3.0 * float((hi - lo).max())
        b_ms = float(np.median([timed(lambda: call(far, None)) for _ in range(args.rounds)]))
        few = far[:min(4, T)].contiguous()
        o4 = {k: v[:min(4, T)].clone() for k, v in o_p.items()}
        call(few, grid, o4, ws)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(few, grid, o4, ws)
        torch.cuda.synchronize()
        estimate = (time.perf_counter() - t0) * 1e3 * max(1.0, T / 4)
        row["far"] = dict(offset_m=3.0 * float((hi - lo).max()), brute_ms=b_ms, estimate_ms=estimate, limit_ms=args.far_limit * b_ms)
        if estimate > args.far_limit * b_ms:
            row["far"]["skipped"] = "the estimate from four placements is above the limit"
        else:
            brute = {k: v.clone() for k, v in call(far, None).items()}
            got = {k: v.clone() for k, v in call(far, grid).items()}
            torch.cuda.synchronize()
            times = []
            for _ in range(args.rounds):                                  # single calls: one may take seconds
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(far, grid)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            row["far"].update(query_ms=float(np.median(times)), runs_ms=times, grid_over_brute=float(np.median(times)) / b_ms,
                              equal_bits=all(bool((got[k].view(torch.int32) == brute[k].view(torch.int32)).all()) for k in brute))
    return row


out = {"metric": "ms per call, signed against unsigned sibling in turns: ops.mesh_signed_distance (all five outputs) / ops.mesh_point_distance "
                 "(all three); ops.mesh_penetration (inside, depth2, deepest) / ops.mesh_transform_residuals (max_d2)", "cases": []}
with torch.inference_mode():
    out["cases"].append(case("true can", sc["gm"]))
    if args.fused_faces:
        V, H, W = args.views, syn.H, syn.W
        P = torch.as_tensor(syn.reference_view_poses(V, 0.5).astype(np.float32), device=dev)
        r = ops.render_crops(get_mesh_handle(sc["gm"]), P, None, sc["K"], H, W, (H, W), sc["diameter"], normalize_xyz=False, want=("color", "depth"))
        depth, rgb = r["depth"], (r["color"].clamp(0, 1) * 255).contiguous()
        Ks = np.tile(np.asarray(sc["K"], np.float64)[None], (V, 1, 1))
        mesh, t = reconstruct_object(rgb, depth, (depth > 0).to(torch.uint8), P, Ks, voxel=0.0025, device=dev, keep_components="largest")
        out["cases"].append(case("can fused at 2.5 mm", t))
        if args.accel == "grid":
            mesh, t = reconstruct_object(rgb, depth, (depth > 0).to(torch.uint8), P, Ks, voxel=None, device=dev, keep_components="largest")
            out["cases"].append(case("can fused at 128 voxels", t))
print(json.dumps(out))
if args.out:
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["bench"] = out
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
