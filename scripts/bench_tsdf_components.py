"""Cost of labelling a volume's surface components (ops.tsdf_components: fp_tsdf_label_components' three launches) next to the
extraction it filters (ops.tsdf_extract: count, emit and torch.unique, the yardstick), on two volumes: the can fused at 2.5 mm from 16
device renders into its 48 x 48 x 64 volume, and a 256^3 volume holding a sphere shell (radius 100 voxels) plus a thousand blobs
of radius 2.2 voxels.  Every figure is the time of a call through the Python wrapper (launches, their enqueue and the allocation of
the outputs included), not a kernel time from a trace: HIP events around back-to-back calls after --warmup calls, as many as fill
--window seconds (0.5 s and more; the extraction synchronises: wall clock there), the smaller of two runs.  Prints one JSON line
and, with --out FILE, keeps it in that file under --variant: an A/B build is loaded through FP_AMD_LIB (profiles/tsdf_components.json
holds the product next to builds of csrc/tsdf_components.hip without the ballot of its init pass, tc_noballot, without the wave sum
of its flatten pass, tc_nowave, and with neither, tc_plain: all slower, so the source keeps no switch for them)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from foundationpose_amd import _lib, ops, synthetic as syn
from foundationpose_amd.reconstruct import TsdfVolume
from foundationpose_amd.Utils import get_mesh_handle

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=0.6, help="seconds of back-to-back calls per measurement")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--big", type=int, default=256, help="side of the second volume, voxels")
ap.add_argument("--blobs", type=int, default=1000)
ap.add_argument("--variant", type=str, default="product", help="the key of this run in --out")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")


def can_volume():
    sc = bench.build_scene(dev, 0, 1)
    V, H, W, s = 16, syn.H, syn.W, 0.0025
    P = torch.as_tensor(syn.reference_view_poses(V, 0.5).astype(np.float32), device=dev)
    r = ops.render_crops(get_mesh_handle(sc["gm"]), P, None, sc["K"], H, W, (H, W), sc["diameter"], normalize_xyz=False, want=("color", "depth"))
    depth, rgb = r["depth"], (r["color"].clamp(0, 1) * 255).contiguous()
    dims = (64, 48, 48)
    lo = -np.asarray([dims[2] - 1, dims[1] - 1, dims[0] - 1]) * s / 2
    vol = TsdfVolume(lo, dims, s, device=dev)
    vol.integrate(rgb, depth, (depth > 0).to(torch.uint8), P, np.tile(np.asarray(sc["K"], np.float64)[None], (V, 1, 1)))
    return vol


def shell_and_blobs(n, blobs, radius=2.2, reach=4):
    """a sphere (radius 0.39 n voxels about the middle) plus `blobs` balls at seeded places off it, as distances in units of trunc"""
    vol = TsdfVolume((0.0, 0.0, 0.0), (n, n, n), 0.001, device=dev)
    ax = torch.arange(n, device=dev, dtype=torch.float32) - (n - 1) / 2
    d = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.39 * n
    vol.tsdf.copy_((d / 4).clamp_(-1, 1))
    vol.weight.fill_(1.0)
    rng = np.random.default_rng(0)
    o = torch.arange(-reach, reach + 1, device=dev, dtype=torch.float32)
    ball = ((torch.sqrt(o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) - radius) / 4).clamp_(-1, 1)
    placed = 0
    while placed < blobs:
        c = rng.integers(reach + 1, n - reach - 1, 3)
        if abs(np.linalg.norm(c - (n - 1) / 2) - 0.39 * n) < 3 * reach:      # clear of the shell (blobs may still meet each other)
            continue
        sl = tuple(slice(int(k) - reach, int(k) + reach + 1) for k in c)
        vol.tsdf[sl] = torch.minimum(vol.tsdf[sl], ball)
        placed += 1
    return vol


def timed(fn, wall=False):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = max(int(np.ceil(args.window / max((time.perf_counter() - t0) / 3, 1e-6))), 3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps if wall else e0.elapsed_time(e1) / reps


def measure(vol):
    nz, ny, nx = vol.dims
    counts = torch.empty((nz - 1, ny - 1, nx - 1), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().fp_tsdf_count_triangles(ops._ptr(vol.tsdf), ops._ptr(vol.weight), nz, ny, nx, 1.0, ops._ptr(counts), ops._stream(counts)),
               "fp_tsdf_count_triangles")
    labels, sizes = ops.tsdf_components(counts, vol.dims)
    comp = sizes[sizes > 0]
    runs = dict(label_ms=[], extract_ms=[], extract_keep_largest_ms=[])
    for _ in range(2):
        runs["label_ms"].append(timed(lambda: ops.tsdf_components(counts, vol.dims)))
        runs["extract_ms"].append(timed(lambda: ops.tsdf_extract(*vol.arrays(), vol.origin, vol.voxel), wall=True))
        runs["extract_keep_largest_ms"].append(timed(lambda: ops.tsdf_extract(*vol.arrays(), vol.origin, vol.voxel, keep="largest"), wall=True))
    out = dict(volume=f"{nx}x{ny}x{nz}", cubes=int(counts.numel()), active_cubes=int((counts > 0).sum()), triangles=int(counts.sum()),
               components=int(comp.numel()), largest=int(comp.max()) if comp.numel() else 0)
    out.update({k: min(v) for k, v in runs.items()})
    out["label_over_extract"] = out["label_ms"] / out["extract_ms"]
    out["runs"] = runs
    return out


with torch.inference_mode():
    res = {"metric": "ms per call through the Python wrappers: labelling the surface components (label_ms) next to the extraction they "
                     "filter (extract_ms: count, emit, unique) and the filtered extraction (extract_keep_largest_ms)",
           "lib": os.path.basename(_lib.LIB_PATH), "can": measure(can_volume()), "shell_and_blobs": measure(shell_and_blobs(args.big, args.blobs))}
print(json.dumps(res))
if args.out:
    kept = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            kept = json.load(f)
    kept[args.variant] = res
    with open(args.out, "w") as f:
        json.dump(kept, f, indent=1)
