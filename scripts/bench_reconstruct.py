"""Cost of the TSDF reconstruction on the device (fp_tsdf_integrate, ops.tsdf_extract) against the numpy restatement on the host.

16 views of the can (480 x 640, the device rasteriser's renders from all around at 0.5 m, true masks) into volumes of 128^3 and 256^3
voxels over the can's box:
  fuse      ops.tsdf_integrate of the 16 views into a fresh volume (the reset is not timed), HIP events around the call, warm, the
            median of --reps; the bytes the kernel must move at the least (the four volume arrays read and written once: 48 bytes a
            voxel; the views' pixels are gathers that mostly hit the caches) over the achievable HBM bandwidth as the floor;
  extract   ops.tsdf_extract (count -> cumsum -> the host read of the total -> emit -> torch.unique), HIP events around the whole
            call, and the two kernels alone through the C entry points;
  bake      ops.texture_bake of an atlas of --texels x --texels texels a face onto the extracted mesh from the same 16 views (tol = two
            voxels, min_cos 0.2; the outputs' allocation is inside the timed call), HIP events, warm, the median of --reps; the bytes
            it must write at the least (13 bytes a texel) over the achievable HBM bandwidth as the floor;
  host      tests/tsdf_model.py (float32 numpy, the same bits) on the same views: integrate and extract, once each (--host_dims), and
            tests/texture_bake_model.py for the bake.
Prints one JSON line; times in milliseconds.  --bake_out FILE puts the bake's figures under "bench" in that JSON file
(profiles/texture_bake.json), beside what the GPU test wrote there."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import tsdf_model as tm
from foundationpose_amd import _lib, ops, synthetic as syn
from foundationpose_amd.mesh import make_can_mesh
from foundationpose_amd.reconstruct import TsdfVolume
from foundationpose_amd.Utils import make_mesh_tensors

HBM_ACHIEVABLE = 6.3e12      # bytes / s (MI355X: 8 TB/s peak, about 6.3 TB/s measured for a streaming copy)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
ap.add_argument("--host_dims", type=int, nargs="*", default=[128], help="volume sizes the host restatement is timed at")
ap.add_argument("--texels", type=int, default=4, help="side of a face's block in the baked atlas")
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--bake_out", type=str, default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
V, H, W = 16, syn.H, syn.W
poses = syn.reference_view_poses(V, 0.5).astype(np.float32)
gm = make_mesh_tensors(make_can_mesh(), device=dev)
out = ops.render_crops(gm["_handle"], torch.as_tensor(poses, device=dev), None, syn.YCBV_K, H, W, (H, W), 0.2, normalize_xyz=False,
                       want=("color", "depth"))
depth = out["depth"].contiguous()
rgb = (out["color"].clamp(0, 1) * 255).contiguous()
masks = (depth > 0).to(torch.uint8).contiguous()
P = torch.as_tensor(poses, device=dev)
Ks = torch.as_tensor(np.tile(syn.YCBV_K[None], (V, 1, 1)), device=dev, dtype=torch.float64)
half = np.asarray([tm.CAN_RADIUS, tm.CAN_RADIUS, tm.CAN_HEIGHT / 2]) + 0.0075


def timed(fn, reps=args.reps, before=None):
    """median and minimum ms of fn() between HIP events, after 3 warm calls"""
    ts = []
    for i in range(reps + 3):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


res = {"views": V, "frame": [H, W], "volumes": {}}
for n in args.dims:
    s = float(2 * half.max() / (n - 1))
    vol = TsdfVolume(-half.max() * np.ones(3), (n, n, n), s, device=dev)
    arrays = vol.arrays()
    fuse = lambda: ops.tsdf_integrate(*arrays, depth, rgb, masks, P, Ks, vol.origin, vol.voxel, vol.trunc, vol.min_depth)   # noqa: E731
    t_fuse = timed(fuse, before=vol.reset)
    vol.reset()
    fuse()
    t_extract = timed(lambda: ops.tsdf_extract(*arrays, vol.origin, vol.voxel, 1.0), reps=max(5, args.reps // 2))
    mesh = ops.tsdf_extract(*arrays, vol.origin, vol.voxel, 1.0)
    T = int(mesh["faces"].shape[0])
    ncubes = (n - 1) ** 3
    counts = torch.empty(ncubes, dtype=torch.int32, device=dev)
    L, st, p = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream), (lambda t: C.c_void_p(t.data_ptr()))
    t_count = timed(lambda: L.fp_tsdf_count_triangles(p(arrays[0]), p(arrays[1]), n, n, n, 1.0, p(counts), st))
    offsets = (torch.cumsum(counts, 0, dtype=torch.int64) - counts).contiguous()
    keys = torch.empty(3 * T, dtype=torch.int64, device=dev)
    o32 = np.ascontiguousarray(vol.origin, np.float32)
    rows = [torch.empty((3 * T, 3), dtype=torch.float32, device=dev) for _ in range(3)]
    t_emit = timed(lambda: L.fp_tsdf_emit_triangles(p(arrays[0]), p(arrays[1]), p(arrays[2]), p(arrays[3]), n, n, n, o32.ctypes.data_as(C.c_void_p),
                                                    vol.voxel, 1.0, p(offsets), T, p(keys), p(rows[0]), p(rows[1]), p(rows[2]), st))
    floor = n ** 3 * 48 / HBM_ACHIEVABLE * 1e3
    r = dict(voxel_mm=s * 1e3, fuse_ms=t_fuse[0], fuse_min_ms=t_fuse[1], fuse_floor_ms=floor, extract_ms=t_extract[0], extract_min_ms=t_extract[1],
             count_kernel_ms=t_count[0], emit_kernel_ms=t_emit[0], vertices=int(mesh["pos"].shape[0]), faces=T)
    vcol = mesh["vertex_color"].add(0.5).floor_().clamp_(0, 255)
    bake = lambda: ops.texture_bake(mesh["pos"], mesh["faces"], vcol, depth, rgb, masks, P, Ks, 2 * s, 0.2, args.texels)   # noqa: E731
    t_bake = timed(bake)
    tex, cov, _, _ = bake()
    real = T * args.texels ** 2                        # texels of the faces' blocks; the rest of the last block row is padding
    r.update(bake_ms=t_bake[0], bake_min_ms=t_bake[1], bake_floor_ms=tex.shape[0] * tex.shape[1] * 13 / HBM_ACHIEVABLE * 1e3,
             atlas=[int(tex.shape[0]), int(tex.shape[1])], texels=args.texels,
             fallback_share=(int((cov == 0).sum()) - (tex.shape[0] * tex.shape[1] - real)) / max(real, 1))
    if n in args.host_dims:
        ref = tm.Volume((n, n, n), vol.origin, vol.voxel, vol.trunc)
        d_h, c_h, m_h = depth.cpu().numpy(), rgb.cpu().numpy(), masks.cpu().numpy()
        t0 = time.perf_counter()
        tm.integrate(ref, d_h, c_h, m_h, poses, Ks.cpu().numpy(), vol.min_depth)
        t1 = time.perf_counter()
        hp, hc, hn, hf = tm.extract(ref)
        t2 = time.perf_counter()
        same = bool(np.array_equal(hp.view(np.uint32), mesh["pos"].cpu().numpy().view(np.uint32)) and np.array_equal(hf, mesh["faces"].cpu().numpy()))
        r.update(host_fuse_ms=(t1 - t0) * 1e3, host_extract_ms=(t2 - t1) * 1e3, host_mesh_bit_equal=same)
        import texture_bake_model as tb
        t3 = time.perf_counter()
        h_tex, h_cov = tb.bake(mesh["pos"].cpu().numpy(), mesh["faces"].cpu().numpy(), vcol.cpu().numpy(), d_h, c_h, m_h, poses, Ks.cpu().numpy(),
                               args.texels, tb.default_bx(T), 2 * s, 0.2)
        r.update(host_bake_ms=(time.perf_counter() - t3) * 1e3,
                 host_atlas_bit_equal=bool(np.array_equal(h_tex.view(np.uint32), tex.cpu().numpy().view(np.uint32)) and np.array_equal(h_cov, cov.cpu().numpy())))
    res["volumes"][str(n)] = r
    del vol, arrays, mesh, counts, offsets, keys, rows, tex, cov, vcol
    torch.cuda.empty_cache()
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
if args.bake_out:
    doc = json.load(open(args.bake_out)) if os.path.exists(args.bake_out) else {}
    keys = ("voxel_mm", "faces", "atlas", "texels", "bake_ms", "bake_min_ms", "bake_floor_ms", "fuse_ms", "extract_ms", "fallback_share",
            "host_bake_ms", "host_atlas_bit_equal")
    doc["bench"] = {"views": V, "frame": [H, W], "volumes": {n: {k: r[k] for k in keys if k in r} for n, r in res["volumes"].items()}}
    with open(args.bake_out, "w") as f:
        json.dump(doc, f, indent=1)
