"""GPU: fp_tsdf_integrate / fp_tsdf_count_triangles / fp_tsdf_emit_triangles and the layers above them (ops.tsdf_integrate /
tsdf_extract, reconstruct.py, FoundationPose.from_reference_views, scripts/run_demo.py --ref_views) against the numpy restatement of
their definition (tests/tsdf_model.py): the four volume arrays, the triangle counts, every emitted corner and the welded mesh bit-equal;
what the kernels may write; streaming and graph replay; and the can rebuilt from 16 noisy views, registered with.  Each test prints its
figures before it asserts; profiles/tsdf_reconstruct.json holds those of a run on an MI355X."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import tsdf_model as tm
from test_gpu_multi_object import dev  # noqa: F401
from test_tsdf_host import CASE_DIMS, CASE_VIEWS, can_model_volume, can_views  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 0x7149F2CA                                                 # the guard elements' bit pattern (1e30 as a float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.argwhere(_bits(got) != _bits(ref))
    assert len(bad) == 0, (what, len(bad), "first at", bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


class Arena:
    """device arrays carved out of one poisoned buffer with 64 guard elements on each side"""

    def __init__(self, dev):
        self.dev, self.blocks = dev, []

    def new(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        buf = torch.empty(n + 128, dtype=dtype, device=self.dev)
        self._raw(buf).fill_(GUARD if dtype.itemsize > 1 else 0xCA)
        t = buf[64:64 + n].view(shape)
        if fill is not None:
            t.fill_(fill)
        self.blocks.append((buf, n))
        return t

    @staticmethod
    def _raw(buf):
        return buf.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[buf.dtype.itemsize])

    def check(self):
        for buf, n in self.blocks:
            raw, want = self._raw(buf), GUARD if buf.dtype.itemsize > 1 else 0xCA
            assert bool((raw[:64] == want).all()) and bool((raw[64 + n:] == want).all()), "a guard was written"


def _fresh(dev, dims, arena=None):
    new = arena.new if arena is not None else (lambda shape, dtype, fill=None: torch.full(shape, fill, dtype=dtype, device=dev))
    return [new(tuple(dims), torch.float32, 1.0), new(tuple(dims), torch.float32, 0.0), new(tuple(dims) + (3,), torch.float32, 0.0),
            new(tuple(dims), torch.float32, 0.0)]


def _upload(dev, case, views=slice(None)):
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a[views]), device=dev)     # noqa: E731
    return dict(depth=t(case["depth"]), rgb=t(case["rgb"]), masks=t(case["masks"]), ob_in_cams=t(case["ob_in_cams"]),
                Ks=torch.as_tensor(np.ascontiguousarray(case["Ks"][views]), device=dev, dtype=torch.float64))


def _integrate(vol, up, case):
    from foundationpose_amd import ops
    ops.tsdf_integrate(*vol, up["depth"], up["rgb"], up["masks"], up["ob_in_cams"], up["Ks"], case["origin"], float(case["voxel"]),
                       float(case["trunc"]), float(case["min_depth"]))


def _compare_volume(vol, ref, what):
    torch.cuda.synchronize()
    for t, (name, a) in zip(vol, ref.arrays().items()):
        got = t.cpu().numpy().reshape(a.shape)
        assert not np.isnan(got).any(), (what, name, "NaN")
        _same_bits(got, a, f"{what}: {name}")


def _count_c(dev, vol, dims, min_weight, counts):
    from foundationpose_amd import _lib
    st = _lib.lib().fp_tsdf_count_triangles(C.c_void_p(vol[0].data_ptr()), C.c_void_p(vol[1].data_ptr()), *dims, float(min_weight),
                                            C.c_void_p(counts.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st, "fp_tsdf_count_triangles")


def _emit_c(dev, vol, dims, origin, voxel, min_weight, offsets, total, arena=None):
    """fp_tsdf_emit_triangles through the C entry point -> keys (3T,) int64, pos / col / nrm (3T,3) float32"""
    from foundationpose_amd import _lib
    new = arena.new if arena is not None else (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev))
    keys = new((3 * total,), torch.int64)
    pos, col, nrm = (new((3 * total, 3), torch.float32) for _ in range(3))
    o = np.ascontiguousarray(origin, f32)
    p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
    st = _lib.lib().fp_tsdf_emit_triangles(p(vol[0]), p(vol[1]), p(vol[2]), p(vol[3]), *dims, o.ctypes.data_as(C.c_void_p), float(voxel),
                                           float(min_weight), p(offsets), total, p(keys), p(pos), p(col), p(nrm),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st, "fp_tsdf_emit_triangles")
    torch.cuda.synchronize()
    return keys, pos, col, nrm


def _compare_extraction(dev, vol, ref, origin, voxel, what, min_weight=1.0):
    """counts, emitted corners and the welded mesh of the device volume `vol` against the restatement on `ref`"""
    from foundationpose_amd import ops
    dims = ref.dims
    ncubes = max(dims[0] - 1, 0) * max(dims[1] - 1, 0) * max(dims[2] - 1, 0)
    ref_counts = tm.count_triangles(ref, min_weight)
    if ncubes:
        counts = torch.full((ncubes,), -7, dtype=torch.int32, device=dev)
        _count_c(dev, vol, dims, min_weight, counts)
        _same_bits(counts.cpu().numpy(), ref_counts, f"{what}: counts")
    keys, pos, col, nrm = tm.emit_triangles(ref, min_weight)
    out = ops.tsdf_extract(*vol, origin, float(voxel), min_weight)
    T = int(ref_counts.sum())
    print(f"{what}: {T} triangles, {len(np.unique(keys))} vertices")
    assert int(out["faces"].shape[0]) == T
    assert sorted(out) == ["faces", "pos", "vertex_color", "vnormals"]
    if T == 0:
        assert int(out["pos"].shape[0]) == 0
        return out
    offsets = (torch.cumsum(counts, 0, dtype=torch.int64) - counts).contiguous()      # the counts were compared above
    ck, cp, cc, cn = (t.cpu().numpy() for t in _emit_c(dev, vol, dims, origin, voxel, min_weight, offsets, T))
    _same_bits(ck, keys, f"{what}: keys")
    _same_bits(cp, pos, f"{what}: corner positions")
    _same_bits(cc, col, f"{what}: corner colours")
    _same_bits(cn, nrm, f"{what}: corner normals")
    wp, wc, wn, wf = tm.weld(keys, pos, col, nrm)
    _same_bits(out["pos"].cpu().numpy(), wp, f"{what}: welded positions")
    _same_bits(out["vertex_color"].cpu().numpy(), wc, f"{what}: welded colours")
    _same_bits(out["vnormals"].cpu().numpy(), wn, f"{what}: welded normals")
    assert out["faces"].dtype == torch.int32 and np.array_equal(out["faces"].cpu().numpy().astype(np.int64), wf)
    assert not np.isnan(cp).any() and not np.isnan(cn).any()
    return out


# ------------------------------------------------------------------ 1. volumes, counts, corners and meshes against the restatement
@functools.lru_cache(maxsize=None)
def _case(di, vi):
    dims, (V, H, W, kv) = CASE_DIMS[di], CASE_VIEWS[vi]
    case = tm.generated_case(dims, V, H, W, kv, seed=V + H + dims[2], with_masks=(V + dims[0]) % 2 == 1)
    return case, tm.fuse_case(case)


@pytest.mark.parametrize("vi", range(len(CASE_VIEWS)), ids=[f"V{v[0]}-{v[1]}x{v[2]}-K{v[3]}" for v in CASE_VIEWS])
@pytest.mark.parametrize("di", range(len(CASE_DIMS)), ids=["x".join(str(n) for n in d) for d in CASE_DIMS])
def test_volume_counts_and_mesh_equal_the_restatement(dev, di, vi):
    case, ref = _case(di, vi)
    arena = Arena(dev)
    vol = _fresh(dev, case["dims"], arena)
    _integrate(vol, _upload(dev, case), case)
    _compare_volume(vol, ref, "fused")
    arena.check()
    _compare_extraction(dev, vol, ref, case["origin"], case["voxel"], "generated", min_weight=1.0)
    _compare_extraction(dev, vol, ref, case["origin"], case["voxel"], "generated, min_weight 2", min_weight=2.0)


def test_the_can_volume_and_mesh_equal_the_restatement(dev, can_views, can_model_volume):
    """48 x 48 x 64 voxels, 16 views of 480 x 640, ~83 k faces: the prefix sum crosses hundreds of workgroups"""
    origin, dims, s, trunc = tm.can_volume_spec()
    case = dict(can_views, dims=dims, origin=origin, voxel=s, trunc=trunc, min_depth=f32(0.001))
    vol = _fresh(dev, dims)
    _integrate(vol, _upload(dev, case), case)
    _compare_volume(vol, can_model_volume, "can")
    out = _compare_extraction(dev, vol, can_model_volume, origin, s, "can")
    faces = out["faces"].cpu().numpy()
    assert len(faces) > 80000 and tm.edge_report(faces)[0] == 0 and tm.edge_report(faces)[2] == 2


def test_one_surface_tetrahedron_and_no_surface(dev):
    from foundationpose_amd import ops
    origin, s = np.zeros(3, f32), f32(0.01)
    ref = tm.Volume((2, 2, 2), origin, s, 4 * s)
    corners = tm.tet_corners(tm.PERMS[3])                      # axes (1, 2, 0): the only tetrahedron whose four corners were observed
    lin = corners[:, 2] * 4 + corners[:, 1] * 2 + corners[:, 0]
    ref.weight[lin] = 1
    ref.tsdf[:] = 0.5
    ref.tsdf[lin[2]] = -0.25
    ref.color[:] = np.arange(24, dtype=f32).reshape(8, 3)
    ref.color_weight[lin[:3]] = 1
    vol = [torch.as_tensor(a.reshape(sh), device=dev) for a, sh in zip(ref.arrays().values(), [(2, 2, 2), (2, 2, 2), (2, 2, 2, 3), (2, 2, 2)])]
    out = _compare_extraction(dev, vol, ref, origin, s, "one tetrahedron")
    assert int(out["faces"].shape[0]) == 1 and int(out["pos"].shape[0]) == 3
    ref.tsdf[:] = 1                                            # nothing inside: no surface
    vol[0].fill_(1.0)
    out = _compare_extraction(dev, vol, ref, origin, s, "no surface")
    assert int(out["faces"].shape[0]) == 0
    flat = [torch.ones((1, 4, 4), device=dev), torch.ones((1, 4, 4), device=dev), torch.zeros((1, 4, 4, 3), device=dev), torch.zeros((1, 4, 4), device=dev)]
    assert int(ops.tsdf_extract(*flat, origin, s)["faces"].shape[0]) == 0          # a volume of one layer has no cubes


# ------------------------------------------------------------------ 2. what is written, streaming, replay
def test_count_and_emit_write_nothing_outside_their_outputs(dev):
    case, ref = _case(1, 3)
    vol = [torch.as_tensor(a, device=dev) for a in ref.arrays().values()]
    dims = ref.dims
    ncubes = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    arena = Arena(dev)
    counts = arena.new((ncubes,), torch.int32)
    _count_c(dev, vol, dims, 1.0, counts)
    ref_counts = tm.count_triangles(ref)
    _same_bits(counts.cpu().numpy(), ref_counts, "counts")
    T = int(ref_counts.sum())
    assert T > 100
    offsets = torch.as_tensor(np.cumsum(ref_counts.astype(np.int64)) - ref_counts, device=dev)
    keys, pos, col, nrm = _emit_c(dev, vol, dims, case["origin"], case["voxel"], 1.0, offsets, T, arena)
    arena.check()
    rk, rp, rc, rn = tm.emit_triangles(ref)
    _same_bits(keys.cpu().numpy(), rk, "keys")
    _same_bits(pos.cpu().numpy(), rp, "pos")
    _same_bits(col.cpu().numpy(), rc, "col")
    _same_bits(nrm.cpu().numpy(), rn, "nrm")


def test_two_calls_are_one_call_and_a_graph_replays_the_eager_bits(dev):
    case, ref = _case(1, 2)                                   # 17 x 9 x 33, 16 views
    up = _upload(dev, case)
    vol = _fresh(dev, case["dims"])
    for sl in (slice(0, 5), slice(5, 16)):
        _integrate(vol, _upload(dev, case, sl), case)
    _compare_volume(vol, ref, "two calls")
    eager = [t.clone() for t in vol]

    def reset():
        vol[0].fill_(1.0)
        for t in vol[1:]:
            t.zero_()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        reset()
        _integrate(vol, up, case)                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    # captured as the package captures (graphs.py, engine.py): under inference_mode.  The capture updates the default generator's
    # graph state in place, and that state is an inference tensor once an earlier capture of the process was made there
    with torch.inference_mode():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _integrate(vol, up, case)
        for _ in range(2):
            reset()
            graph.replay()
            torch.cuda.synchronize()
            for t, e in zip(vol, eager):
                assert torch.equal(t.view(torch.int32), e.view(torch.int32))
    _compare_volume(vol, ref, "replayed")


# ------------------------------------------------------------------ 3. end to end
def _noisy_reference_views(scene, dev, n=16):
    """the can rendered by the device rasteriser at the reference poses, each frame composed like synthetic.compose_frame (background
    plane, 1 mm noise, 2 % dropout) with its true mask"""
    from foundationpose_amd import ops, synthetic as syn
    from foundationpose_amd.Utils import make_mesh_tensors
    poses = tm.can_view_poses(n, 0.5).astype(f32)
    gm = make_mesh_tensors(scene["mesh"], device=dev)
    out = ops.render_crops(gm["_handle"], torch.as_tensor(poses, device=dev), None, scene["K"], scene["H"], scene["W"], (scene["H"], scene["W"]),
                           scene["diameter"], normalize_xyz=False, want=("color", "depth"))
    color, depth = out["color"].cpu().numpy(), out["depth"].cpu().numpy()
    frames = [syn.compose_frame(color[i], depth[i], seed=50 + i) for i in range(n)]
    return dict(rgb=np.stack([f[0] for f in frames]), depth=np.stack([f[1] for f in frames]),
                masks=np.stack([f[2] for f in frames]).astype(np.uint8), ob_in_cams=poses, Ks=np.tile(scene["K"][None], (n, 1, 1)))


def test_the_can_from_noisy_views_and_registration_with_it(scene, dev):
    """The bounds: every vertex within one voxel edge (2.5 mm) of the cylinder, on the device and in the restatement alike (their
    meshes are bit-equal); ADD-S of the registration with the reconstructed model at most one voxel edge above that with the true
    mesh, both with the stand-in networks.  FP_TSDF_PROFILE_OUT=<file> writes the figures of a run (profiles/tsdf_reconstruct.json)."""
    from foundationpose_amd import ops
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.reconstruct import reconstruct_object
    from test_gpu_pose_errors import _estimator
    v = _noisy_reference_views(scene, dev)
    mesh, tensors = reconstruct_object(v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"], voxel=tm.CAN_VOXEL, device=dev)
    bad, edges, euler = tm.edge_report(mesh.faces)
    d = tm.cylinder_distance(mesh.vertices, tm.CAN_RADIUS, tm.CAN_HEIGHT) * 1e3
    print(f"can from 16 noisy views: {len(mesh.vertices)} vertices / {len(mesh.faces)} faces, {bad} bad of {edges} edges, Euler {euler}, "
          f"distance to the cylinder median {np.median(d):.3f} p99 {np.percentile(d, 99):.3f} max {d.max():.3f} mm")
    assert mesh.visual.vertex_colors.dtype == np.uint8 and tensors["pos"].is_cuda and tensors["faces"].dtype == torch.int32
    # the restatement on the same inputs and the same volume: the reference itself stays inside the bound, and the device equals it
    from foundationpose_amd.reconstruct import PAD_VOXELS, bounds_from_views
    blo, bhi = bounds_from_views(v["depth"], v["masks"], v["ob_in_cams"], v["Ks"], 0.0, 0.001, dev)
    blo, bhi = blo - PAD_VOXELS * tm.CAN_VOXEL, bhi + PAD_VOXELS * tm.CAN_VOXEL
    nx, ny, nz = (int(np.ceil(e / tm.CAN_VOXEL - 1e-9)) + 1 for e in (bhi - blo))
    ref = tm.Volume((nz, ny, nx), blo, tm.CAN_VOXEL, 4.0 * tm.CAN_VOXEL)
    tm.integrate(ref, v["depth"], v["rgb"].astype(f32), v["masks"], v["ob_in_cams"], v["Ks"])
    rp, rc, rn, rf = tm.extract(ref)
    rd = tm.cylinder_distance(rp, tm.CAN_RADIUS, tm.CAN_HEIGHT) * 1e3
    print(f"the restatement on the same views: {len(rp)} vertices, max {rd.max():.3f} mm")
    assert rd.max() <= 2.5 and tm.edge_report(rf)[0] == 0
    _same_bits(np.asarray(mesh.vertices, f32), rp, "reconstruct_object against the restatement")
    assert np.array_equal(mesh.faces, rf)
    assert bad == 0 and euler == 2 and tm.repeated_vertex_faces(mesh.faces) == 0
    assert d.max() <= 2.5
    # registration with the reconstructed model against registration with the true textured mesh
    true_est = _estimator(scene["mesh"], dev)
    rec_est = FoundationPose.from_reference_views(v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"], voxel=tm.CAN_VOXEL,
                                                  scorer=true_est.scorer, refiner=true_est.refiner, device=dev)
    assert len(rec_est.mesh.faces) == len(mesh.faces)
    # the estimator took the reconstruction's device tensors, centred: the bits an upload of its centred mesh gives
    from foundationpose_amd.Utils import make_mesh_tensors
    up = make_mesh_tensors(rec_est.mesh, device=dev)
    for k in ("pos", "vnormals", "vertex_color", "faces"):
        assert rec_est.mesh_tensors[k].dtype == up[k].dtype and torch.equal(rec_est.mesh_tensors[k], up[k]), k
    pts = torch.as_tensor(np.asarray(scene["mesh"].vertices, f32), device=dev)
    gt = torch.as_tensor(np.asarray(scene["gt"], np.float64)[None], device=dev)
    errs = {}
    for name, est in (("true mesh", true_est), ("reconstructed", rec_est)):
        pose = est.register(scene["K"], scene["rgb"], scene["depth"], scene["mask"], iteration=5)
        table = ops.pose_errors(pts, torch.as_tensor(np.asarray(pose, f32)[None], device=dev), gt, want=("add", "adds"))
        errs[name] = float(ops.PoseErrors.rows(table)[0].adds)
    print(f"ADD-S of the registration: true mesh {errs['true mesh'] * 1e3:.3f} mm, reconstructed {errs['reconstructed'] * 1e3:.3f} mm "
          f"(gate: at most {tm.CAN_VOXEL * 1e3} mm more)")
    path = os.environ.get("FP_TSDF_PROFILE_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(noisy_views=dict(vertices=len(mesh.vertices), faces=len(mesh.faces), median_mm=float(np.median(d)),
                                            p99_mm=float(np.percentile(d, 99)), max_mm=float(d.max())),
                           adds_true_mesh_m=errs["true mesh"], adds_reconstructed_m=errs["reconstructed"]), f, indent=1)
    assert errs["reconstructed"] <= errs["true mesh"] + tm.CAN_VOXEL


def test_refusals_that_need_the_device(scene, dev):
    from foundationpose_amd.reconstruct import reconstruct_object
    d = np.full((2, 24, 32), 0.5, f32)
    rgb, poses = np.zeros((2, 24, 32, 3), np.uint8), np.tile(np.eye(4, dtype=f32), (2, 1, 1))
    K = np.array([[40.0, 0, 16], [0, 40, 12], [0, 0, 1]])
    with pytest.raises(ValueError, match="masks are empty"):
        reconstruct_object(rgb, d, np.zeros((2, 24, 32), np.uint8), poses, K, device=dev)
    # observed, but no tetrahedron whose four corners were observed five times by two views: no surface
    with pytest.raises(ValueError, match="no surface"):
        reconstruct_object(rgb, d, np.ones((2, 24, 32), np.uint8), poses, K, voxel=0.01, min_weight=5, device=dev)


def test_run_demo_with_synthetic_reference_views(tmp_path, dev):
    import importlib.util
    from foundationpose_amd.mesh_io import load_ply
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_demo", os.path.join(root, "scripts", "run_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ply = str(tmp_path / "can.ply")
    times = mod.main(["--synthetic_ref_views", "16", "--synthetic", "3", "--standin_weights", "--save_mesh", ply, "--debug_dir", str(tmp_path / "d")])
    assert len(times) == 3
    mesh = load_ply(ply)
    assert len(mesh.faces) > 10000 and int(mesh.faces.max()) == len(mesh.vertices) - 1
    assert mesh.visual.vertex_colors is not None and len(mesh.visual.vertex_colors) == len(mesh.vertices)
    # at the default pitch (128 voxels on the longest side, 1.2 mm) under frames quantised to millimetres with 2 % dropout, a few
    # voxels next to the surface stay unobserved and leave holes: reported, not gated (the gates are at 2.5 mm, above)
    d = tm.cylinder_distance(mesh.vertices, tm.CAN_RADIUS, tm.CAN_HEIGHT)
    print(f"run_demo's mesh: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces, {tm.edge_report(mesh.faces)[0]} edges not shared by "
          f"exactly two faces, max {d.max() * 1e3:.2f} mm from the cylinder")
    for i in range(3):
        assert np.isfinite(np.loadtxt(tmp_path / "d" / "ob_in_cam" / f"{i:07d}.txt")).all()
