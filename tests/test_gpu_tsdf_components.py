"""GPU: fp_tsdf_label_components and the layers above it (ops.tsdf_components, ops.tsdf_extract(keep=...), TsdfVolume.extract /
components, reconstruct_object(keep_components=...), FoundationPose.from_reference_views, scripts/run_demo.py --ref_keep_components)
against the numpy restatement (tests/tsdf_components_model.py): labels and sizes element for element on generated counts arrays,
what the kernels may write, repeated calls, graph replay, another stream, and the can with a floater written into its volume.  Each
test prints its figures before it asserts."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import tsdf_components_model as cm
import tsdf_model as tm
from test_gpu_multi_object import dev  # noqa: F401
from test_gpu_tsdf import Arena, _noisy_reference_views, _same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = cm.generated_cases()


@functools.lru_cache(maxsize=None)
def _reference(i):
    name, dims, counts = CASES[i]
    return cm.label(counts, dims)


def _label_c(counts, dims, labels, sizes):
    from foundationpose_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr() if t.numel() else 0)     # noqa: E731
    st = _lib.lib().fp_tsdf_label_components(p(counts), *dims, p(labels), p(sizes), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st, "fp_tsdf_label_components")


# ------------------------------------------------------------------ 1. labels and sizes against the restatement
def test_labels_and_sizes_equal_the_restatement_and_nothing_else_is_written(dev):
    """every generated case through the C entry point, into poisoned arrays with guards on both sides, twice"""
    components = 0
    for i, (name, dims, counts) in enumerate(CASES):
        ref_labels, ref_sizes = _reference(i)
        arena = Arena(dev)
        n = counts.size
        c = arena.new((n,), torch.int32)
        c.copy_(torch.as_tensor(counts))
        labels, sizes = arena.new((n,), torch.int32), arena.new((n,), torch.int32)
        _label_c(c, dims, labels, sizes)
        torch.cuda.synchronize()
        first = labels.cpu().numpy(), sizes.cpu().numpy()
        _same_bits(first[0], ref_labels, f"{name}: labels")
        _same_bits(first[1], ref_sizes, f"{name}: sizes")
        _same_bits(c.cpu().numpy(), counts, f"{name}: counts are read only")
        _label_c(c, dims, labels, sizes)                          # over its own output: the kernels write every element themselves
        torch.cuda.synchronize()
        _same_bits(labels.cpu().numpy(), first[0], f"{name}: labels of a second call")
        _same_bits(sizes.cpu().numpy(), first[1], f"{name}: sizes of a second call")
        arena.check()
        components += int((ref_sizes > 0).sum())
    print(f"{len(CASES)} cases, {components} components")
    assert components > 1000


def test_a_volume_without_cubes_writes_nothing(dev):
    from foundationpose_amd import ops
    arena = Arena(dev)
    labels, sizes, counts = (arena.new((16,), torch.int32) for _ in range(3))
    before = [t.clone() for t in (labels, sizes, counts)]
    for dims in ((5, 1, 7), (1, 1, 1), (1, 4096, 4096)):
        _label_c(counts, dims, labels, sizes)
    torch.cuda.synchronize()
    arena.check()
    assert all(torch.equal(a, b) for a, b in zip((labels, sizes, counts), before))
    l, s = ops.tsdf_components(torch.empty((0,), dtype=torch.int32, device=dev), (5, 1, 7))
    assert tuple(l.shape) == tuple(s.shape) == (4, 0, 6) and l.dtype == s.dtype == torch.int32


def _case_named(name):
    i = next(k for k, c in enumerate(CASES) if c[0] == name)
    return CASES[i][1], CASES[i][2], _reference(i)


def test_the_wrapper_on_another_stream_and_a_graph_replayed_three_times(dev):
    from foundationpose_amd import ops
    dims, counts, (ref_labels, ref_sizes) = _case_named("33x20x9 density 0.3")
    c = torch.as_tensor(counts, device=dev)
    shape = cm.cube_shape(dims)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        labels, sizes = ops.tsdf_components(c.reshape(shape), dims)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert tuple(labels.shape) == tuple(sizes.shape) == shape
    _same_bits(labels.cpu().numpy().reshape(-1), ref_labels, "labels on a side stream")
    _same_bits(sizes.cpu().numpy().reshape(-1), ref_sizes, "sizes on a side stream")
    # the long chain, captured: the three launches replay without a host call between them
    dims, counts, (ref_labels, ref_sizes) = _case_named("serpentine")
    c = torch.as_tensor(counts, device=dev)
    out_l, out_s = (torch.empty((counts.size,), dtype=torch.int32, device=dev) for _ in range(2))
    with torch.inference_mode():                                  # captured as the package captures (see test_gpu_tsdf.py)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _label_c(c, dims, out_l, out_s)
        for k in range(3):
            out_l.fill_(-77)
            out_s.fill_(-77)
            graph.replay()
            torch.cuda.synchronize()
            _same_bits(out_l.cpu().numpy(), ref_labels, f"labels of replay {k}")
            _same_bits(out_s.cpu().numpy(), ref_sizes, f"sizes of replay {k}")


# ------------------------------------------------------------------ 2. end to end: the can with a floater
@pytest.fixture(scope="module")
def noisy_views(scene, dev):
    """the can's 16 noisy device renders with their true masks, as test_gpu_tsdf.py builds them"""
    return _noisy_reference_views(scene, dev)


def test_the_can_with_a_ball_keeps_the_can(noisy_views, dev):
    from foundationpose_amd.reconstruct import TsdfVolume
    v = noisy_views
    origin, dims, s, trunc = tm.can_volume_spec()
    vol = TsdfVolume(origin, dims, float(s), float(trunc), device=dev)
    vol.integrate(v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"])
    at, dist = cm.ball_footprint(dims)
    vol.tsdf.reshape(-1)[torch.as_tensor(at, device=dev)] = torch.as_tensor(cm.ball_values(dist), device=dev)
    # the device's own arrays, through the restatement
    ref = tm.Volume(dims, origin, s, trunc)
    ref.tsdf, ref.weight, ref.color, ref.color_weight = (t.cpu().numpy().reshape(a.shape) for t, a in zip(vol.arrays(), ref.arrays().values()))
    assert (ref.weight[at] >= 1).all()
    want = cm.extract_kept(ref, "largest")
    mesh, tensors = vol.extract(keep="largest")
    print(f"can + ball on the device: components {mesh.components}, {mesh.dropped_triangles} triangles dropped, {len(mesh.faces)} kept")
    _same_bits(tensors["pos"].cpu().numpy(), want["pos"], "kept positions")
    _same_bits(tensors["vnormals"].cpu().numpy(), want["nrm"], "kept normals")
    assert tensors["faces"].dtype == torch.int32 and np.array_equal(tensors["faces"].cpu().numpy().astype(np.int64), want["faces"])
    assert mesh.components == want["components"] and mesh.dropped_triangles == want["dropped_triangles"] > 100
    assert len(mesh.components) == 2 and tm.edge_report(mesh.faces)[0] == 0 and tm.edge_report(mesh.faces)[2] == 2
    assert tm.cylinder_distance(mesh.vertices, tm.CAN_RADIUS, tm.CAN_HEIGHT).max() <= float(s)
    # the report without extracting
    rep = vol.components()
    assert rep["components"] == want["components"]
    _same_bits(rep["labels"].cpu().numpy().reshape(-1), want["labels"], "TsdfVolume.components: labels")
    # keep=n: both components up to the ball's size, the can alone from one above it; too many: refused, naming the largest
    ball, can = min(mesh.components), max(mesh.components)
    m_all, t_all = vol.extract(keep=ball)
    m_can, t_can = vol.extract(keep=ball + 1)
    assert m_all.dropped_triangles == 0 and len(m_all.faces) == ball + can
    assert torch.equal(t_can["pos"], tensors["pos"]) and torch.equal(t_can["faces"], tensors["faces"])
    with pytest.raises(ValueError, match=str(can)):
        vol.extract(keep=can + 1)
    # keep=None is the call as it was: the same bits, no report
    m0, t0 = vol.extract()
    m1, t1 = vol.extract(keep=None)
    for k in ("pos", "vnormals", "vertex_color", "faces"):
        assert torch.equal(t0[k], t1[k]) and torch.equal(t0[k], t_all[k]), k
    assert not hasattr(m0, "components") and tm.edge_report(m0.faces)[2] == 4
    assert tm.cylinder_distance(m0.vertices, tm.CAN_RADIUS, tm.CAN_HEIGHT).max() > 0.010


def test_from_reference_views_without_a_floater_gives_the_same_mesh(scene, noisy_views, dev):
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.reconstruct import reconstruct_object
    from test_gpu_pose_errors import _estimator
    v = noisy_views
    true_est = _estimator(scene["mesh"], dev)
    args = (v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"])
    kw = dict(voxel=tm.CAN_VOXEL, scorer=true_est.scorer, refiner=true_est.refiner, device=dev)
    plain = FoundationPose.from_reference_views(*args, **kw)
    kept = FoundationPose.from_reference_views(*args, reconstruct_args={"keep_components": "largest"}, **kw)
    for k in ("pos", "vnormals", "vertex_color", "faces"):
        assert torch.equal(plain.mesh_tensors[k], kept.mesh_tensors[k]), k
    assert np.array_equal(plain.mesh.faces, kept.mesh.faces) and np.array_equal(plain.mesh.vertices, kept.mesh.vertices)
    # the report, and the refine_poses rounds and the texture bake with the filter in place
    mesh, _ = reconstruct_object(*args, voxel=tm.CAN_VOXEL, device=dev, keep_components=1000, refine_poses=1, refine_iterations=1, texture=2)
    print(f"reconstruct_object(keep_components=1000): components {mesh.components}, dropped {mesh.dropped_triangles}")
    assert sum(n for n in mesh.components if n >= 1000) == len(mesh.faces) > 80000
    assert sum(mesh.components) - mesh.dropped_triangles == len(mesh.faces) and mesh.ob_in_cams.shape == (16, 4, 4)
    # more triangles than any component has: the refusal names the largest (here the whole mesh: 'largest' dropped nothing above)
    with pytest.raises(ValueError, match=f"keep=10000000 triangles, the largest of the 1 components has {len(plain.mesh.faces)}"):
        reconstruct_object(*args, voxel=tm.CAN_VOXEL, device=dev, keep_components=10_000_000)


def test_run_demo_with_the_keep_flag(tmp_path, dev):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_demo", os.path.join(root, "scripts", "run_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from foundationpose_amd.mesh_io import load_ply
    ply = str(tmp_path / "can.ply")
    times = mod.main(["--synthetic_ref_views", "16", "--synthetic", "2", "--standin_weights", "--ref_keep_components", "largest",
                      "--save_mesh", ply, "--debug_dir", str(tmp_path / "d")])
    assert len(times) == 2
    mesh = load_ply(ply)
    assert len(mesh.faces) > 10000 and int(mesh.faces.max()) == len(mesh.vertices) - 1
