"""CPU: the definition of fp_tsdf_label_components (include/fp_amd.h) and of the kept-mesh filter of ops.tsdf_extract(keep=...)
through their numpy restatement (tests/tsdf_components_model.py), which the GPU tests then hold the kernels to element for element:
the partition against scipy.ndimage.label, every deliberately wrong variant told apart on a named case, the can alone and with a
floater written into its volume, and every refusal that needs no device.  Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_components_model as cm
import tsdf_model as tm
from test_tsdf_host import can_model_volume, can_views  # noqa: F401

f32 = np.float32
CASES = cm.generated_cases()


# ------------------------------------------------------------------ the labelling
def test_partition_is_scipys_and_every_label_is_the_smallest_index():
    from scipy import ndimage
    seen = 0
    for name, dims, counts in CASES:
        shape = cm.cube_shape(dims)
        sweeps = []
        labels, sizes = cm.label(counts, dims, sweeps=sweeps)
        assert labels.dtype == np.int32 and sizes.dtype == np.int32 and labels.shape == sizes.shape == counts.shape
        if counts.size == 0:
            continue
        ref, n = ndimage.label(counts.reshape(shape) > 0)                    # the default structure: faces
        assert cm.partition(labels) == cm.partition(np.where(ref > 0, ref, -1)), name
        parts = cm.partition(labels)
        assert len(parts) == n == int((sizes > 0).sum())
        for g in parts:
            g = np.asarray(g)
            assert (labels[g] == g[0]).all() and sizes[g[0]] == counts[g].sum() and (sizes[g[1:]] == 0).all(), name
        assert ((labels == -1) == (counts <= 0)).all() and (sizes[counts <= 0] == 0).all()
        print(f"{name}: {int((counts > 0).sum())} active of {counts.size} cubes, {n} components, {sweeps[0]} sweeps")
        seen += n
    assert seen > 1000


def test_the_serpentine_is_one_chain():
    name, dims, counts = next(c for c in CASES if c[0] == "serpentine")
    labels, sizes = cm.label(counts, dims)
    active = counts > 0
    # a chain: every cube has two active face neighbours, but its two ends
    a = active.reshape(cm.cube_shape(dims))
    nb = np.zeros(a.shape, int)
    for d in cm.FACES:
        s, t = cm._pairs(a.shape, d)
        both = a[s] & a[t]
        nb[s] += both
        nb[t] += both
    print(f"serpentine: {int(active.sum())} cubes in one chain of {a.size}")
    assert (labels[active] == 0).all() and sizes[0] == counts.sum() and active.sum() > 1200
    assert sorted(np.bincount(nb[a])[1:].tolist()) == [2, int(active.sum()) - 2]


def test_wrong_labellings_are_told_apart():
    for (dims, counts), other in ((cm.edge_contact_case(), 3), (cm.corner_contact_case(), 7)):
        labels, sizes = cm.label(counts, dims)
        assert np.nonzero(labels >= 0)[0].tolist() == [0, other] and labels[0] == 0 and labels[other] == other
        assert sizes[0] == 2 and sizes[other] == 5 and sizes.sum() == 7
        l26, s26 = cm.label(counts, dims, wrong="26")
        assert len(cm.partition(l26)) == 1 and s26[s26 > 0].tolist() == [7]
    name, dims, counts = cm.equal_sizes_case()
    labels, sizes = cm.label(counts, dims)
    assert labels.tolist() == [0, 0, -1, -1, -1, 5, -1] and sizes.tolist() == [7, 0, 0, 0, 0, 7, 0]
    lmax, smax = cm.label(counts, dims, wrong="max_label")
    assert lmax.tolist() == [1, 1, -1, -1, -1, 5, -1] and not np.array_equal(lmax, labels)
    lc, sc = cm.label(counts, dims, wrong="cube_sizes")
    assert np.array_equal(lc, labels) and sc.tolist() == [2, 0, 0, 0, 0, 1, 0]
    # a tie for the largest goes to the smaller label
    assert cm.choose(labels, sizes, "largest")[0].tolist() == [0]
    assert cm.choose(labels, sizes, "largest", wrong="ties_high")[0].tolist() == [5]
    assert cm.choose(labels, sizes, 7)[0].tolist() == [0, 5] and cm.choose(labels, sizes, 7)[1] == [7, 7]
    with pytest.raises(ValueError, match="largest component has 7"):
        cm.choose(labels, sizes, 8)


# ------------------------------------------------------------------ the can, and the can with a floater
def test_the_can_is_one_component(can_model_volume):
    counts = tm.count_triangles(can_model_volume)
    sweeps = []
    labels, sizes = cm.label(counts, can_model_volume.dims, sweeps=sweeps)
    l26, _ = cm.label(counts, can_model_volume.dims, wrong="26")
    print(f"the can: {int((counts > 0).sum())} active cubes, {int(counts.sum())} triangles, sizes {sizes[sizes > 0].tolist()}, {sweeps[0]} sweeps")
    assert sizes[sizes > 0].tolist() == [83024] and len(cm.partition(l26)) == 1
    out = cm.extract_kept(can_model_volume, "largest")
    ref = tm.extract(can_model_volume)
    assert out["dropped_triangles"] == 0 and out["components"] == [83024]
    for got, want in zip((out["pos"], out["col"], out["nrm"], out["faces"]), ref):
        assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def can_with_ball(can_model_volume):
    vol = can_model_volume.copy()
    at, dist = cm.ball_footprint(vol.dims)
    # nothing of the can reaches the ball's footprint: there the fusion left tsdf exactly 1 (carved, or seen from beyond trunc), observed
    assert (vol.tsdf[at] == 1).all() and (vol.weight[at] >= 1).all() and len(at) > 200
    vol.tsdf[at] = cm.ball_values(dist)
    return vol


def test_the_can_with_a_ball_is_two_components(can_model_volume, can_with_ball):
    vol = can_with_ball
    s_mm = float(vol.voxel) * 1e3
    counts = tm.count_triangles(vol)
    labels, sizes = cm.label(counts, vol.dims)
    comp = sizes[sizes > 0].tolist()
    l26, _ = cm.label(counts, vol.dims, wrong="26")
    pos, col, nrm, faces = tm.extract(vol)
    bad, _, euler = tm.edge_report(faces)
    d = tm.cylinder_distance(pos, tm.CAN_RADIUS, tm.CAN_HEIGHT) * 1e3
    print(f"can + ball: components {comp} (by labels {np.nonzero(sizes > 0)[0].tolist()}), unfiltered {len(faces)} triangles, {bad} bad "
          f"edges, Euler {euler}, farthest vertex {d.max():.2f} mm from the cylinder")
    assert len(comp) == 2 and len(cm.partition(l26)) == 2
    ball = min(comp)
    assert max(comp) == 83024 and ball == len(faces) - 83024 and ball > 100
    assert bad == 0 and euler == 4 and d.max() > 10.0
    # the ball sits in the corner of smallest indices, so it carries the smaller label: 'largest' is not 'first'
    assert sizes[np.nonzero(sizes > 0)[0][0]] == ball
    kept = cm.extract_kept(vol, "largest")
    kbad, _, keuler = tm.edge_report(kept["faces"])
    kd = tm.cylinder_distance(kept["pos"], tm.CAN_RADIUS, tm.CAN_HEIGHT) * 1e3
    print(f"keep='largest': {len(kept['faces'])} triangles, {kbad} bad edges, Euler {keuler}, farthest vertex {kd.max():.3f} mm (one voxel "
          f"edge: {s_mm} mm), dropped {kept['dropped_triangles']}")
    assert kbad == 0 and keuler == 2 and kd.max() <= s_mm
    assert kept["components"] == sorted(comp, reverse=True) and kept["dropped_triangles"] == ball
    # what is kept is the can as it is extracted alone, bit for bit
    for got, want in zip((kept["pos"], kept["col"], kept["nrm"], kept["faces"]), tm.extract(can_model_volume)):
        assert np.array_equal(got, want)
    for n in (1, ball):
        both = cm.extract_kept(vol, n)
        assert both["dropped_triangles"] == 0 and np.array_equal(both["faces"], faces) and np.array_equal(both["pos"], pos)
    alone = cm.extract_kept(vol, ball + 1)
    assert np.array_equal(alone["faces"], kept["faces"]) and np.array_equal(alone["pos"], kept["pos"])
    with pytest.raises(ValueError, match="83024"):
        cm.extract_kept(vol, 83025)


# ------------------------------------------------------------------ refusals that need no device
def test_wrappers_refuse_before_any_device_call():
    from foundationpose_amd import _lib, ops
    from foundationpose_amd.reconstruct import reconstruct_object
    E = _lib.FpAmdError
    dims = (4, 5, 6)
    vol = [torch.ones(dims), torch.zeros(dims), torch.zeros(dims + (3,)), torch.zeros(dims)]
    for bad in (True, False, 0, -3, "biggest", "", 2.5, [1]):
        with pytest.raises(ValueError, match="keep must be"):
            ops.tsdf_extract(*vol, (0, 0, 0), 0.01, keep=bad)
        with pytest.raises(ValueError, match="keep_components must be"):
            reconstruct_object(np.zeros((1, 4, 4, 3)), np.ones((1, 4, 4)), np.ones((1, 4, 4)), np.eye(4)[None], np.eye(3), keep_components=bad)
    for good in ("largest", 1, np.int64(40)):                 # accepted: the next refusal is the device's
        with pytest.raises(E, match="CUDA"):
            ops.tsdf_extract(*vol, (0, 0, 0), 0.01, keep=good)
    counts = torch.zeros((3, 4, 5), dtype=torch.int32)
    with pytest.raises(E, match="CUDA"):
        ops.tsdf_components(counts, dims)
    with pytest.raises(E, match="cubes"):
        ops.tsdf_components(counts, (4, 5, 7))
    with pytest.raises(E, match="dimension"):
        ops.tsdf_components(counts, (4, 0, 6))
    with pytest.raises(E, match="dimension"):
        ops.tsdf_components(counts, (4, 5000, 6))
    with pytest.raises(ValueError, match="dims must be"):
        ops.tsdf_components(counts, (4, 5))
    with pytest.raises(E, match="tensor"):
        ops.tsdf_components(np.zeros(60, np.int32), dims)


def test_run_demo_refuses_a_keep_that_is_neither():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_demo", os.path.join(root, "scripts", "run_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit):
        mod.main(["--ref_keep_components", "biggest"])


def test_c_entry_point_reports_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(16)

    def call(nz=4, ny=4, nx=4, counts=p, labels=p, sizes=p):
        return lib.fp_tsdf_label_components(counts, nz, ny, nx, labels, sizes, None)

    for kw, word in ((dict(nx=0), b"dimension"), (dict(nz=-1), b"dimension"), (dict(ny=4097), b"dimension"),
                     (dict(nz=2048, ny=2048, nx=2048), b"2^30"), (dict(counts=None), b"NULL"), (dict(labels=None), b"NULL"),
                     (dict(sizes=None), b"NULL")):
        assert call(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_tsdf_label_components") and word in msg, (kw, msg)
    # no cubes: nothing to do, nothing is looked at
    assert call(ny=1, counts=None, labels=None, sizes=None) == 0 and call(nz=1, nx=1) == 0
