"""GPU: fp_mesh_point_distance against the numpy restatement of its definition (tests/mesh_distance_model.py) on every generated case
(tests/mesh_distance_cases.py): dist2 and closest bit-equal, face equal, no tolerance; what it may write; the same bits alone, in
another order, on another stream and from a replayed graph; the wrapper's refusals; reconstruct.sample_surface against its numpy
stand-in; and the layers above it (reconstruct.compare_meshes on the can fused from 16 noisy device renders, the setting of
tests/test_gpu_tsdf.py; FoundationPose.compare_to_mesh; scripts/run_demo.py --compare_mesh).

FP_MESH_DISTANCE_PROFILE_OUT=<file> merges the figures of a run into that JSON file (profiles/mesh_distance.json)."""
import itertools
import json

import numpy as np
import pytest
import torch

import mesh_distance_cases as mc
import mesh_distance_model as mm
import tsdf_model as tm
from test_gpu_multi_object import dev  # noqa: F401
from test_gpu_tsdf import Arena, _noisy_reference_views
from test_mesh_distance_host import CAN_N_ANG, facet_sag, record

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = mc.all_cases()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind == "i" else a.view(np.uint32)


def _assert_equal(got, ref, what):
    """got: the wrapper's dict (any subset of the outputs); ref: the restatement's (dist2, face, closest, ...)"""
    for k, r in zip(("dist2", "face", "closest"), ref):
        if k in got:
            g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
            assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
            bad = np.argwhere(_bits(g) != _bits(r))
            assert len(bad) == 0, (what, k, len(bad), "mismatches, first at", bad[0], g[tuple(bad[0])], r[tuple(bad[0])])


def _up(dev, c):
    return (torch.as_tensor(c["points"], device=dev), torch.as_tensor(c["pos"], device=dev), torch.as_tensor(c["faces"], device=dev))


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"].replace(" ", "_") for c in CASES])
def test_every_generated_case_equals_the_restatement(dev, ci):
    from foundationpose_amd import ops
    c = CASES[ci]
    pts, pos, faces = _up(dev, c)
    got = ops.mesh_point_distance(pts, pos=pos, faces=faces)
    assert sorted(got) == ["closest", "dist2", "face"]
    _assert_equal(got, mc.references()[c["name"]], c["name"])


def test_many_query_tiles_cut_the_faces_into_longer_chunks(dev):
    """2048 query tiles and more leave one chunk of all the faces to a workgroup (5 tiles of 256 here, the last one partial): the
    call on all 2048 * 256 + 77 queries has the bits of the calls on slices of it, which scan chunks of 1024 faces, and a seeded
    subset equals the restatement"""
    from foundationpose_amd import ops
    c = mc.soup(1100, 2048 * 256 + 77, 991)
    pts, pos, faces = _up(dev, c)
    whole = ops.mesh_point_distance(pts, pos=pos, faces=faces)
    for lo, hi in ((0, 1000), (300_000, 300_257), (len(c["points"]) - 65, len(c["points"]))):
        part = ops.mesh_point_distance(pts[lo:hi].contiguous(), pos=pos, faces=faces)
        for k in whole:
            assert torch.equal(part[k], whole[k][lo:hi]) and np.array_equal(_bits(part[k].cpu().numpy()), _bits(whole[k][lo:hi].cpu().numpy())), (k, lo)
    pick = np.random.default_rng(5).choice(len(c["points"]), 400, replace=False)
    ref = mm.mesh_point_distance(c["pos"], c["faces"], c["points"][pick])
    _assert_equal({k: v[torch.as_tensor(pick, device=dev)] for k, v in whole.items()}, ref, "subset of the large batch")


# ------------------------------------------------------------------ 2. what it writes
def test_writes_nothing_outside_its_outputs_and_workspace_for_every_subset(dev):
    """poisoned arenas around dist2, face, closest and the workspace (through the C ABI, where the workspace is the caller's), for every
    subset of the optional outputs; Q = 0 and F = 0"""
    from foundationpose_amd import _lib, ops
    lib = _lib.lib()
    c = next(c for c in CASES if c["name"] == "soup F=1025 Q=65")
    pts, pos, faces = _up(dev, c)
    ref = mc.references()[c["name"]]
    Q, F, Nv = len(c["points"]), len(c["faces"]), len(c["pos"])
    for want_face, want_closest in itertools.product((False, True), repeat=2):
        arena = Arena(dev)
        d2 = arena.new((Q,), torch.float32)
        fc = arena.new((Q,), torch.int32) if want_face else None
        cl = arena.new((Q, 3), torch.float32) if want_closest else None
        ws = arena.new((Q,), torch.int64)
        st = lib.fp_mesh_point_distance(ops._ptr(pos), Nv, ops._ptr(faces), F, ops._ptr(pts), Q, ops._ptr(d2), ops._ptr(fc), ops._ptr(cl),
                                        ops._ptr(ws), Q * 8, ops._stream(pts))
        assert st == 0, lib.fp_last_error()
        torch.cuda.synchronize()
        arena.check()
        got = dict(dist2=d2)
        if want_face:
            got["face"] = fc
        if want_closest:
            got["closest"] = cl
        _assert_equal(got, ref, f"face={want_face} closest={want_closest}")
        # the wrapper's subsets: dist2 is always there
        names = tuple(n for n, w in (("face", want_face), ("closest", want_closest)) if w) or ("dist2",)
        w = ops.mesh_point_distance(pts, pos=pos, faces=faces, want=names)
        assert sorted(w) == sorted(set(names) | {"dist2"})
        _assert_equal(w, ref, f"want={names}")
    # F = 0: every query unanswered; Q = 0: nothing happens, nothing is written
    arena = Arena(dev)
    d2, fc, cl, ws = arena.new((Q,), torch.float32), arena.new((Q,), torch.int32), arena.new((Q, 3), torch.float32), arena.new((Q,), torch.int64)
    assert lib.fp_mesh_point_distance(ops._ptr(pos), Nv, None, 0, ops._ptr(pts), Q, ops._ptr(d2), ops._ptr(fc), ops._ptr(cl), ops._ptr(ws),
                                      Q * 8, ops._stream(pts)) == 0
    torch.cuda.synchronize()
    arena.check()
    assert bool(torch.isinf(d2).all()) and bool((d2 > 0).all()) and bool((fc == -1).all()) and bool((cl == 0).all())
    before = [t.clone() for t in (d2, fc, cl, ws)]
    assert lib.fp_mesh_point_distance(ops._ptr(pos), Nv, ops._ptr(faces), F, ops._ptr(pts), 0, ops._ptr(d2), ops._ptr(fc), ops._ptr(cl),
                                      ops._ptr(ws), Q * 8, ops._stream(pts)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (d2, fc, cl, ws)))
    empty = ops.mesh_point_distance(pts[:0].contiguous(), pos=pos, faces=faces)
    assert tuple(empty["dist2"].shape) == (0,) and tuple(empty["closest"].shape) == (0, 3)
    none = ops.mesh_point_distance(pts, pos=pos, faces=faces[:0].contiguous())
    assert bool(torch.isinf(none["dist2"]).all()) and bool((none["face"] == -1).all()) and bool((none["closest"] == 0).all())


# ------------------------------------------------------------------ 3. the same bits every time
def test_alone_reversed_repeated_on_a_stream_and_from_a_graph(dev):
    from foundationpose_amd import ops
    c = next(c for c in CASES if c["name"] == "soup F=3000 Q=1000")
    pts, pos, faces = _up(dev, c)
    ref = mc.references()[c["name"]]
    batch = ops.mesh_point_distance(pts, pos=pos, faces=faces)
    _assert_equal(batch, ref, "batch")
    for k in (0, 255, 256, 999):                                   # a query alone
        one = ops.mesh_point_distance(pts[k:k + 1].contiguous(), pos=pos, faces=faces)
        _assert_equal(one, tuple(r[k:k + 1] for r in ref[:3]), f"query {k} alone")
    rev = ops.mesh_point_distance(pts.flip(0).contiguous(), pos=pos, faces=faces)
    _assert_equal({k: v.flip(0) for k, v in rev.items()}, ref, "reversed")
    for _ in range(3):
        _assert_equal(ops.mesh_point_distance(pts, pos=pos, faces=faces), ref, "repeated")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = ops.mesh_point_distance(pts, pos=pos, faces=faces)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _assert_equal(other, ref, "another stream")
    # a captured graph owns its outputs (out=) and takes its workspace from its own pool
    out = dict(dist2=torch.zeros(len(c["points"]), device=dev), face=torch.zeros(len(c["points"]), dtype=torch.int32, device=dev),
               closest=torch.zeros((len(c["points"]), 3), device=dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = ops.mesh_point_distance(pts, pos=pos, faces=faces, out=out)
    assert all(r[k].data_ptr() == out[k].data_ptr() for k in out)
    for _ in range(3):
        for t in out.values():
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(out, ref, "graph replay")
    pts.copy_(pts.flip(0))                                         # new queries in the graph's input buffer: the replay computes them
    g.replay()
    torch.cuda.synchronize()
    _assert_equal({k: v.flip(0) for k, v in out.items()}, ref, "graph replay on new queries")


def test_wrapper_refusals_on_device_tensors(dev):
    from foundationpose_amd import _lib, ops
    c = next(c for c in CASES if c["name"] == "box")               # 594 queries, 882 coordinates, 1296 indices: room for the aliases
    pts, pos, faces = _up(dev, c)
    Q = len(c["points"])
    big = torch.zeros(4 * Q, device=dev)
    for kw, msg in ((dict(points=pts.double()), "points: expected dtype"),
                    (dict(pos=pos.half()), "pos: expected dtype"),
                    (dict(faces=faces.long()), "faces: expected dtype"),
                    (dict(faces=faces.cpu()), "faces: expected a CUDA"),
                    (dict(pos=pos.cpu()), "pos: expected a CUDA"),
                    (dict(points=torch.zeros((2 * Q, 3), device=dev)[::2]), "points: tensor must be contiguous"),
                    (dict(pos=torch.zeros((3, len(c["pos"])), device=dev).t()), "pos: tensor must be contiguous"),
                    (dict(out=dict(dist2=torch.zeros(Q, dtype=torch.float64, device=dev))), r"out\['dist2'\]: expected dtype"),
                    (dict(out=dict(face=torch.zeros(Q, dtype=torch.int64, device=dev))), r"out\['face'\]: expected dtype"),
                    (dict(out=dict(closest=torch.zeros((Q, 3)))), r"out\['closest'\]: expected a CUDA"),
                    (dict(out=dict(closest=torch.zeros((3, Q), device=dev).t())), r"out\['closest'\]: tensor must be contiguous"),
                    (dict(out=dict(closest=torch.zeros((Q, 4), device=dev))), r"out\['closest'\] must be a tensor of shape"),
                    (dict(out=dict(closest=pts)), r"out\['closest'\] overlaps points"),
                    (dict(out=dict(dist2=pos.view(-1)[:Q])), r"out\['dist2'\] overlaps pos"),
                    (dict(out=dict(face=faces.view(-1)[:Q])), r"out\['face'\] overlaps faces"),
                    (dict(out=dict(dist2=big[:Q], closest=big[Q - 1:4 * Q - 1].view(Q, 3))), r"overlaps out\['")):
        args = dict(points=pts, pos=pos, faces=faces)
        args.update(kw)
        with pytest.raises(_lib.FpAmdError, match=msg):
            ops.mesh_point_distance(**args)
    good = ops.mesh_point_distance(pts, dict(pos=pos, faces=faces), out=dict(dist2=big[:Q], closest=big[Q:4 * Q].view(Q, 3)))
    _assert_equal(good, mc.references()[c["name"]], "mesh_tensors and adjacent buffers")


# ------------------------------------------------------------------ 4. sample_surface
def test_sample_surface_equals_its_stand_in(dev):
    """faces equal; points within the rounding of one float32 barycentric combination (three products and two sums of values up to
    M = max |coordinate|, each rounded once: 4 * 2^-24 * M covers a contracted evaluation too)"""
    from foundationpose_amd.reconstruct import sample_surface
    import geometry_cases as gc
    for m in (gc.l_prism(), gc.crossed_boxes(), gc.sliver_soup(n=500, n_twins=20)):
        pos, faces = np.asarray(m.vertices, f32), np.asarray(m.faces, np.int32)
        t = dict(pos=torch.as_tensor(pos, device=dev), faces=torch.as_tensor(faces, device=dev))
        for n, seed in ((1, 0), (1000, 0), (4097, 5)):
            pts, f = sample_surface(t, n, seed)
            rp, rf = mm.sample_surface(pos, faces, n, seed)
            assert pts.is_cuda and pts.dtype == torch.float32 and tuple(pts.shape) == (n, 3) and f.dtype == torch.int64
            assert np.array_equal(f.cpu().numpy(), rf)
            err = np.abs(pts.cpu().numpy().astype(np.float64) - rp).max()
            assert err <= 4 * 2.0 ** -24 * np.abs(pos).max(), (n, seed, err)


# ------------------------------------------------------------------ 5. end to end
@pytest.fixture(scope="module")
def can_fusion(scene, dev):
    from foundationpose_amd.reconstruct import reconstruct_object
    v = _noisy_reference_views(scene, dev)
    mesh, tensors = reconstruct_object(v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"], voxel=tm.CAN_VOXEL, device=dev)
    return v, mesh, tensors


SAMPLES = 200          # per direction: 200 x 4 900 + 200 x ~84 000 pair tests for the restatement


def test_compare_meshes_on_the_fused_can(scene, dev, can_fusion):
    """compare_meshes on the device equals the restatement's report computed from the device's own mesh arrays: both distance arrays
    bit-equal, every figure of the report equal; and its accuracy agrees with the distance of the same samples to the analytic
    cylinder within the sag of the true mesh's facets (tests/test_mesh_distance_host.py has the derivation)"""
    from foundationpose_amd.reconstruct import compare_meshes, sample_surface
    v, mesh, tensors = can_fusion
    true = scene["mesh"]
    thr = tuple(k * tm.CAN_VOXEL for k in (0.5, 1.0, 2.0, 4.0))
    got = compare_meshes(tensors, true, samples=SAMPLES, unit=tm.CAN_VOXEL)
    assert got.thresholds == thr and got.dist_a_to_b.is_cuda and got.dist_b_to_a.is_cuda
    a = (tensors["pos"].cpu().numpy(), tensors["faces"].cpu().numpy())
    b = (np.asarray(true.vertices, f32), np.asarray(true.faces, np.int32))
    ref = mm.compare_meshes(a, b, SAMPLES, thr)
    for k in ("dist_a_to_b", "dist_b_to_a"):
        g, r = getattr(got, k).cpu().numpy(), getattr(ref, k)
        assert g.dtype == r.dtype == f32 and np.array_equal(_bits(g), _bits(r)), k
    assert got[:8] == ref[:8], (got[:8], ref[:8])
    pts, _ = sample_surface(tensors, SAMPLES)
    d_cyl = tm.cylinder_distance(pts.cpu().numpy(), tm.CAN_RADIUS, tm.CAN_HEIGHT)
    d_mesh = got.dist_a_to_b.cpu().numpy().astype(np.float64)
    sag = facet_sag(tm.CAN_RADIUS, CAN_N_ANG)
    print(f"can from 16 noisy views, {len(a[1])} faces, {SAMPLES} samples: accuracy {got.accuracy}, completeness {got.completeness}, "
          f"chamfer {got.chamfer * 1e3:.3f} mm, F-score {got.fscore}; largest |to the mesh - to the cylinder| {np.abs(d_mesh - d_cyl).max() * 1e3:.4f} mm "
          f"(sag {sag * 1e3:.4f} mm)")
    assert np.abs(d_mesh - d_cyl).max() <= sag + 1e-7
    for name, fn in (("mean", np.mean), ("median", np.median), ("p99", lambda d: np.percentile(d, 99)), ("max", np.max)):
        assert abs(getattr(got.accuracy, name) - float(fn(d_cyl))) <= sag + 1e-7, name
    assert got.accuracy.max <= tm.CAN_VOXEL + sag
    record("can_device", dict(faces=len(a[1]), samples=SAMPLES, report=got.as_dict(), facet_sag_m=sag,
                              largest_difference_to_cylinder_distance_m=float(np.abs(d_mesh - d_cyl).max())))


def test_estimator_compare_to_mesh(scene, dev, can_fusion):
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.reconstruct import compare_meshes
    from test_gpu_pose_errors import _estimator
    v, mesh, tensors = can_fusion
    true_est = _estimator(scene["mesh"], dev)
    est = FoundationPose.from_reference_views(v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"], voxel=tm.CAN_VOXEL,
                                              scorer=true_est.scorer, refiner=true_est.refiner, device=dev)
    got = est.compare_to_mesh(scene["mesh"], samples=SAMPLES)             # unit: the pitch the mesh was fused at
    by_hand = compare_meshes(est.mesh_ori, scene["mesh"], samples=SAMPLES, unit=tm.CAN_VOXEL, device=dev)
    assert got[:8] == by_hand[:8] and got.thresholds == tuple(k * tm.CAN_VOXEL for k in (0.5, 1.0, 2.0, 4.0))
    assert torch.equal(got.dist_a_to_b, by_hand.dist_a_to_b) and torch.equal(got.dist_b_to_a, by_hand.dist_b_to_a)
    # ... and the fusion's own device tensors give the same report: mesh_ori holds their values
    direct = compare_meshes(tensors, scene["mesh"], samples=SAMPLES, unit=tm.CAN_VOXEL)
    assert direct[:8] == got[:8]
    with pytest.raises(ValueError, match="pass unit="):
        true_est.compare_to_mesh(scene["mesh"], samples=SAMPLES)           # a CAD estimator has no pitch: the caller names the unit


def test_run_demo_compare_mesh(tmp_path, dev, capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_demo", os.path.join(root, "scripts", "run_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    times = mod.main(["--synthetic_ref_views", "16", "--synthetic", "1", "--standin_weights", "--compare_mesh", "synthetic",
                      "--compare_samples", "20000", "--debug_dir", str(tmp_path / "d")])
    assert len(times) == 1
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{"compare_mesh"')]
    assert len(lines) == 1
    rep = json.loads(lines[0])["compare_mesh"]
    assert sorted(rep) == ["accuracy", "chamfer", "completeness", "faces", "fscore", "hausdorff", "precision", "recall", "samples",
                           "thresholds", "unit_m"]
    assert rep["samples"] == [20000, 20000] and len(rep["thresholds"]) == 4 and rep["faces"][1] == 4900
    assert rep["thresholds"] == [m * rep["unit_m"] for m in (0.5, 1.0, 2.0, 4.0)]
    assert 0 < rep["accuracy"]["median"] <= rep["accuracy"]["p99"] <= rep["accuracy"]["max"] <= rep["hausdorff"] < 0.01
    assert all(0.0 <= x <= 1.0 for k in ("precision", "recall", "fscore") for x in rep[k]) and rep["fscore"][-1] > 0.9
    print("run_demo --compare_mesh:", lines[0])
