"""GPU: fp_mesh_transform_residuals against the numpy restatement of its definition (tests/mesh_symmetry_model.py) on every generated
case (tests/mesh_symmetry_cases.py): max_d2 and dist2 bit-equal, over equal, no tolerance; what it may write; the same bits alone, in
another order, on another stream and from a replayed graph; the wrapper's refusals on device tensors; and the layers above it:
reconstruct.detect_symmetries on shapes with known groups and on the can, true and fused from 16 noisy device renders (the setting of
tests/test_gpu_tsdf.py), FoundationPose(symmetry_tfs="detect"), scripts/run_demo.py --detect_symmetry and
scripts/bench_mesh_symmetry.py."""
import itertools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_distance_cases as mc
import mesh_symmetry_cases as sc
import mesh_symmetry_model as sm
import tsdf_model as tm
from test_gpu_mesh_distance import _bits, can_fusion  # noqa: F401
from test_gpu_multi_object import dev  # noqa: F401
from test_gpu_tsdf import Arena
from test_mesh_distance_host import record
from test_mesh_symmetry_host import SHAPES, SIZES, group_tolerance, threshold_case

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = sc.kernel_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_equal(got, ref, what):
    """got: a dict with any of max_d2, over, dist2 (tensors or arrays); ref: the restatement's (max_d2, over, dist2)"""
    for k, r in zip(("max_d2", "over", "dist2"), ref):
        if k in got:
            g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
            assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
            bad = np.argwhere(_bits(g) != _bits(r))
            assert len(bad) == 0, (what, k, len(bad), "mismatches, first at", bad[0], g[tuple(bad[0])], r[tuple(bad[0])])


def _up(dev, c):
    return tuple(torch.as_tensor(c[k], device=dev) for k in ("points", "tfs", "pos", "faces"))


def _call(dev, c, dist2=True, stream_of=None):
    """the C entry point on a case, with the case's own squared thresholds -> dict of tensors"""
    from foundationpose_amd import _lib, ops
    lib = _lib.lib()
    pts, tfs, pos, faces = _up(dev, c)
    T, Q, L = len(c["tfs"]), len(c["points"]), len(c["thr2"])
    thr2 = torch.as_tensor(c["thr2"], device=dev) if L else None
    out = dict(max_d2=torch.empty(T, device=dev), over=torch.empty((T, L), dtype=torch.int32, device=dev))
    if dist2:
        out["dist2"] = torch.empty((T, Q), device=dev)
    need = int(lib.fp_mesh_transform_residuals_workspace_bytes(T, Q))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    st = lib.fp_mesh_transform_residuals(ops._ptr(pos), len(c["pos"]), ops._ptr(faces), len(c["faces"]), ops._ptr(pts), Q, ops._ptr(tfs), T,
                                         ops._ptr(thr2), L, ops._ptr(out["max_d2"]), ops._ptr(out["over"]) if L else None,
                                         ops._ptr(out.get("dist2")), ops._ptr(ws), need, ops._stream(pts))
    assert st == 0, lib.fp_last_error()
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"].replace(" ", "_") for c in CASES])
def test_every_generated_case_equals_the_restatement(dev, ci):
    c = CASES[ci]
    _assert_equal(_call(dev, c), sc.references()[c["name"]], c["name"])         # L = 0: over is (T, 0) on both sides


def test_identity_equals_mesh_point_distance_and_the_wrapper_squares_thresholds(dev):
    from foundationpose_amd import ops
    c = next(c for c in mc.all_cases() if c["name"] == "soup F=1025 Q=65")
    pts, pos, faces = (torch.as_tensor(c[k], device=dev) for k in ("points", "pos", "faces"))
    eye = torch.eye(4, device=dev)[None].contiguous()
    thr = (0.01, 0.02, 0.035, 0.05)
    got = ops.mesh_transform_residuals(pts, eye, pos=pos, faces=faces, thresholds=thr, want=("max_d2", "over", "dist2"))
    d2 = ops.mesh_point_distance(pts, pos=pos, faces=faces, want=("dist2",))["dist2"]
    assert torch.equal(got["dist2"][0], d2) and np.array_equal(_bits(got["dist2"][0].cpu().numpy()), _bits(mc.references()[c["name"]][0]))
    ref = sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], np.eye(4, dtype=f32)[None], sm.square_thresholds(thr))
    _assert_equal(got, ref, "wrapper with thresholds")
    few = ops.mesh_transform_residuals(pts, eye, dict(pos=pos, faces=faces))                 # no thresholds: no `over`
    assert sorted(few) == ["max_d2"] and torch.equal(few["max_d2"], got["max_d2"])


def test_thresholds_on_a_value_and_one_ulp_either_side(dev):
    c = threshold_case()
    _assert_equal(_call(dev, c), sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], c["tfs"], c["thr2"]), c["name"])


def test_many_pair_tiles_per_transform(dev):
    """T * Q = 3 x 180 011 pairs: 2 110 pair tiles, more than the 2 048 workgroups the grid wants, so the faces stay one chunk and a
    transform's samples spread over 700 tiles; the batch has the bits of its transforms alone (which cut the faces into chunks) and a
    seeded subset of its samples equals the restatement"""
    from foundationpose_amd import ops
    c = mc.soup(1100, 180_011, 992)
    pts, pos, faces = (torch.as_tensor(c[k], device=dev) for k in ("points", "pos", "faces"))
    tfs_h = sc.rigid_transforms(3, 17, 0.1)
    tfs = torch.as_tensor(tfs_h, device=dev)
    whole = ops.mesh_transform_residuals(pts, tfs, pos=pos, faces=faces, thresholds=(0.01, 0.03), want=("max_d2", "over", "dist2"))
    for t in range(3):
        one = ops.mesh_transform_residuals(pts[:70_000].contiguous(), tfs[t:t + 1].contiguous(), pos=pos, faces=faces, want=("dist2",))
        assert torch.equal(one["dist2"][0], whole["dist2"][t, :70_000])
    pick = np.random.default_rng(5).choice(len(c["points"]), 300, replace=False)
    ref = sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"][pick], tfs_h)
    assert np.array_equal(_bits(whole["dist2"][:, torch.as_tensor(pick, device=dev)].cpu().numpy()), _bits(ref[2]))
    d2 = whole["dist2"]
    assert torch.equal(whole["max_d2"], d2.max(dim=1).values)
    thr2 = torch.as_tensor(sm.square_thresholds((0.01, 0.03)), device=dev)
    assert torch.equal(whole["over"], (d2[:, :, None] > thr2).sum(dim=1).int())


# ------------------------------------------------------------------ 2. what it writes
def test_writes_nothing_outside_its_outputs_and_workspace_for_every_subset(dev):
    from foundationpose_amd import _lib, ops
    lib = _lib.lib()
    c = next(c for c in CASES if c["name"] == "three chunks T=5")
    pts, tfs, pos, faces = _up(dev, c)
    ref = sc.references()[c["name"]]
    T, Q, F, Nv, L = len(c["tfs"]), len(c["points"]), len(c["faces"]), len(c["pos"]), len(c["thr2"])
    thr2 = torch.as_tensor(c["thr2"], device=dev)
    for want_over, want_dist2 in itertools.product((False, True), repeat=2):
        arena = Arena(dev)
        mx = arena.new((T,), torch.float32)
        ov = arena.new((T, L), torch.int32) if want_over else None
        d2 = arena.new((T, Q), torch.float32) if want_dist2 else None
        ws = arena.new((T * Q,), torch.int32)
        st = lib.fp_mesh_transform_residuals(ops._ptr(pos), Nv, ops._ptr(faces), F, ops._ptr(pts), Q, ops._ptr(tfs), T,
                                             ops._ptr(thr2) if want_over else None, L if want_over else 0, ops._ptr(mx), ops._ptr(ov),
                                             ops._ptr(d2), ops._ptr(ws), T * Q * 4, ops._stream(pts))
        assert st == 0, lib.fp_last_error()
        torch.cuda.synchronize()
        arena.check()
        got = dict(max_d2=mx)
        if want_over:
            got["over"] = ov
        if want_dist2:
            got["dist2"] = d2
        _assert_equal(got, ref, f"over={want_over} dist2={want_dist2}")
    # Q = 0: max_d2 = 0 and over = 0, nothing else; T = 0: nothing happens
    arena = Arena(dev)
    mx, ov, ws = arena.new((T,), torch.float32), arena.new((T, L), torch.int32), arena.new((8,), torch.int32)
    assert lib.fp_mesh_transform_residuals(ops._ptr(pos), Nv, ops._ptr(faces), F, None, 0, None, T, ops._ptr(thr2), L, ops._ptr(mx), ops._ptr(ov),
                                           None, None, 0, ops._stream(pts)) == 0, lib.fp_last_error()
    torch.cuda.synchronize()
    arena.check()
    assert bool((mx == 0).all()) and bool((ov == 0).all())
    mx.fill_(3.0)
    assert lib.fp_mesh_transform_residuals(ops._ptr(pos), Nv, ops._ptr(faces), F, ops._ptr(pts), Q, ops._ptr(tfs), 0, ops._ptr(thr2), L,
                                           ops._ptr(mx), ops._ptr(ov), None, ops._ptr(ws), 32, ops._stream(pts)) == 0
    torch.cuda.synchronize()
    arena.check()
    assert bool((mx == 3.0).all())
    empty = ops.mesh_transform_residuals(pts[:0].contiguous(), tfs, pos=pos, faces=faces, thresholds=(0.1,), want=("max_d2", "over", "dist2"))
    assert tuple(empty["dist2"].shape) == (T, 0) and bool((empty["max_d2"] == 0).all()) and bool((empty["over"] == 0).all())
    none = ops.mesh_transform_residuals(pts, tfs[:0].contiguous(), pos=pos, faces=faces, thresholds=(0.1,))
    assert tuple(none["max_d2"].shape) == (0,) and tuple(none["over"].shape) == (0, 1)


# ------------------------------------------------------------------ 3. the same bits every time
def test_alone_reversed_repeated_on_a_stream_and_from_a_graph(dev):
    from foundationpose_amd import ops
    c = next(c for c in CASES if c["name"] == "three chunks T=5")
    pts, tfs, pos, faces = _up(dev, c)
    ref = sc.references()[c["name"]]
    thr = (0.004, 0.011, 0.02)
    ref = sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], c["tfs"], sm.square_thresholds(thr))
    names = ("max_d2", "over", "dist2")
    run = lambda p=pts, m=tfs, **kw: ops.mesh_transform_residuals(p, m, pos=pos, faces=faces, thresholds=thr, want=names, **kw)   # noqa: E731
    _assert_equal(run(), ref, "batch")
    for t in range(len(c["tfs"])):                                 # a transform alone
        _assert_equal(run(m=tfs[t:t + 1].contiguous()), tuple(r[t:t + 1] for r in ref), f"transform {t} alone")
    rev = run(m=tfs.flip(0).contiguous())
    _assert_equal({k: v.flip(0) for k, v in rev.items()}, ref, "transforms reversed")
    rev = run(p=pts.flip(0).contiguous())
    _assert_equal(dict(max_d2=rev["max_d2"], over=rev["over"], dist2=rev["dist2"].flip(1)), ref, "samples reversed")
    for _ in range(3):
        _assert_equal(run(), ref, "repeated")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _assert_equal(other, ref, "another stream")
    T, Q = len(c["tfs"]), len(c["points"])
    out = dict(max_d2=torch.zeros(T, device=dev), over=torch.zeros((T, 3), dtype=torch.int32, device=dev), dist2=torch.zeros((T, Q), device=dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = run(out=out)
    assert all(r[k].data_ptr() == out[k].data_ptr() for k in out)
    for _ in range(3):
        for t in out.values():
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(out, ref, "graph replay")
    tfs.copy_(tfs.flip(0))                                         # new transforms in the graph's input buffer: the replay computes them
    g.replay()
    torch.cuda.synchronize()
    _assert_equal({k: v.flip(0) for k, v in out.items()}, ref, "graph replay on new transforms")


def test_wrapper_refusals_on_device_tensors(dev):
    from foundationpose_amd import _lib, ops
    c = next(c for c in CASES if c["name"] == "box three transforms")
    pts, tfs, pos, faces = _up(dev, c)
    T, Q = len(c["tfs"]), len(c["points"])
    big = torch.zeros(T * Q + T + 4, device=dev)
    for kw, msg in ((dict(points=pts.double()), "points: expected dtype"), (dict(tfs=tfs.double()), "tfs: expected dtype"),
                    (dict(pos=pos.half()), "pos: expected dtype"), (dict(faces=faces.long()), "faces: expected dtype"),
                    (dict(faces=faces.cpu()), "faces: expected a CUDA"), (dict(tfs=tfs.cpu()), "tfs: expected a CUDA"),
                    (dict(tfs=torch.zeros((T, 4, 8), device=dev)[:, :, ::2]), "tfs: tensor must be contiguous"),
                    (dict(out=dict(max_d2=torch.zeros(T, dtype=torch.float64, device=dev))), r"out\['max_d2'\]: expected dtype"),
                    (dict(thresholds=(0.1,), out=dict(over=torch.zeros((T, 1), dtype=torch.int64, device=dev))), r"out\['over'\]: expected dtype"),
                    (dict(want=("dist2",), out=dict(dist2=torch.zeros((T, Q)))), r"out\['dist2'\]: expected a CUDA"),
                    (dict(out=dict(max_d2=tfs.view(-1)[:T])), r"out\['max_d2'\] overlaps tfs"),
                    (dict(out=dict(max_d2=pts.view(-1)[:T])), r"out\['max_d2'\] overlaps points"),
                    (dict(want=("dist2",), out=dict(max_d2=big[:T], dist2=big[T - 1:T - 1 + T * Q].view(T, Q))), r"overlaps out\['")):
        args = dict(points=pts, tfs=tfs, pos=pos, faces=faces)
        args.update(kw)
        with pytest.raises(_lib.FpAmdError, match=msg):
            ops.mesh_transform_residuals(**args)
    good = ops.mesh_transform_residuals(pts, tfs, pos=pos, faces=faces, want=("dist2",), out=dict(max_d2=big[:T], dist2=big[T:T + T * Q].view(T, Q)))
    ref = sc.references()[c["name"]]
    _assert_equal(good, (ref[0], None, ref[2]), "adjacent buffers")


# ------------------------------------------------------------------ 4. detection on the device
@pytest.mark.parametrize("name", ["cube", "box 1x1x2"])
def test_detected_groups_of_closed_form_shapes(dev, name):
    from foundationpose_amd.reconstruct import detect_symmetries
    from foundationpose_amd.symmetry import surface_centre
    shape, group, kw = SHAPES[name]
    pos, faces, R, t = sc.posed(shape(), seed=3 + len(name))
    rec = detect_symmetries(dict(pos=torch.as_tensor(pos, device=dev), faces=torch.as_tensor(faces, device=dev)), **kw)
    _, radius = surface_centre(pos, faces)
    ok, worst = sc.match_groups(rec.tfs[:, :3, :3], R @ group() @ R.T, group_tolerance(rec, radius))
    assert len(rec.tfs) == SIZES[name] and ok, (name, len(rec.tfs), worst)
    assert (rec.residuals <= rec.tol).all()


def _check_can(rec, axis, centre, what):
    """a continuous axis along `axis` through `centre` with one flip: 144 transforms at 5 degrees"""
    assert rec.continuous_axis is not None, (what, rec.axes)
    tilt = math.degrees(math.acos(min(1.0, abs(float(rec.continuous_axis @ axis)))))
    off = np.linalg.norm(np.cross(rec.centre - centre, axis))
    print(f"{what}: {len(rec.tfs)} transforms, axes {[k for _, k in rec.axes]}, axis off by {tilt:.4f} deg and {off * 1e3:.4f} mm, largest residual "
          f"{rec.residuals.max() * 1e3:.4f} mm (tol {rec.tol * 1e3:.3f} mm)")
    assert [k for _, k in rec.axes] == [math.inf, 2] and len(rec.tfs) == 144, (what, rec.axes, len(rec.tfs))
    assert (rec.residuals <= rec.tol).all()
    return tilt, off


def test_the_true_can(scene, dev):
    from foundationpose_amd.reconstruct import detect_symmetries
    rec = detect_symmetries(scene["mesh"])
    tilt, off = _check_can(rec, np.array([0.0, 0, 1]), np.zeros(3), "true can")
    # the axis within the detector's own merging angle (symmetry.py: max(1 degree, 2 tol / radius)), the centre within tol of it
    assert tilt <= math.degrees(max(math.radians(1.0), 2 * rec.tol / math.hypot(tm.CAN_RADIUS, tm.CAN_HEIGHT / 2))) and off <= rec.tol
    record("symmetry_true_can_device", dict(transforms=len(rec.tfs), tilt_deg=tilt, largest_residual_m=float(rec.residuals.max())))


def test_the_can_fused_from_noisy_renders(scene, dev, can_fusion):
    """The can fused on the device from 16 noisy renders: the residual of the true axis at 2 pi / 7 and 2 pi / 11 is measured, the
    detector runs at twice that and no less than one voxel (the rule tests/test_mesh_symmetry_host.py records), and finds the
    continuous axis with its flip"""
    from foundationpose_amd import ops
    from foundationpose_amd.reconstruct import detect_symmetries, sample_surface
    from foundationpose_amd.symmetry import about, axis_rotation
    v, mesh, tensors = can_fusion
    pts, _ = sample_surface(tensors, 512)
    tfs = np.stack([about(np.zeros(3), axis_rotation((0, 0, 1), 2 * math.pi / k)) for k in (7, 11)]).astype(f32)
    res = ops.mesh_transform_residuals(pts, torch.as_tensor(tfs, device=dev), tensors)["max_d2"].double().sqrt().cpu().numpy()
    tol = float(max(2 * res.max(), tm.CAN_VOXEL))
    print(f"fused can, {int(tensors['faces'].shape[0])} faces: residual of the true axis at 2pi/7 {res[0] * 1e3:.4f} mm, at 2pi/11 {res[1] * 1e3:.4f} mm; "
          f"detector at {tol * 1e3:.3f} mm")
    rec = detect_symmetries(tensors, tol=tol)
    tilt, off = _check_can(rec, np.array([0.0, 0, 1]), np.zeros(3), "fused can")
    assert tilt <= math.degrees(max(math.radians(1.0), 2 * rec.tol / math.hypot(tm.CAN_RADIUS, tm.CAN_HEIGHT / 2))) and off <= rec.tol
    record("symmetry_fused_can_device", dict(faces=int(tensors["faces"].shape[0]), residual_2pi_7_m=float(res[0]), residual_2pi_11_m=float(res[1]),
                                             tol_m=tol, tilt_deg=tilt, transforms=len(rec.tfs)))


# ------------------------------------------------------------------ 5. through the estimator
def test_estimator_with_detected_symmetries(scene, dev, can_fusion):
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.symmetry import about, axis_rotation
    from foundationpose_amd.Utils import cluster_poses
    from test_gpu_pose_errors import _estimator
    v, mesh, tensors = can_fusion
    true_est = _estimator(scene["mesh"], dev)
    args = (v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"])
    kw = dict(voxel=tm.CAN_VOXEL, scorer=true_est.scorer, refiner=true_est.refiner, device=dev)
    # None: as before.  (from_reference_views hands the fused mesh to the constructor; the fixture's fusion is that mesh.)
    plain = FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, mesh=mesh, mesh_tensors=tensors,
                           scorer=true_est.scorer, refiner=true_est.refiner, device=dev)
    assert plain.symmetries is None and tuple(plain.symmetry_tfs.shape) == (1, 4, 4) and len(plain.rot_grid) == 252
    assert torch.equal(plain.symmetry_tfs[0], torch.eye(4, device=dev))
    est = FoundationPose.from_reference_views(*args, symmetry_tfs="detect", **kw)
    rec = est.symmetries
    assert rec is not None and rec.tol == 2 * tm.CAN_VOXEL and len(rec.tfs) == 144 and tuple(est.symmetry_tfs.shape) == (144, 4, 4)
    # the hand-written table of the same group, about the same point: rotations about z every 5 degrees, times one flip
    c = rec.centre + est.model_center
    hand = about(c, np.stack([s @ f for f in (np.eye(3), axis_rotation((1, 0, 0), math.pi))
                              for s in (axis_rotation((0, 0, 1), math.radians(d)) for d in range(0, 360, 5))]))
    grid = cluster_poses(30, 99999, plain.rot_grid.cpu().numpy(), hand.astype(np.float32))
    print(f"rotation grid: {len(est.rot_grid)} hypotheses with the detected table, {len(grid)} with the hand-written one, 252 without")
    assert len(est.rot_grid) < 252 and len(est.rot_grid) == len(grid)
    # a pose turned about the detected axis: the same pose to the symmetry-aware error, another one to ADD
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = axis_rotation((1, 2, 3), 0.7), (0.02, -0.01, 0.6)
    turned = gt @ about(c, axis_rotation(rec.continuous_axis, math.radians(100.0)))
    from_centred = np.eye(4)                                       # poses are given in the centred-mesh frame
    from_centred[:3, 3] = est.model_center
    errs = est.pose_errors(gt, poses=(turned @ from_centred)[None]).cpu().numpy()[0]
    print(f"pose turned by 100 deg about the detected axis: add {errs[0] * 1e3:.3f} mm, add_sym {errs[2] * 1e3:.3f} mm, mssd {errs[3] * 1e3:.3f} mm")
    assert errs[0] > 0.02 and errs[3] < rec.tol and errs[2] < rec.tol
    with pytest.raises(ValueError, match="'detect'"):
        est.reset_object(mesh.vertices, mesh.vertex_normals, symmetry_tfs="auto", mesh=mesh)


def test_run_demo_detect_symmetry(tmp_path, dev, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_demo", os.path.join(ROOT, "scripts", "run_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    times = mod.main(["--synthetic", "1", "--standin_weights", "--detect_symmetry", "--debug_dir", str(tmp_path / "d")])
    assert len(times) == 1
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{"detect_symmetry"')]
    assert len(lines) == 1
    rep = json.loads(lines[0])["detect_symmetry"]
    assert rep["transforms"] == 144 and rep["hypotheses"] < 252 and [a["order"] for a in rep["axes"]] == ["continuous", 2]
    assert rep["largest_residual_m"] <= rep["tol_m"]
    print("run_demo --detect_symmetry:", lines[0])


def test_bench_script_runs(dev):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_mesh_symmetry.py"), "--transforms", "40", "--iters", "2",
                          "--fused_faces", "0", "--skip_detection"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["transforms"] == 40 and line["samples"] == 64 and line["cases"][0]["faces"] == 4900
    assert line["cases"][0]["fused_ms"] > 0 and line["cases"][0]["materialised_ms"] > 0 and isinstance(line["cases"][0]["same_bits"], bool)
    # the two routes differ by the rounding of the transformed points alone (torch's matmul has its own order and may fuse): 24 u M
    # with M = 0.1 m is 0.14 um (tests/test_mesh_symmetry_host.py has the count); a root of a small d2 amplifies it, so 1 um
    assert line["cases"][0]["largest_difference_m"] <= 1e-6
