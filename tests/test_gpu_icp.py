"""GPU: point-to-plane ICP (fp_icp_point_plane, ops.icp_point_plane, PoseRefinePredictor.depth_polish, estimater.depth_polish,
FoundationPose.polish, reconstruct.refine_view_poses, reconstruct_object(refine_poses=), scripts/run_demo.py --ref_refine_poses) from
the kernel up, against the numpy restatement of the definition (tests/icp_model.py).  The pair counts and the status are integers and
compared for equality; the float64 sums are held to the summation-error bound against exactly rounded sums, the step to the backward
error bound of the factorisation on the device's own system, the pose to one float32 ulp of the float64 update by the device's own
step.  Each test prints its figures before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import icp_model as im
import tsdf_model as tm
from conftest import ROOT
from test_gpu_depth_agreement import _estimators, _refiner, xyz  # noqa: F401
from test_gpu_multi_object import _t, dev, gmeshes, meshes  # noqa: F401
from test_gpu_multi_view import stack  # noqa: F401
from test_gpu_tsdf import _noisy_reference_views

pytestmark = pytest.mark.gpu
F = np.float32
POISON = -7.25


def profile():
    return json.load(open(os.path.join(ROOT, "profiles", "icp_polish.json")))


def _arena(shape, dtype, dev, pad=64):
    """a tensor of `shape` in the middle of a poisoned buffer -> (view, check): check() asserts the margins still hold the poison"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), POISON, dtype=dtype, device=dev)
    view = buf[pad:pad + n].view(shape)

    def check():
        assert (buf[:pad] == POISON).all() and (buf[pad + n:] == POISON).all(), "written outside the buffer"
    return view, check


def _run(c, dev, rows=None, min_pairs=6, damping=1e-3, arenas=False):
    """the op on a generated case (or on its rows `rows`) -> (system (n,40), poses_out (n,4,4)) numpy"""
    from foundationpose_amd import ops
    rows = np.arange(len(c["poses"])) if rows is None else np.asarray(rows)
    views = None
    if c["V"] > 1:
        views = ops.Views([np.eye(3)] * c["V"], np.zeros(len(rows), np.int64), dev)
        views.dev = _t(c["view"][rows].astype(np.int32), dev)            # the raw index: values outside 0..V-1 included
    xm = _t(c["xyz_map"] if c["V"] > 1 else c["xyz_map"][0], dev)
    n, (oh, ow) = len(rows), c["xyz_crops"].shape[1:3]
    kw, checks = {}, []
    if arenas:
        need = ops.icp_workspace(n, oh, ow, dev).numel()
        (kw["system"], c0), (kw["poses_out"], c1), (kw["workspace"], c2) = (_arena((n, 40), torch.float64, dev), _arena((n, 4, 4), torch.float32, dev),
                                                                             _arena((need,), torch.float64, dev))
        checks = [c0, c1, c2]
    out, system = ops.icp_point_plane(_t(c["xyz_crops"][rows], dev), _t(c["normal_crops"][rows], dev), xm, _t(c["tf"][rows], dev),
                                      _t(c["poses"][rows], dev), c["max_dist"], damping=damping, min_pairs=min_pairs, views=views, **kw)
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    return system.cpu().numpy(), out.cpu().numpy()


def _check_against_model(c, system, out, min_pairs=6, damping=1e-3):
    """every gate of the issue on one call's outputs; -> figures for the print"""
    pair, J, r = im.pixel_terms(c["xyz_crops"], c["normal_crops"], c["xyz_map"], c["tf"], c["poses"], c["max_dist"], c["view"])
    S, absS = im.sums(pair, J, r, exact=True)
    want_sys, _ = im.finish(S, c["poses"], damping, min_pairs)
    assert np.array_equal(system[:, 28], S[:, 28]), np.argwhere(system[:, 28] != S[:, 28])[:8]
    assert np.array_equal(system[:, 29], want_sys[:, 29]), (system[:, 29], want_sys[:, 29])
    assert (system[:, 36:] == 0).all()
    worst_sum = worst_res = worst_ulp = 0.0
    for n in range(len(S)):
        ok = np.isfinite(S[n, :28])
        # any order of summation of k terms is within (k - 1) u sum|term| of the exact sum, and the reference is its rounding
        bound = S[n, 28] * 2.0 ** -53 * absS[n]
        err = np.abs(system[n, :28][ok] - S[n, :28][ok])
        assert (err <= bound[ok]).all(), (n, err, bound)
        assert not np.isfinite(system[n, :28][~ok]).any()
        if ok.any() and (bound[ok] > 0).any():
            worst_sum = max(worst_sum, float((err[bound[ok] > 0] / bound[ok][bound[ok] > 0]).max()))
        x = system[n, 30:36]
        if system[n, 29] != 0:
            assert (x == 0).all() and np.array_equal(out[n].view(np.uint32), c["poses"][n].view(np.uint32)), n
            continue
        A = im.damped(system[n], damping).astype(np.longdouble)
        res = float(np.abs(A @ x.astype(np.longdouble) - system[n, 21:27].astype(np.longdouble)).max())
        bound = im.ldl_backward_bound(A.astype(np.float64), x)
        assert res <= bound, (n, res, bound)
        worst_res = max(worst_res, res / bound)
        ref = im.update64(c["poses"][n], x)
        ulp = np.spacing(np.abs(ref.astype(F))).astype(np.float64)
        d = np.abs(out[n].astype(np.float64) - ref) / ulp
        assert (d <= 1.0).all(), (n, d.max())
        assert np.array_equal(out[n, 3], c["poses"][n, 3])
        worst_ulp = max(worst_ulp, float(d.max()))
    return dict(pairs=S[:, 28].astype(int), status=system[:, 29].astype(int), sum_in_bounds=worst_sum, residual_in_bounds=worst_res,
                pose_in_ulps=worst_ulp)


# ------------------------------------------------------------------ 1. generated arrays
# crops of 1 x 1, 2 x 3, 37 x 53, 160 x 160 and one pixel below / above a workgroup's chunk of 256; N of 1, 3 and 70; V of 1 and 3
SHAPES = [(1, 1, 1, 1), (3, 2, 3, 3), (70, 37, 53, 3), (3, 160, 160, 1), (3, 15, 17, 1), (4, 257, 1, 3), (70, 16, 16, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_%dx%d_V%d" % s)
def test_generated_arrays(dev, shape):
    N, oh, ow, V = shape
    c = im.generated_case(N, oh, ow, V, seed=N + oh)
    system, out = _run(c, dev, arenas=True)
    fig = _check_against_model(c, system, out)
    print(f"{shape}: pairs {fig['pairs'][:10]}, status {fig['status'][:10]}, {c['thresholds']} threshold pixels; sums at {fig['sum_in_bounds']:.3f} "
          f"of their bound, residual at {fig['residual_in_bounds']:.3f} of its bound, poses within {fig['pose_in_ulps']:.3f} ulp")
    if N >= 70:
        assert {0, 1, 2} <= set(fig["status"].tolist())
    if V > 1 and N >= 3:
        off = (c["view"] < 0) | (c["view"] >= V)
        assert off.any() and (system[off, 28] == 0).all() and (system[off, :28] == 0).all()


def test_min_pairs_and_damping(dev):
    c = im.generated_case(4, 15, 17, V=1, seed=5)
    base, _ = _run(c, dev)
    n = int(np.argmax(np.where(base[:, 29] == 0, base[:, 28], -1)))
    k = int(base[n, 28])
    for mp, want in ((k + 1, 1), (k, 0)):
        system, out = _run(c, dev, min_pairs=mp)
        _check_against_model(c, system, out, min_pairs=mp)
        assert system[n, 29] == want
    system, out = _run(c, dev, damping=1.0)
    _check_against_model(c, system, out, damping=1.0)
    assert np.array_equal(system[:, :29], base[:, :29]) and not np.array_equal(system[n, 30:36], base[n, 30:36])
    from foundationpose_amd import ops
    e = ops.icp_point_plane(torch.zeros((0, 15, 17, 3), device=dev), torch.zeros((0, 15, 17, 3), device=dev), _t(c["xyz_map"][0], dev),
                            torch.zeros((0, 3, 3), device=dev), torch.zeros((0, 4, 4), device=dev), 0.02)
    assert e[0].shape == (0, 4, 4) and e[1].shape == (0, 40)


def test_rows_alone_reversed_and_repeated(dev):
    c = im.generated_case(70, 37, 53, 3, seed=107)
    system, out = _run(c, dev)
    again = _run(c, dev)
    assert np.array_equal(system.view(np.uint64), again[0].view(np.uint64)) and np.array_equal(out.view(np.uint32), again[1].view(np.uint32))
    rev = _run(c, dev, rows=np.arange(70)[::-1])
    assert np.array_equal(system.view(np.uint64), rev[0][::-1].view(np.uint64)) and np.array_equal(out.view(np.uint32), rev[1][::-1].view(np.uint32))
    for n in (0, 2, 3, 4, 33, 69):
        one = _run(c, dev, rows=[n])
        assert np.array_equal(one[0][0].view(np.uint64), system[n].view(np.uint64)), n
        assert np.array_equal(one[1][0].view(np.uint32), out[n].view(np.uint32)), n
    some = [5, 1, 68, 20]
    part = _run(c, dev, rows=some)
    assert np.array_equal(part[0].view(np.uint64), system[some].view(np.uint64))


def test_refusals_on_the_device(dev):
    from foundationpose_amd import _lib, ops
    c = im.generated_case(3, 15, 17, V=1, seed=3)
    a = [_t(c[k], dev) for k in ("xyz_crops", "normal_crops")] + [_t(c["xyz_map"][0], dev), _t(c["tf"], dev), _t(c["poses"], dev)]
    E = _lib.FpAmdError
    with pytest.raises(E, match="must not overlap"):
        ops.icp_point_plane(*a, 0.02, poses_out=a[4])
    with pytest.raises(E, match="must not overlap"):
        ops.icp_point_plane(*a, 0.02, poses_out=a[4].view(-1)[:48].view(3, 4, 4))
    with pytest.raises(E, match="system must be"):
        ops.icp_point_plane(*a, 0.02, system=torch.zeros((3, 39), dtype=torch.float64, device=dev))
    with pytest.raises(E, match="workspace of"):
        ops.icp_point_plane(*a, 0.02, workspace=torch.zeros(8, dtype=torch.float64, device=dev))
    with pytest.raises(E, match="normal_crops must be"):
        ops.icp_point_plane(a[0], a[1][:2].contiguous(), *a[2:], 0.02)
    with pytest.raises(E, match="poses of shape"):
        ops.icp_point_plane(*a[:4], a[4][:2].contiguous(), 0.02)
    with pytest.raises(E, match="xyz_map must be"):
        ops.icp_point_plane(a[0], a[1], a[2][None], a[3], a[4], 0.02)


# ------------------------------------------------------------------ 2. the scene
def _scene_of(scene, gmeshes, n):
    from foundationpose_amd.crops import Scene
    from foundationpose_amd.Utils import get_mesh_handle
    return Scene(get_mesh_handle(gmeshes["can"]), scene["diameter"], scene["K"], scene["H"], scene["W"], n)


def test_depth_polish_on_the_scene(scene, dev, gmeshes, xyz):
    """the 32 perturbations of the CPU test, four iterations on the device: inside the CPU test's gates; the loop is the three eager
    ops, and the pairs of every iteration are those of the restatement fed the device's renders"""
    from foundationpose_amd import ops
    prof = profile()["tracked_pose"]
    gate_t, gate_r = 2 * prof["worst_translation_mm"] * 1e-3, 2 * prof["worst_tilt_deg"]
    refiner = _refiner(dev)
    P0 = im.perturbations(scene["gt"], 32, seed=0)
    sc = _scene_of(scene, gmeshes, 32)
    with torch.inference_mode():
        P, system = refiner.depth_polish(_t(P0, dev), xyz, sc, iterations=4)
    dt, tilt = im.pose_errors(P.cpu().numpy(), scene["gt"])
    steps = ops.IcpStep.rows(system)
    print(f"depth_polish: {dt.max() * 1e3:.4f} mm, tilt {tilt.max():.5f} deg after 4 iterations (gates {gate_t * 1e3:.3f} mm, {gate_r:.4f} deg); "
          f"pairs {min(s.pairs for s in steps)} .. {max(s.pairs for s in steps)}, rms {max(s.rms for s in steps) * 1e3:.3f} mm")
    assert all(s.status == 0 for s in steps)
    assert dt.max() <= gate_t and tilt.max() <= gate_r
    # the same loop as eager ops, with the restatement's pairs per iteration
    Q = _t(P0, dev)
    xyz_np = xyz.cpu().numpy()
    for it in range(4):
        tf, bb = sc.crop_windows(Q, refiner.cfg["crop_ratio"], (160, 160))
        r = sc.render_crops(Q, bb, (160, 160), xyz_thr=0.001, normalize_xyz=False, want=("xyz", "normal"))
        Qn, sysd = sc.icp_point_plane(r["xyz"], r["normal"], xyz, tf, Q, 0.02)
        pair, _, _ = im.pixel_terms(r["xyz"].cpu().numpy(), r["normal"].cpu().numpy(), xyz_np, tf.cpu().numpy(), Q.cpu().numpy(), 0.02)
        assert np.array_equal(sysd[:, 28].cpu().numpy(), pair.reshape(32, -1).sum(1)), it
        Q = Qn
    assert torch.equal(Q, P) and torch.equal(sysd, system)
    with pytest.raises(ValueError, match="iterations"):
        refiner.depth_polish(_t(P0, dev), xyz, sc, iterations=0)


def test_depth_polish_graph_replays_the_eager_bits(scene, dev, gmeshes, xyz):
    refiner = _refiner(dev)
    sc = _scene_of(scene, gmeshes, 8)
    P0 = _t(im.perturbations(scene["gt"], 32, seed=0)[:8], dev)
    P1 = _t(im.perturbations(scene["gt"], 32, seed=1)[:8], dev)
    static = P0.clone()
    ws = sc.workspace(8, 160, 160, dev)
    with torch.inference_mode():
        eager = [tuple(t.clone() for t in refiner.depth_polish(p, xyz, sc, iterations=3, workspace=ws)) for p in (P0, P1)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            refiner.depth_polish(static, xyz, sc, iterations=3, workspace=ws)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out, system = refiner.depth_polish(static, xyz, sc, iterations=3, workspace=ws)
        for p, want in ((P0, eager[0]), (P1, eager[1]), (P0, eager[0])):
            static.copy_(p)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want[0]) and torch.equal(system.view(torch.int64), want[1].view(torch.int64))
    assert not torch.equal(eager[0][0], eager[1][0])


def test_estimators_polish(scene, dev, meshes, stack):
    """a multi-object, multi-view call equals the single calls; FoundationPose.polish is the one-estimator form"""
    from foundationpose_amd import estimater, ops
    names = ("can", "small_can", "can")
    ests = _estimators(meshes, names, dev)
    start = [_t(p[None], dev) for p in im.perturbations(scene["gt"], 32, seed=2)[:3]]

    def reset():
        for e, s in zip(ests, start):
            e.pose_last = s.clone()
    views = [2, 0, 1]
    reset()
    got = estimater.depth_polish(ests, stack["depths"], stack["Ks"], views=views, iterations=2)
    poses = [e.pose_last.clone() for e in ests]
    assert all(isinstance(s, ops.IcpStep) for s in got) and got[0].status == 0 and got[2].status == 0
    for k, e in enumerate(ests):
        reset()
        one = estimater.depth_polish([e], stack["depths"][views[k]], stack["Ks"][views[k]], iterations=2)
        assert repr(one[0]) == repr(got[k]) and torch.equal(e.pose_last, poses[k]), k       # (repr: a row without pairs has a NaN rms)
        assert e.pose_last.shape == (1, 4, 4)
    # one frame, several objects
    reset()
    many = estimater.depth_polish(ests[:2], scene["depth"], scene["K"], iterations=3)
    both = [e.pose_last.clone() for e in ests[:2]]
    reset()
    extra = {}
    pose = ests[0].polish(scene["depth"], scene["K"], iterations=3, extra=extra)
    assert extra["icp"] == many[0] and torch.equal(ests[0].pose_last, both[0])
    want = (ests[0].pose_last.reshape(4, 4) @ ests[0].get_tf_to_centered_mesh()).cpu().numpy()
    assert pose.shape == (4, 4) and np.array_equal(pose, want)
    dt, tilt = im.pose_errors(pose, scene["gt"])
    dt0, _ = im.pose_errors(start[0].cpu().numpy(), scene["gt"])
    print(f"FoundationPose.polish: {dt0[0] * 1e3:.2f} mm -> {dt[0] * 1e3:.3f} mm, tilt {tilt[0]:.4f} deg, {extra['icp']}")
    assert dt[0] <= 2e-3 * profile()["tracked_pose"]["after_3_iterations"]["worst_translation_mm"] and dt0[0] > 5e-3


# ------------------------------------------------------------------ 3. reference views
def _cylinder(vertices):
    d = tm.cylinder_distance(np.asarray(vertices), tm.CAN_RADIUS, tm.CAN_HEIGHT) * 1e3
    return float(np.median(d)), float(np.percentile(d, 99)), float(d.max())


def test_reference_view_poses_are_refined(scene, dev):
    """16 noisy device renders of the can with every pose off by up to 4 mm per axis and 0.5 .. 1.5 degrees: reconstruct_object with
    refine_poses=2 against the gates of the CPU test (the midpoints between the unrefined and the refined fuse measured there,
    profiles/icp_polish.json); refine_poses=0 is today's call, bit for bit; refine_view_poses moves the poses towards the truth"""
    from foundationpose_amd.reconstruct import reconstruct_object, refine_view_poses
    prof = profile()["reference_views"]
    v = _noisy_reference_views(scene, dev)
    P = im.view_perturbations(v["ob_in_cams"], seed=0)
    args = (v["rgb"], v["depth"], v["masks"])
    plain, pt = reconstruct_object(*args, P, v["Ks"], voxel=tm.CAN_VOXEL, device=dev)
    zero, zt = reconstruct_object(*args, P, v["Ks"], voxel=tm.CAN_VOXEL, device=dev, refine_poses=0)
    assert np.array_equal(plain.vertices, zero.vertices) and np.array_equal(plain.faces, zero.faces) and not hasattr(zero, "ob_in_cams")
    assert torch.equal(pt["pos"], zt["pos"]) and torch.equal(pt["vertex_color"], zt["vertex_color"])
    ref, _ = reconstruct_object(*args, P, v["Ks"], voxel=tm.CAN_VOXEL, device=dev, refine_poses=2)
    a, b = _cylinder(plain.vertices), _cylinder(ref.vertices)
    print(f"distance to the cylinder (median, p99, max) mm: perturbed poses {a}, after two rounds {b}; gates median {prof['gate_median_mm']:.3f}, "
          f"p99 {prof['gate_p99_mm']:.3f}")
    assert b[0] <= prof["gate_median_mm"] and b[1] <= prof["gate_p99_mm"]
    assert ref.ob_in_cams.shape == (16, 4, 4) and ref.ob_in_cams.dtype == np.float32
    # the poses themselves: one call of refine_view_poses against the first fuse
    Q, steps = refine_view_poses(pt, v["depth"], v["masks"], P, v["Ks"])
    e0 = np.linalg.norm(P[:, :3, 3] - v["ob_in_cams"][:, :3, 3], axis=1) * 1e3
    e1 = np.linalg.norm(Q.cpu().numpy()[:, :3, 3] - v["ob_in_cams"][:, :3, 3], axis=1) * 1e3
    print(f"view translations: {e0.mean():.2f} mm off on average before, {e1.mean():.2f} mm after one call; status {[s.status for s in steps]}")
    assert all(s.status == 0 for s in steps) and e1.mean() < e0.mean()
    # through the estimator: the refined poses stay readable
    from foundationpose_amd.estimater import FoundationPose
    from test_gpu_pose_errors import _estimator
    true_est = _estimator(scene["mesh"], dev)
    kw = dict(voxel=tm.CAN_VOXEL, scorer=true_est.scorer, refiner=true_est.refiner, device=dev)
    est = FoundationPose.from_reference_views(*args, P, v["Ks"], reconstruct_args={"refine_poses": 2}, **kw)
    assert np.array_equal(est.ref_ob_in_cams, ref.ob_in_cams) and len(est.mesh.faces) == len(ref.faces)
    assert FoundationPose.from_reference_views(*args, P, v["Ks"], **kw).ref_ob_in_cams is None


def test_run_demo_refines_reference_poses(tmp_path, dev):
    import importlib.util
    from foundationpose_amd.mesh_io import load_ply
    spec = importlib.util.spec_from_file_location("run_demo", os.path.join(ROOT, "scripts", "run_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ply = str(tmp_path / "can.ply")
    times = mod.main(["--synthetic_ref_views", "16", "--ref_refine_poses", "1", "--synthetic", "2", "--standin_weights", "--save_mesh", ply,
                      "--debug_dir", str(tmp_path / "d")])
    assert len(times) == 2
    mesh = load_ply(ply)
    d = tm.cylinder_distance(mesh.vertices, tm.CAN_RADIUS, tm.CAN_HEIGHT)
    print(f"run_demo --ref_refine_poses 1: {len(mesh.vertices)} vertices, max {d.max() * 1e3:.2f} mm from the cylinder")
    assert len(mesh.faces) > 10000 and np.median(d) < 1e-3
    with pytest.raises(SystemExit):
        mod.main(["--ref_refine_poses", "1", "--mesh_file", "x.obj", "--test_scene_dir", str(tmp_path)])
