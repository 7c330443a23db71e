"""GPU: the depth-agreement check (fp_depth_agreement, ops.depth_agreement, PoseRefinePredictor.depth_check) from the kernel up to the
estimators.  The counts are integers, so every comparison here is equality: the kernel against the numpy restatement of
tests/agreement_model.py on the GPU render's depth crops and the z channel of the REFINE warp, the trackers' table against the eager
op on their output poses, graph replay against eager launches.  The geometric tests check the directions the counts move in."""
import numpy as np
import pytest
import torch

from agreement_model import counts as model_counts
from test_gpu_multi_object import _diameter, _interleaved, _poses, _set, _t, dev, gmeshes, meshes  # noqa: F401
from test_gpu_multi_view import stack  # noqa: F401

pytestmark = pytest.mark.gpu
TOLS = (0.002, 0.01, 0.05)


def _ingest(depth, K, dev):
    """the tracking ingest of one frame: erode, bilateral, back-projection in f32 -> (H,W,3)"""
    from foundationpose_amd import ops
    d = ops.bilateral_filter_depth(ops.erode_depth(torch.as_tensor(np.asarray(depth, np.float32), device=dev), radius=2), radius=2)
    return ops.depth_to_xyz(d, K, zfar=float("inf"), f64_internal=False)


@pytest.fixture(scope="module")
def xyz(scene, dev):
    return _ingest(scene["depth"], scene["K"], dev)


def _op(P, xyz_t, K, handle, diam, tol, obj=None, views=None, crop=(160, 160), crop_ratio=1.2):
    """the check as three eager ops: crop windows, the render's depth, depth_agreement -> ((N,4) int32, tf, depth crops)"""
    from foundationpose_amd import ops
    oh, ow = crop
    tf, bb = ops.crop_windows(P, K, diam, crop_ratio, (ow, oh), obj=obj, views=views)
    H, W = int(xyz_t.shape[-3]), int(xyz_t.shape[-2])
    dc = ops.render_crops(handle, P, bb, K, H, W, (oh, ow), diam, normalize_xyz=False, want=("depth",), obj=obj, views=views)["depth"]
    return ops.depth_agreement(dc, xyz_t, tf, tol, views=views), tf, dc


def _z_of_warp(rgb_t, xyz_t, tf, K, P, diam, obj=None, views=None):
    """z channel of the REFINE warp without normalisation, the translations zeroed: the observed z of every crop pixel"""
    from foundationpose_amd import ops
    P0 = P.clone()
    P0[:, :3, 3] = 0
    B = ops.warp_crops(rgb_t, xyz_t, None, tf, K, P0, diam, ops.MODE_REFINE, normalize_xyz=False, obj=obj, views=views)
    return B[:, 5].cpu().numpy()


# ------------------------------------------------------------------ 1. exact counts
def test_counts_are_the_numpy_classification(scene, dev, gmeshes, xyz):
    """the 252 grid poses, the GT pose and 32 perturbations of it, three tolerances: the kernel's counts equal the numpy classification
    of the render's depth crops against the warp's z, element for element"""
    from foundationpose_amd.Utils import get_mesh_handle
    handle = get_mesh_handle(gmeshes["can"])
    P = np.concatenate([scene["poses"], scene["gt"][None], _poses(scene, 32, seed=3, max_trans=0.02, max_rot_deg=20)]).astype(np.float32)
    Pt = _t(P, dev)
    rgb_t = torch.as_tensor(scene["rgb"], device=dev).float().contiguous()
    seen = np.zeros(4, np.int64)
    for tol in TOLS:
        got, tf, dc = _op(Pt, xyz, scene["K"], handle, scene["diameter"], tol)
        zo = _z_of_warp(rgb_t, xyz, tf, scene["K"], Pt, scene["diameter"])
        want = model_counts(dc.cpu().numpy(), zo, tol)
        assert np.array_equal(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:8]
        seen += want.sum(0)
        front = want[:, 1] - want[:, 2] - want[:, 3]
        assert (front >= 0).all() and (want[:, 3] > 0).any() and (front > 0).any()
    assert (seen > 0).all()
    # replay-stable and order-free: a second call, and the rows in reverse order, give the same integers
    again = _op(Pt, xyz, scene["K"], handle, scene["diameter"], 0.01)[0]
    rev = _op(Pt.flip(0).contiguous(), xyz, scene["K"], handle, scene["diameter"], 0.01)[0]
    assert torch.equal(again, rev.flip(0))
    # N == 0 is a no-op
    from foundationpose_amd import ops
    e = ops.depth_agreement(torch.zeros((0, 160, 160), device=dev), xyz, torch.zeros((0, 3, 3), device=dev), 0.01)
    assert e.shape == (0, 4)


def test_views_are_the_single_frame_calls(scene, dev, meshes, gmeshes, stack):
    """48 hypotheses over four meshes and three frames with different K: the view form equals single-frame calls per view; a view
    index outside 0..V-1 reads nothing (valid == agree == behind == 0, model as before)"""
    from foundationpose_amd import ops
    names = ("can", "box", "torus", "small_can")
    mset, _, diam = _set(names, meshes, gmeshes, dev)
    dt = ops.object_diameters(diam, dev)
    N = 48
    view = _interleaved(3, N, seed=21)
    obj = _t(_interleaved(4, N, seed=22), dev)
    vt = ops.Views(stack["Ks"], view, dev)
    P = _t(_poses(scene, N, seed=23, max_rot_deg=30), dev)
    tf, bb = ops.crop_windows(P, None, dt, 1.2, (160, 160), obj=obj, views=vt)
    dc = ops.render_crops(mset, P, bb, None, 480, 640, (160, 160), dt, normalize_xyz=False, want=("depth",), obj=obj, views=vt)["depth"]
    for tol in TOLS:
        got = ops.depth_agreement(dc, stack["xyz_t"], tf, tol, views=vt)
        zo = _z_of_warp(stack["rgb_t"], stack["xyz_t"], tf, None, P, dt, obj=obj, views=vt)
        assert np.array_equal(got.cpu().numpy(), model_counts(dc.cpu().numpy(), zo, tol))
        for v in range(3):
            r = torch.as_tensor(np.nonzero(view == v)[0], device=dev)
            one = ops.depth_agreement(dc[r].contiguous(), stack["xyz_t"][v], tf[r].contiguous(), tol)
            assert torch.equal(one, got[r])
        assert (got[:, 2] > 0).sum() >= N // 2
    bad = ops.Views(stack["Ks"], view, dev)
    vb = view.copy()
    vb[::5] = 3
    vb[1::7] = -1
    bad.dev = _t(vb.astype(np.int32), dev)
    out = torch.full((N, 4), -7, dtype=torch.int32, device=dev)
    ops.depth_agreement(dc, stack["xyz_t"], tf, 0.01, views=bad, out=out)      # out=: zeroed and filled
    good = ops.depth_agreement(dc, stack["xyz_t"], tf, 0.01, views=vt)
    off = (vb < 0) | (vb >= 3)
    o = out.cpu().numpy()
    assert (o[off, 1:] == 0).all() and np.array_equal(o[off, 0], good.cpu().numpy()[off, 0]) and (o[off, 0] > 0).all()
    assert np.array_equal(o[~off], good.cpu().numpy()[~off])


# ------------------------------------------------------------------ 2. geometry
def _shifted(T, along_ray_m=0.0, sideways_m=0.0):
    P = np.asarray(T, np.float64).copy()
    t = P[:3, 3]
    P[:3, 3] = t + along_ray_m * t / np.linalg.norm(t) + np.asarray([sideways_m, 0.0, 0.0])
    return P.astype(np.float32)


def test_geometry(scene, dev, gmeshes, xyz):
    from foundationpose_amd.ops import DepthAgreement
    from foundationpose_amd.Utils import get_mesh_handle
    handle = get_mesh_handle(gmeshes["can"])
    gt = scene["gt"]
    P = np.stack([gt.astype(np.float32), _shifted(gt, -0.05), _shifted(gt, 0.05), _shifted(gt, sideways_m=2.0)])
    at, toward, away, aside = DepthAgreement.rows(_op(_t(P, dev), xyz, scene["K"], handle, scene["diameter"], 0.01)[0])
    # measured on MI355X (model, valid, agree, behind): GT (6258, 5884, 5771, 110), agree_frac 0.981; 5 cm toward the camera
    # (6287, 5867, 0, 5867); 5 cm away (6271, 6257, 0, 0), front 6257; 2 m sideways (11722, 0, 0, 0).  The thresholds leave margin.
    assert at.agree_frac > 0.9 and toward.agree_frac < 0.1
    assert toward.behind > 0.8 * toward.valid
    assert away.front > 0.8 * away.valid
    assert aside.model > 0 and aside.valid == 0
    # an occluder: a band of the observed depth at 0.4 m across the middle third of the object's rows
    v, u = np.nonzero(scene["mask"])
    v0, v1 = v.min(), v.max()
    h = v1 - v0 + 1
    occ = scene["depth"].copy()
    occ[v0 + h // 3:v0 + 2 * h // 3, u.min():u.max() + 1] = 0.4
    xyz_occ = _ingest(occ, scene["K"], dev)
    b = DepthAgreement.rows(_op(_t(P[:1], dev), xyz_occ, scene["K"], handle, scene["diameter"], 0.01)[0])[0]
    # measured: (6258, 5720, 3071, 71), front 2578 against 3 on the clean frame; agree 3071 against 5771 (both moves ~0.4 model)
    assert b.front > at.front + 0.2 * at.model and b.agree < at.agree - 0.2 * at.model


# ------------------------------------------------------------------ 3. trackers
def _refiner(dev):
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    from foundationpose_amd.weights import CONTRACTION_HEAD_SCALE, DEFAULT_REFINE_CFG, random_state_dict
    return PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), device=dev,
                               state_dict=random_state_dict("refine", seed=0, head_scale=CONTRACTION_HEAD_SCALE))


def _tracker_op(trk, P, xyz_t):
    """the eager op on a tracker's poses: its own meshes, diameters, object / view index and crop settings"""
    oh, ow = int(trk.refiner.cfg["input_resize"][0]), int(trk.refiner.cfg["input_resize"][1])
    obj = None if trk.obj is None else trk.obj.dev
    K = None if trk.views is not None else trk.K
    return _op(P, xyz_t, K, trk.handle, trk.diameter, trk.agreement_tol, obj=obj, views=trk.views, crop=(oh, ow),
               crop_ratio=trk.refiner.cfg["crop_ratio"])[0]


CASES = {"one": dict(names=None, views=None), "four_meshes": dict(names=("can", "torus", "box", "small_can"), views=None),
         "three_views": dict(names=("can", "box", "can", "torus", "box", "small_can"), views=[0, 0, 1, 1, 2, 2])}


@pytest.mark.parametrize("case", list(CASES))
def test_tracker_agreement(scene, dev, meshes, gmeshes, stack, case):
    """poses_out bit-identical with and without agreement_tol; trk.agreement = the eager op on poses_out; replay = step_eager; the
    FramePipeline fills the same table as step (single-view trackers)"""
    from foundationpose_amd.graphs import FramePipeline, GraphedTracker
    c = CASES[case]
    refiner = _refiner(dev)
    if c["names"] is None:
        args = (gmeshes["can"], scene["diameter"], scene["K"])
        M = 1
    else:
        M = len(c["names"])
        args = ([gmeshes[k] for k in c["names"]], [_diameter(meshes[k]) for k in c["names"]],
                scene["K"] if c["views"] is None else stack["Ks"])
    kw = dict(n_hyp=1, iteration=2, device=dev, views=c["views"])
    plain = GraphedTracker(refiner, *args, 480, 640, **kw).capture()
    trk = GraphedTracker(refiner, *args, 480, 640, agreement_tol=0.01, **kw).capture()
    assert plain.agreement is None and trk.agreement.shape == (M, 4)
    frames = []
    for f in range(3):
        P = _poses(scene, M, seed=61 + f, max_trans=0.02, max_rot_deg=15)
        if c["views"] is None:
            frames.append((scene["rgb"], (scene["depth"] + 0.0007 * f).astype(np.float32), P))
        else:
            frames.append(([np.roll(r, 2 * f, axis=1) for r in stack["rgbs"]], [d + 0.001 * f for d in stack["depths"]], P))
    for rgb, depth, P in frames:
        a = plain.step(rgb, depth, P).clone()
        b = trk.step(rgb, depth, P).clone()
        assert torch.equal(a, b)
        g = trk.agreement.clone()
        assert torch.equal(g, _tracker_op(trk, trk.poses_out, trk.xyz))
        assert (g[:, 0] > 0).all() and (g[:, 2] > 0).any()
        e = trk.step_eager(rgb, depth, P).clone()
        assert torch.equal(e, b) and torch.equal(trk.agreement, g)
    if c["views"] is not None:
        return
    ref = []
    for rgb, depth, P in frames:
        trk.step(rgb, depth, P)
        ref.append(trk.agreement.clone())
    pipe = FramePipeline(trk)
    trk._have_output = False
    got = []
    to_host = [(torch.from_numpy(np.ascontiguousarray(rgb)).pin_memory(), torch.from_numpy(depth).pin_memory(),
                torch.from_numpy(P).pin_memory()) for rgb, depth, P in frames]
    pipe.submit(0, *to_host[0])
    for f in range(len(frames)):
        if f + 1 < len(frames):
            pipe.submit((f + 1) % 2, *to_host[f + 1])
        pipe.run(f % 2)
        got.append(trk.agreement.clone())
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, ref))


# ------------------------------------------------------------------ 4. estimators
def _estimators(meshes, names, dev, refiner=None, track_graph=False):
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.predict_score import ScorePredictor
    from foundationpose_amd.weights import DEFAULT_SCORE_CFG, random_state_dict
    refiner = refiner or _refiner(dev)
    scorer = ScorePredictor(cfg=dict(DEFAULT_SCORE_CFG), state_dict=random_state_dict("score", seed=0), device=dev)
    return [FoundationPose(model_pts=meshes[k].vertices, model_normals=meshes[k].vertex_normals, mesh=meshes[k], scorer=scorer,
                           refiner=refiner, device=dev, track_graph=track_graph) for k in names]


def _est_op(ests, P, xyz_t, K, dev, views=None):
    from foundationpose_amd import ops
    from foundationpose_amd.estimater import _object_tables
    mset, diam = _object_tables(ests[0].refiner, ests)
    obj = torch.arange(len(ests), dtype=torch.int32, device=dev)
    table = _op(P, xyz_t, K, mset, diam, 0.01, obj=obj, views=views)[0]
    return ops.DepthAgreement.rows(table)


@pytest.mark.parametrize("graphed", [True, False], ids=["graphed", "eager"])
def test_track_one(scene, dev, meshes, xyz, graphed):
    from foundationpose_amd import ops
    from foundationpose_amd.Utils import get_mesh_handle
    est = _estimators(meshes, ("can",), dev, track_graph=graphed)[0]
    assert est.depth_agreement is None
    start = _t(_poses(scene, 1, seed=71, max_trans=0.015, max_rot_deg=10), dev)
    for f in range(3):
        depth = (scene["depth"] + 0.0005 * f).astype(np.float32)
        est.pose_last = start.clone()
        plain = est.track_one(scene["rgb"], depth, scene["K"], iteration=2)
        assert est.depth_agreement is None
        est.pose_last = start.clone()
        extra = {}
        got = est.track_one(scene["rgb"], depth, scene["K"], iteration=2, extra=extra, agreement_tol=0.01)
        assert np.array_equal(plain, got)
        want = ops.DepthAgreement.rows(_op(est.pose_last.reshape(1, 4, 4), _ingest(depth, scene["K"], dev), scene["K"],
                                           get_mesh_handle(est.mesh_tensors), est.diameter, 0.01)[0])[0]
        assert est.depth_agreement == want and extra["depth_agreement"] == want and want.model > 0
    est.pose_last = start.clone()
    est.track_one(scene["rgb"], scene["depth"], scene["K"], iteration=2)
    assert est.depth_agreement is None


def test_track_objects_and_views(scene, dev, meshes, stack):
    from foundationpose_amd import ops
    from foundationpose_amd.estimater import track_objects, track_views
    names = ("can", "torus", "box")
    ests = _estimators(meshes, names, dev)
    start = [_t(p[None], dev) for p in _poses(scene, len(ests), seed=81, max_trans=0.015, max_rot_deg=10)]

    def reset():
        for e, s in zip(ests, start):
            e.pose_last = s.clone()
    reset()
    plain = track_objects(ests, scene["rgb"], scene["depth"], scene["K"], iteration=2)
    assert all(e.depth_agreement is None for e in ests)
    reset()
    got = track_objects(ests, scene["rgb"], scene["depth"], scene["K"], iteration=2, agreement_tol=0.01)
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    P = torch.cat([e.pose_last for e in ests]).contiguous()
    want = _est_op(ests, P, _ingest(scene["depth"], scene["K"], dev), scene["K"], dev)
    assert [e.depth_agreement for e in ests] == want and want[0].agree > 0
    # several views
    views = [2, 0, 1]
    reset()
    plain = track_views(ests, views, stack["rgbs"], stack["depths"], stack["Ks"], iteration=2)
    assert all(e.depth_agreement is None for e in ests)
    reset()
    got = track_views(ests, views, stack["rgbs"], stack["depths"], stack["Ks"], iteration=2, agreement_tol=0.01)
    assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    P = torch.cat([e.pose_last for e in ests]).contiguous()
    vt = ops.Views(stack["Ks"], views, dev)
    xyz_v = ops.ingest_frames(torch.stack([torch.as_tensor(d, device=dev) for d in stack["depths"]]).contiguous(), vt)
    want = _est_op(ests, P, xyz_v, None, dev, views=vt)
    assert [e.depth_agreement for e in ests] == want and all(w.model > 0 for w in want)


def test_depth_agreement_after_register_objects(scene, dev, meshes, stack):
    from foundationpose_amd import estimater, ops
    from foundationpose_amd.estimater import register_objects
    ests = _estimators(meshes, ("can", "small_can"), dev)
    register_objects(ests, scene["K"], scene["rgb"], scene["depth"], [scene["mask"], scene["mask"]], iteration=1)
    got = estimater.depth_agreement(ests, scene["depth"], scene["K"])
    P = torch.stack([e.pose_last.reshape(4, 4) for e in ests]).contiguous()
    want = _est_op(ests, P, _ingest(scene["depth"], scene["K"], dev), scene["K"], dev)
    assert got == want and got[0].model > 0 and got[0].valid > 0
    # the view form: each estimator's pose on its own frame
    views = [1, 0]
    got = estimater.depth_agreement(ests, stack["depths"][:2], stack["Ks"][:2], views=views, tol=0.01)
    vt = ops.Views(stack["Ks"][:2], views, dev)
    xyz_v = ops.ingest_frames(torch.stack([torch.as_tensor(d, device=dev) for d in stack["depths"][:2]]).contiguous(), vt)
    assert got == _est_op(ests, P, xyz_v, None, dev, views=vt)
    with pytest.raises(ValueError, match="tolerance"):
        estimater.depth_agreement(ests, scene["depth"], scene["K"], tol=-0.01)
