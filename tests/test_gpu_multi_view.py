"""GPU: several camera frames per refine call -- a per-hypothesis view index from the kernels (the crop stage with a view table and the
batched ingest) up to estimater.track_views.  Every hypothesis of a multi-view call must see what a call on its own frame alone
computes: the kernels bit for bit against their host-K form called per view, the refine loop against per-view calls, the
graphed tracker against its eager loop, and the estimator against per-estimator track_one on its own frame."""
import numpy as np
import pytest
import torch

from test_gpu_multi_object import (_close, _diameter, _interleaved, _poses, _set, _t, _three_object_frame, _trained,  # noqa: F401
                                   dev, frame, gmeshes, meshes)

pytestmark = pytest.mark.gpu


def _Ks(scene):
    """three views with different K: the scene's own, another focal length, a shifted principal point"""
    K0 = np.asarray(scene["K"], dtype=np.float64)
    K1 = K0.copy()
    K1[0, 0] *= 1.13
    K1[1, 1] *= 1.13
    K2 = K0.copy()
    K2[0, 2] += 23.5
    K2[1, 2] -= 17.25
    return [K0, K1, K2]


@pytest.fixture(scope="module")
def stack(scene, dev):
    """three frames of one size: the scene and two perturbed copies (rgb noise, a depth offset), pre-processed per frame"""
    from foundationpose_amd import ops
    rng = np.random.default_rng(5)
    Ks = _Ks(scene)
    rgbs, depths = [], []
    for v in range(3):
        rgbs.append(np.clip(scene["rgb"].astype(np.float32) + (rng.normal(0, 6, scene["rgb"].shape) if v else 0), 0, 255).astype(np.uint8))
        depths.append((scene["depth"] + 0.003 * v).astype(np.float32))
    rgb_t = torch.stack([torch.as_tensor(r, device=dev).float() for r in rgbs]).contiguous()
    depth_raw = torch.stack([torch.as_tensor(d, device=dev) for d in depths]).contiguous()
    pre = [ops.bilateral_filter_depth(ops.erode_depth(depth_raw[v], radius=2), radius=2) for v in range(3)]
    depth_t = torch.stack(pre).contiguous()
    xyz_t = torch.stack([ops.depth_to_xyz(pre[v], Ks[v], zfar=float("inf"), f64_internal=False) for v in range(3)]).contiguous()
    return dict(Ks=Ks, rgbs=rgbs, depths=depths, rgb_t=rgb_t, depth_raw=depth_raw, depth_t=depth_t, xyz_t=xyz_t)


def _rows(idx, v):
    return np.nonzero(np.asarray(idx) == v)[0]


# ------------------------------------------------------------------ 1. per kernel against the host-K form per view
ALL_OUT = ("A", "color", "depth", "xyz", "zbuf", "tri_id")


@pytest.mark.parametrize("with_obj", [False, True], ids=["obj_null", "obj"])
def test_views_kernels_are_the_multi_kernels_per_view(scene, dev, meshes, gmeshes, stack, with_obj):
    from foundationpose_amd import ops
    names = ("can", "box", "torus", "small_can") if with_obj else ("can",)
    mset, _, diam = _set(names, meshes, gmeshes, dev)
    dt = ops.object_diameters(diam, dev)
    N = 48
    view = _interleaved(3, N, seed=11)
    obj = _interleaved(len(names), N, seed=12) if with_obj else np.zeros(N, np.int32)
    ot = _t(obj, dev) if with_obj else None
    vt = ops.Views(stack["Ks"], view, dev)
    P = _t(_poses(scene, N, seed=13, max_rot_deg=30), dev)
    tf, bb = ops.crop_windows(P, None, dt, 1.2, (160, 160), obj=ot, views=vt)
    r = ops.render_crops(mset, P, bb, None, 480, 640, (160, 160), dt, want=ALL_OUT, obj=ot, views=vt)
    Br = {nz: ops.warp_crops(stack["rgb_t"], stack["xyz_t"], None, tf, None, P, dt, ops.MODE_REFINE, normalize_xyz=nz, obj=ot, views=vt)
          for nz in (True, False)}
    Bs = ops.warp_crops(stack["rgb_t"], None, stack["depth_t"], tf, None, P, dt, ops.MODE_SCORE, obj=ot, views=vt)
    rng = np.random.default_rng(14)
    trans = _t(rng.normal(0, 0.5, (N, 3)).astype(np.float32), dev)
    rot = _t(rng.normal(0, 0.5, (N, 3)).astype(np.float32), dev)
    upd = {}
    for rep in ("tracknet", "deepim"):
        td, rd = torch.empty((N, 3), device=dev), torch.empty((N, 3, 3), device=dev)
        upd[rep] = (ops.pose_update(trans, rot, P, normalize_xyz=True, trans_normalizer=(0.2, 0.2, 0.2), rot_normalizer=0.35,
                                    mesh_diameter=dt, trans_delta_out=td, rot_delta_out=rd, trans_rep=rep, tf_to_crops=tf,
                                    input_w=160, obj=ot, views=vt), td, rd)
    for v in range(3):
        rows = _rows(view, v)
        rv = torch.as_tensor(rows, device=dev)
        Pv, K = P[rv].contiguous(), stack["Ks"][v]
        ov = _t(obj[rows], dev) if with_obj else None
        tfv, bbv = ops.crop_windows(Pv, K, dt, 1.2, (160, 160), obj=ov)
        assert torch.equal(tf[rv], tfv) and torch.equal(bb[rv], bbv), v
        rr = ops.render_crops(mset, Pv, bbv, K, 480, 640, (160, 160), dt, want=ALL_OUT, obj=ov)
        for k in ALL_OUT:
            assert torch.equal(r[k][rv], rr[k]), (v, k)
        for nz in (True, False):
            ref = ops.warp_crops(stack["rgb_t"][v], stack["xyz_t"][v], None, tfv, K, Pv, dt, ops.MODE_REFINE, normalize_xyz=nz, obj=ov)
            assert torch.equal(Br[nz][rv], ref), (v, nz)
        ref = ops.warp_crops(stack["rgb_t"][v], None, stack["depth_t"][v], tfv, K, Pv, dt, ops.MODE_SCORE, obj=ov)
        assert torch.equal(Bs[rv], ref), v
        for rep in ("tracknet", "deepim"):
            td, rd = torch.empty((len(rows), 3), device=dev), torch.empty((len(rows), 3, 3), device=dev)
            o = ops.pose_update(trans[rv].contiguous(), rot[rv].contiguous(), Pv, normalize_xyz=True, trans_normalizer=(0.2, 0.2, 0.2),
                                rot_normalizer=0.35, mesh_diameter=dt, trans_delta_out=td, rot_delta_out=rd, trans_rep=rep, K=K,
                                tf_to_crops=tfv, input_w=160, obj=ov)
            assert torch.equal(upd[rep][0][rv], o) and torch.equal(upd[rep][1][rv], td) and torch.equal(upd[rep][2][rv], rd), (v, rep)
    # the views matter: the same hypotheses all in view 0 give other windows
    tf0, _ = ops.crop_windows(P, stack["Ks"][0], dt, 1.2, (160, 160), obj=ot if with_obj else None)
    assert not torch.equal(tf, tf0)


# ------------------------------------------------------------------ 2. the batched ingest
def test_frames_ingest_is_the_per_frame_ingest(dev, stack):
    from foundationpose_amd import ops
    vt = ops.Views(stack["Ks"], [0, 1, 2], dev)
    er = ops.erode_depth_frames(stack["depth_raw"], radius=2)
    bl = ops.bilateral_filter_depth_frames(er, radius=2)
    for v in range(3):
        e1 = ops.erode_depth(stack["depth_raw"][v].contiguous(), radius=2)
        assert torch.equal(er[v], e1), v
        assert torch.equal(bl[v], ops.bilateral_filter_depth(e1, radius=2)), v
    for f64 in (False, True):
        xyz = ops.depth_to_xyz_frames(bl, vt, zfar=float("inf"), f64_internal=f64)
        for v in range(3):
            assert torch.equal(xyz[v], ops.depth_to_xyz(bl[v].contiguous(), stack["Ks"][v], zfar=float("inf"), f64_internal=f64)), (v, f64)
    assert torch.equal(ops.ingest_frames(stack["depth_raw"], vt), stack["xyz_t"])


# ------------------------------------------------------------------ 3. / 4. the refine loop against per-view calls
def _views_vs_single(pred, scene, stack, dev, meshes, gmeshes, names, obj, view, P, iteration=2, same_size=False, first=False):
    """-> (one multi-view refine call, per-view calls) as poses, or with first=True the first network input (2N, 6, h, w).
    same_size: every per-view call refines ALL of P (rows kept in place) with that view's frame and K and contributes its rows"""
    from foundationpose_amd import ops
    from foundationpose_amd.crops import Scene
    from foundationpose_amd.predict_pose_refine import ObjectIndex
    mset, _, diam = _set(names, meshes, gmeshes, dev)
    dt = ops.object_diameters(diam, dev)
    Pt, N = _t(P, dev), len(P)
    vt = ops.Views(stack["Ks"], view, dev)
    oi = ObjectIndex(obj, dev, view=view) if obj is not None else None
    if first:
        st = pred.refine_part(0, (0, N), stack["rgb_t"], stack["xyz_t"], Pt, Scene(mset, dt, None, 480, 640, N, obj=oi, views=vt), range(1),
                              pred.alloc_outputs(N, dev) + (1,))
        multi = st["AB"].clone()
    else:
        multi = pred.refine_device(stack["rgb_t"], stack["xyz_t"], Pt, None, 480, 640, mset, dt, iteration, obj=oi, views=vt)[0]
    single = torch.empty_like(multi)
    for v in range(3):
        rows = _rows(view, v)
        if not len(rows):
            continue
        r = torch.as_tensor(rows, device=dev)
        sel = np.arange(N) if same_size else rows
        ov = None if obj is None else ObjectIndex(np.asarray(obj)[sel], dev)
        Pv = Pt[torch.as_tensor(sel, device=dev)].contiguous()
        args = (stack["rgb_t"][v], stack["xyz_t"][v], Pv, stack["Ks"][v], 480, 640, mset, dt)
        if first:
            n = len(sel)
            sk = pred.refine_part(0, (0, n), *args[:3], Scene(mset, dt, stack["Ks"][v], 480, 640, n, obj=ov), range(1),
                                  pred.alloc_outputs(n, dev) + (1,))
            single[r], single[r + N] = sk["AB"][:n], sk["AB"][n:]
        else:
            out = pred.refine_device(*args, iteration, obj=ov)[0]
            single[r] = out[r] if same_size else out
    return multi, single


@pytest.mark.parametrize("with_obj", [False, True], ids=["obj_null", "obj"])
def test_refine_loop_three_views_is_per_view_calls_on_the_large_call_kernels(scene, dev, meshes, gmeshes, stack, with_obj):
    from foundationpose_amd import engine
    names = ("can", "torus", "box") if with_obj else ("can",)
    # no group of exactly two rows, neither per (view, object) nor per object: the two-pose quirk (test below) stays out of this
    # comparison, whose same-size per-view calls refine all seven poses
    view = [2, 0, 1, 0, 2, 0, 2]
    obj = [0, 0, 0, 0, 1, 0, 2] if with_obj else None
    with engine.overrides(SPLITK_MAX_HYPS=0, HEADS_TWO_STREAMS_MAX_HYPS=0):
        pred = _trained(dev)
        P = _poses(scene, len(view), seed=21, max_rot_deg=20)
        a, b = _views_vs_single(pred, scene, stack, dev, meshes, gmeshes, names, obj, view, P, same_size=True)
        assert torch.equal(a, b), (a - b).abs().max()
        a1, b1 = _views_vs_single(pred, scene, stack, dev, meshes, gmeshes, names, obj, view, P, first=True)
        assert torch.equal(a1, b1)
        # against one-hypothesis calls per (view, object): the small-call gates
        one = torch.empty_like(a)
        from foundationpose_amd import ops
        mset, _, diam = _set(names, meshes, gmeshes, dev)
        dt = ops.object_diameters(diam, dev)
        from foundationpose_amd.predict_pose_refine import ObjectIndex
        for n in range(len(view)):
            v = view[n]
            one[n] = pred.refine_device(stack["rgb_t"][v], stack["xyz_t"][v], _t(P[n:n + 1], dev), stack["Ks"][v], 480, 640, mset, dt, 2,
                                        obj=ObjectIndex([0 if obj is None else obj[n]], dev))[0][0]
        ok, err = _close(a, one)
        assert ok, err
    assert not torch.equal(a, _t(P, dev))


def test_one_object_in_two_views_is_not_the_two_pose_quirk(scene, dev, meshes, gmeshes, stack):
    """one object with one hypothesis in each of two views = two one-pose calls: the quirk must not pair them (a per-object grouping
    would); one view with two hypotheses keeps it"""
    from foundationpose_amd import engine
    with engine.overrides(SPLITK_MAX_HYPS=0, HEADS_TWO_STREAMS_MAX_HYPS=0):
        pred = _trained(dev)
        P = _poses(scene, 2, seed=31, max_rot_deg=20)
        P[1, :3, 3] += [0.02, -0.01, 0.03]
        for obj in (None, [0, 0]):
            a, b = _views_vs_single(pred, scene, stack, dev, meshes, gmeshes, ("can",), obj, [0, 1], P, first=True)
            assert torch.equal(a, b), obj
        # the naive grouping (by object only) would render both with the paired window: the crops differ from the correct ones
        from foundationpose_amd import ops
        from foundationpose_amd.predict_pose_refine import ObjectIndex
        mset, _, diam = _set(("can",), meshes, gmeshes, dev)
        from foundationpose_amd.crops import Scene
        naive = pred.refine_part(0, (0, 2), stack["rgb_t"][0], stack["xyz_t"][0], _t(P, dev),
                                 Scene(mset, ops.object_diameters(diam, dev), stack["Ks"][0], 480, 640, 2, obj=ObjectIndex([0, 0], dev)),
                                 range(1), pred.alloc_outputs(2, dev) + (1,))["AB"]
        assert not torch.equal(a[:1], naive[:1])
        # one view, two hypotheses: the quirk applies as in the single-view call
        a, b = _views_vs_single(pred, scene, stack, dev, meshes, gmeshes, ("can",), None, [1, 1], P, first=True)
        assert torch.equal(a, b)
        assert ops.Views(stack["Ks"], [1, 1], dev).pairs == [(0, 1)]


# ------------------------------------------------------------------ 5. the graphed tracker
@pytest.mark.parametrize("n_hyp", [1, 2])
def test_views_tracker_graph_is_eager(scene, dev, meshes, gmeshes, stack, n_hyp):
    from foundationpose_amd.graphs import FramePipeline, GraphedTracker
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    from foundationpose_amd.weights import CONTRACTION_HEAD_SCALE, DEFAULT_REFINE_CFG, random_state_dict
    refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), device=dev,
                                  state_dict=random_state_dict("refine", seed=0, head_scale=CONTRACTION_HEAD_SCALE))
    names = ("can", "torus", "can", "box")
    views = [2, 0, 1, 0]
    trk = GraphedTracker(refiner, [gmeshes[k] for k in names], [_diameter(meshes[k]) for k in names], stack["Ks"], 480, 640,
                         n_hyp=n_hyp, iteration=2, device=dev, views=views).capture()
    assert trk.N == 4 * n_hyp and trk.rgb.shape == (3, 480, 640, 3)
    assert len(trk.obj.pairs) == (4 if n_hyp == 2 else 0)
    eager, graphed = [], []
    for f in range(3):
        P = _poses(scene, trk.N, seed=41 + f, max_rot_deg=20)
        if n_hyp == 2:
            P[1::2, :3, 3] += [0.01, -0.01, 0.02]
        rgbs = [np.roll(r, 3 * f, axis=1) for r in stack["rgbs"]]
        depths = [d + 0.001 * f for d in stack["depths"]]
        eager.append(trk.step_eager(rgbs, depths, P).clone())
        graphed.append(trk.step(np.stack(rgbs), np.stack(depths), P).clone())    # a stacked array is accepted too
    assert all(torch.equal(a, b) for a, b in zip(eager, graphed))
    assert not torch.equal(graphed[0], graphed[1])
    with pytest.raises(ValueError, match="pipelining views"):
        FramePipeline(trk)


# ------------------------------------------------------------------ 6. the estimator
def test_track_views_is_per_estimator_track_one(scene, dev, meshes, stack):
    """two cameras with different K see the can and the box (each pose in its own camera's frame); four estimators -- the can
    and the box in each camera, two pairs sharing a mesh -- tracked with track_views against track_one on the own frame.  One
    batched call of four hypotheses against one-hypothesis calls: the kernel choice described before
    test_gpu_multi_object.py::test_refine_loop_three_objects..., so those poses are gated; against same-size calls on each camera's
    frame (a views-free tracker over the same four meshes) the result is bit for bit"""
    from foundationpose_amd import engine
    from foundationpose_amd.estimater import FoundationPose, track_views
    from foundationpose_amd.graphs import FramePipeline
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    from foundationpose_amd.predict_score import ScorePredictor
    from foundationpose_amd.weights import DEFAULT_REFINE_CFG, DEFAULT_SCORE_CFG, random_state_dict, trained_refiner_state_dict
    names = ("can", "box")
    Ks = [stack["Ks"][0], stack["Ks"][1]]
    gt = []                       # gt[c][k]: object k in camera c
    for c in range(2):
        g = np.stack([scene["gt"].copy() for _ in names])
        g[0, 0, 3] += -0.05 + 0.02 * c
        g[1, 0, 3] += 0.06 - 0.01 * c
        g[1, 2, 3] += 0.02
        g[1, :3, :3] = _poses(scene, 1, seed=91 + c, max_rot_deg=50)[0, :3, :3]
        gt.append(g)
    frames, starts = [], []
    for f in range(3):
        fr, st = [], []
        for c in range(2):
            P = gt[c].copy()
            P[:, 0, 3] += 0.002 * f
            sc = dict(scene, K=Ks[c])
            fr.append(_three_object_frame(sc, meshes, names, P))
            S = P.copy()
            S[:, :3, 3] += [0.004, -0.003, 0.006]
            st.append(S)
        frames.append(fr)
        starts.append(st)
    est_view = [0, 0, 1, 1]
    est_obj = [0, 1, 0, 1]
    with engine.overrides(SPLITK_MAX_HYPS=0, HEADS_TWO_STREAMS_MAX_HYPS=0):
        refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
        scorer = ScorePredictor(cfg=dict(DEFAULT_SCORE_CFG), state_dict=random_state_dict("score", seed=0), device=dev)
        ests = [FoundationPose(model_pts=meshes[names[k]].vertices, model_normals=meshes[names[k]].vertex_normals,
                               mesh=meshes[names[k]], scorer=scorer, refiner=refiner, device=dev) for k in est_obj]
        rgbs0, depths0 = [frames[0][c][0] for c in range(2)], [frames[0][c][1] for c in range(2)]
        with pytest.raises(RuntimeError, match="not registered"):
            track_views(ests, est_view, rgbs0, depths0, Ks)

        def reset(f):
            for e, c, k in zip(ests, est_view, est_obj):
                e.pose_last = torch.as_tensor(starts[f][c][k], device=dev, dtype=torch.float).reshape(1, 4, 4)
        one, many = [], []
        for f in range(len(frames)):
            rgbs, depths = [frames[f][c][0] for c in range(2)], [frames[f][c][1] for c in range(2)]
            reset(f)
            one.append(np.stack([e.track_one(rgbs[c], depths[c], Ks[c], iteration=2) for e, c in zip(ests, est_view)]))
            last = [e.pose_last.clone() for e in ests]
            reset(f)
            many.append(np.stack(track_views(ests, est_view, rgbs, depths, Ks, iteration=2)))
        trk = refiner._views_tracker[1]
        assert trk.N == 4 and trk.V == 2
        # translation within the small-call gate (1e-4 m).  Rotation: measured up to 5.2e-4 rad on frame 0 at translation gaps of
        # 2e-6 m -- last-place differences of the one-hypothesis kernels, amplified by two iterations of the untrained box's updates --
        # so the bound is 1e-3 rad here; the bit-exact check below is what pins the multi-view path down
        from amp_util import geodesic
        for f in range(len(frames)):
            dR = geodesic(many[f][:, :3, :3], one[f][:, :3, :3])
            dt = np.linalg.norm(many[f][:, :3, 3].astype(np.float64) - one[f][:, :3, 3].astype(np.float64), axis=1)
            assert dt.max() <= 1e-4 and dR.max() <= 1e-3, (f, dt, dR)
        from foundationpose_amd.graphs import GraphedTracker
        reset(len(frames) - 1)
        track_views(ests, est_view, [frames[-1][c][0] for c in range(2)], [frames[-1][c][1] for c in range(2)], Ks, iteration=2)
        got = torch.stack([e.pose_last[0] for e in ests])
        for c in range(2):
            same = GraphedTracker(refiner, [e.mesh_tensors for e in ests], [e.diameter for e in ests], Ks[c], 480, 640, n_hyp=1,
                                  iteration=2, device=dev).capture()
            start = torch.as_tensor(np.stack([starts[-1][cv][k] for cv, k in zip(est_view, est_obj)]), device=dev, dtype=torch.float)
            ref = same.step(frames[-1][c][0], frames[-1][c][1], start)
            rows = [k for k in range(4) if est_view[k] == c]
            assert torch.equal(got[rows], ref[rows]), c
        for e, p, m in zip(ests, last, many[-1]):
            assert e.pose_last.shape == (1, 4, 4) and _close(e.pose_last, p)[0]
            assert torch.equal((e.pose_last[0] @ e.get_tf_to_centered_mesh()).cpu(), torch.as_tensor(m))
        # the can, tracked in each camera's own frame
        for c in range(2):
            assert np.abs(many[-1][2 * c, :3, 3] - gt[c][0, :3, 3]).max() < 0.01, c
        # the refusals
        with pytest.raises(ValueError, match="outside 0..1"):
            track_views(ests, [0, 0, 1, 2], rgbs0, depths0, Ks)
        with pytest.raises(ValueError, match="listed twice"):
            track_views([ests[0], ests[0]], [0, 1], rgbs0, depths0, Ks)
        with pytest.raises(ValueError, match="one H x W"):
            track_views(ests, est_view, [rgbs0[0], rgbs0[1][:240]], [depths0[0], depths0[1][:240]], Ks)
        other = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
        stranger = FoundationPose(model_pts=meshes["can"].vertices, model_normals=meshes["can"].vertex_normals, mesh=meshes["can"],
                                  scorer=scorer, refiner=other, device=dev)
        stranger.pose_last = ests[0].pose_last.clone()
        with pytest.raises(ValueError, match="share one refiner"):
            track_views(ests[:1] + [stranger], [0, 1], rgbs0, depths0, Ks)
        with pytest.raises(ValueError, match="pipelining views"):
            FramePipeline(trk)


# ------------------------------------------------------------------ 7. a view index outside 0..V-1
@pytest.mark.parametrize("with_obj", [False, True], ids=["obj_null", "obj"])
def test_view_index_outside_the_table(scene, dev, meshes, gmeshes, stack, with_obj):
    """the kernels guard the index: nothing is read outside the stack or the table; the render draws nothing, the warp writes what a
    pixel outside the frame gets, crop windows and pose update give NaN.  (The obj form documents the same convention: an object
    index outside 0..M-1 draws nothing.)"""
    from foundationpose_amd import ops
    names = ("can", "box") if with_obj else ("can",)
    mset, _, diam = _set(names, meshes, gmeshes, dev)
    dt = ops.object_diameters(diam, dev)
    N = 6
    view = np.array([0, 1, 2, 0, 1, 2], np.int32)
    obj = np.array([0, 1, 0, 1, 0, 1], np.int32) if with_obj else np.zeros(N, np.int32)
    ot = _t(obj, dev) if with_obj else None
    vt = ops.Views(stack["Ks"], view, dev)
    P = _t(_poses(scene, N, seed=71, max_rot_deg=20), dev)
    tf, bb = ops.crop_windows(P, None, dt, 1.2, (160, 160), obj=ot, views=vt)
    bad = [1, 4]
    vt.dev[bad[0]] = 3          # one past the end
    vt.dev[bad[1]] = -7
    tfb, bbb = ops.crop_windows(P, None, dt, 1.2, (160, 160), obj=ot, views=vt)
    good = [0, 2, 3, 5]
    assert torch.equal(tfb[good], tf[good]) and torch.isnan(tfb[bad]).any(dim=(1, 2)).all() and torch.isnan(bbb[bad]).all()
    r = ops.render_crops(mset, P, bb, None, 480, 640, (160, 160), dt, want=ALL_OUT, obj=ot, views=vt)
    assert (r["tri_id"][bad] == -1).all() and (r["zbuf"][bad].view(torch.int32) == -1).all()
    assert (r["color"][bad] == 0).all() and (r["depth"][bad] == 0).all()
    assert (r["tri_id"][good] >= 0).any(dim=(1, 2)).all()
    # warp: every pixel of a bad row = a pixel outside the frame (a window far off the frame, in a good view, gives the reference)
    far = tf.clone()
    far[:, 0, 2] -= 1e5
    far[:, 1, 2] -= 1e5
    for mode, a, b in ((ops.MODE_REFINE, stack["xyz_t"], None), (ops.MODE_SCORE, None, stack["depth_t"])):
        Bb = ops.warp_crops(stack["rgb_t"], a, b, tf, None, P, dt, mode, obj=ot, views=vt)
        ok = ops.Views(stack["Ks"], np.zeros(N, np.int32), dev)
        Bf = ops.warp_crops(stack["rgb_t"], a, b, far, None, P, dt, mode, obj=ot, views=ok)
        assert torch.equal(Bb[bad], Bf[bad]), mode
        assert (Bb[bad][:, :3] == 0).all()
    td, rd = torch.empty((N, 3), device=dev), torch.empty((N, 3, 3), device=dev)
    rng = np.random.default_rng(72)
    trans = _t(rng.normal(0, 0.5, (N, 3)).astype(np.float32), dev)
    rot = _t(rng.normal(0, 0.5, (N, 3)).astype(np.float32), dev)
    for rep in ("tracknet", "deepim"):
        o = ops.pose_update(trans, rot, P, normalize_xyz=True, trans_normalizer=(0.2, 0.2, 0.2), rot_normalizer=0.35, mesh_diameter=dt,
                            trans_delta_out=td, rot_delta_out=rd, trans_rep=rep, tf_to_crops=tf, input_w=160, obj=ot, views=vt)
        assert torch.isnan(o[bad]).all() and torch.isnan(td[bad]).all() and torch.isnan(rd[bad]).all(), rep
        assert not torch.isnan(o[good]).any(), rep
