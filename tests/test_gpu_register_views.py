"""GPU: registering objects in several camera streams in one call -- the mask statistics of the translation guess
(fp_mask_depth_stats), the segmented shared observed crop (fp_replicate_segments_f16, the plan's segmented shared_b, refine_device with
shared_translation=<Segments>), the scorer over several views, and estimater.register_views against per-estimator register() on its
own frame."""
import types

import numpy as np
import pytest
import torch

from test_gpu_multi_object import _close, _diameter, _poses, _set, _trained, dev, gmeshes, meshes  # noqa: F401
from test_gpu_multi_view import _Ks, stack  # noqa: F401
from test_gpu_register_objects import _frame, _scorer, _state, _zrot, objects  # noqa: F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the mask statistics
def _ref_stats(d, m):
    """guess_translation's statistics with torch: box, valid count, the two middle elements of torch.sort"""
    mm = m > 0
    rows, cols = torch.nonzero(mm.any(dim=1)).reshape(-1), torch.nonzero(mm.any(dim=0)).reshape(-1)
    box = [-1] * 4 if rows.numel() == 0 else [int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])]
    z = torch.sort(d[mm & (d >= 0.001)]).values
    n = int(z.numel())
    lo, hi = (np.float32(np.nan),) * 2 if n == 0 else (z[(n - 1) // 2].cpu().numpy(), z[n // 2].cpu().numpy())
    return box, n, np.float32(lo), np.float32(hi)


def _mask_cases(depths, rng):
    """(view, mask) pairs: empty, no valid depth, 1 / 2 / 3 / 4 valid depths, odd and even counts, ties at the median, the frame
    border, full frames"""
    V, H, W = depths.shape
    out = []

    def pick(v, k_valid, k_invalid):
        d = depths[v]
        valid, invalid = np.argwhere(d >= np.float32(0.001)), np.argwhere(~(d >= np.float32(0.001)))
        m = np.zeros((H, W), np.uint8)
        for arr, k in ((valid, k_valid), (invalid, k_invalid)):
            for r, c in arr[rng.choice(len(arr), k, replace=False)]:
                m[r, c] = 1 + rng.integers(0, 200)          # any nonzero value is inside
        return m
    out.append((0, np.zeros((H, W), np.uint8)))
    out.append((1, pick(1, 0, 9)))
    for k, v in ((1, 2), (2, 0), (3, 1), (4, 2)):
        out.append((v, pick(v, k, 3)))
    out.append((0, pick(0, 101, 20)))                        # odd count
    out.append((1, pick(1, 250, 20)))                        # even count
    m = np.zeros((H, W), np.uint8)
    m[5:15, 10:30] = 1                                       # frame 2 holds a flat patch here: ties at the median
    out.append((2, m))
    m = np.zeros((H, W), np.uint8)
    m[0, 3] = m[H - 1, 5] = m[7, 0] = m[9, W - 1] = 1
    m[H - 4:, W - 6:] = 1
    out.append((0, m))
    out.append((1, np.ones((H, W), np.uint8)))
    out.append((2, np.full((H, W), 255, np.uint8)))
    return out


def _depth_stack(V, H, W, rng):
    d = np.round(rng.uniform(0.3, 2.0, (V, H, W)), 2).astype(np.float32)      # two decimals: many ties
    d[rng.random((V, H, W)) < 0.1] = 0.0
    d[rng.random((V, H, W)) < 0.05] = -0.5
    d[rng.random((V, H, W)) < 0.01] = np.nan
    d[0, 1, 1] = np.inf
    d[2, 5:15, 10:30] = 0.75
    d[2, 5:7, 10:30] = 0.70
    return d


@pytest.mark.parametrize("hw", [(48, 64), (37, 53)], ids=["four_pixel_loads", "odd_size"])
def test_mask_depth_stats_is_the_sort(dev, hw):
    from foundationpose_amd import ops
    from foundationpose_amd.estimater import FoundationPose, translation_from_stats
    rng = np.random.default_rng(21)
    H, W = hw
    depths = _depth_stack(3, H, W, rng)
    cases = _mask_cases(depths, rng)
    assert len(cases) == 12
    d_t = torch.as_tensor(depths, device=dev)
    mk = torch.as_tensor(np.stack([m for _, m in cases]), device=dev)
    vw = torch.as_tensor(np.asarray([v for v, _ in cases], np.int32), device=dev)
    box, n, lo, hi = ops.mask_depth_stats_host(ops.mask_depth_stats(d_t, mk, vw))       # one launch for all twelve masks
    Ks = _Ks(dict(K=np.array([[572.4, 0, 25.1], [0, 573.6, 19.4], [0, 0, 1]])))
    stub = types.SimpleNamespace(device=dev)
    seen = set()
    for i, (v, m) in enumerate(cases):
        rb, rn, rlo, rhi = _ref_stats(d_t[v], torch.as_tensor(m, device=dev))
        assert list(box[i]) == rb and n[i] == rn, (i, box[i], rb, n[i], rn)
        if rn == 0:
            assert np.isnan(lo[i]) and np.isnan(hi[i])
        else:
            assert lo[i].view(np.int32) == rlo.view(np.int32) and hi[i].view(np.int32) == rhi.view(np.int32), (i, lo[i], rlo, hi[i], rhi)
        seen.add(min(rn, 5) if rn < 5 else 5 + rn % 2)
        # the centre built from the statistics is guess_translation's, bit for bit
        K = Ks[v]
        ref = FoundationPose.guess_translation(stub, depth=d_t[v], mask=m, K=K)
        got = translation_from_stats(K, box[i], n[i], lo[i], hi[i])
        assert np.array_equal(got, ref), (i, got, ref)
    assert seen == {0, 1, 2, 3, 4, 5, 6}                     # 0..4 valid depths, odd and even counts
    # one frame needs no view index
    one = ops.mask_depth_stats(d_t[:1].contiguous(), mk[:3].contiguous())
    assert torch.equal(one, ops.mask_depth_stats(d_t, mk[:3].contiguous(), torch.zeros(3, dtype=torch.int32, device=dev)))


# ------------------------------------------------------------------ 2. the segmented replication
def _ref_replicate(buf, lengths, c0, c1):
    ref = buf.clone()
    off = np.concatenate([[0], np.cumsum(lengths)])
    for s in range(len(lengths)):
        ref[off[s]:off[s + 1], :, :, c0:c1] = buf[s, :, :, c0:c1]
    return ref


def test_replicate_segments_is_the_reference_copy(dev):
    from foundationpose_amd import ops
    rng = np.random.default_rng(3)
    many = list(rng.integers(1, 6, 64))
    many[0] = many[5] = many[63] = 1                         # one-row segments, including the first and the last
    for lengths, c0, c1 in (([7], 128, 256), (many, 128, 256), ([3, 1, 40, 2, 1], 8, 72), ([1, 1, 1], 0, 256)):
        n = int(np.sum(lengths))
        buf = torch.randn((n, 12, 10, 256), generator=torch.Generator().manual_seed(n)).to(torch.float16).to(dev)
        ref = _ref_replicate(buf, lengths, c0, c1)
        seg = ops.Segments(lengths, dev)
        got = ops.replicate_segments(buf.clone(), seg, c0, c1)
        assert torch.equal(got, ref), (len(lengths), c0, c1)
    with pytest.raises(Exception, match="at least one image"):
        ops.replicate_segments(buf.clone(), ops.Segments([2, 0, 1], dev), 0, 256)
    # graph replay gives the same bits (captured in inference mode, as the predictors capture their loops)
    lengths = [5, 1, 17, 2]
    seg = ops.Segments(lengths, dev)
    src = torch.randn((25, 12, 10, 256), generator=torch.Generator().manual_seed(9)).to(torch.float16).to(dev)
    with torch.inference_mode():
        static = src.clone()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            ops.replicate_segments(static, seg, 128, 256)       # warm-up outside the capture
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.replicate_segments(static, seg, 128, 256)
        static.copy_(src)
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(static, _ref_replicate(src, lengths, 128, 256))


# ------------------------------------------------------------------ 3. the plan with the segmented shared_b
@pytest.mark.parametrize("lengths", [[17, 1, 2, 20], [3, 1, 2]], ids=["large_call", "small_call"])
def test_plan_segmented_shared_b_is_the_expanded_plan(dev, lengths):
    from foundationpose_amd import ops
    pred = _trained(dev)
    plan = pred.plan()
    oh, ow, _, _ = pred._loop_constants()
    n, S = int(np.sum(lengths)), len(lengths)
    g = torch.Generator().manual_seed(n)
    A = torch.rand((n, 6, oh, ow), generator=g).to(torch.float16).to(dev)
    B = torch.rand((S, 6, oh, ow), generator=g).to(torch.float16).to(dev)
    idx = torch.as_tensor(np.repeat(np.arange(S), lengths), device=dev)
    raw_seg = {k: v.clone() for k, v in plan(torch.cat([A, B]).contiguous(), slot=0, shared_b=ops.Segments(lengths, dev)).items()}
    raw_exp = {k: v.clone() for k, v in plan(torch.cat([A, B[idx]]).contiguous(), slot=0).items()}
    for k in ("trans", "rot"):
        assert torch.equal(raw_seg[k], raw_exp[k]), (k, (raw_seg[k] - raw_exp[k]).abs().max())
    with pytest.raises(ValueError, match="segments cover"):
        plan(torch.cat([A, B]).contiguous(), slot=0, shared_b=ops.Segments(lengths[:-1] + [lengths[-1] + 1], dev))


# ------------------------------------------------------------------ 4. refine_device with one translation per segment
def _segment_hyps(scene, lengths, seed):
    P = []
    for k, L in enumerate(lengths):
        p = _poses(scene, L, seed=seed + k, max_trans=0.03, max_rot_deg=90)
        p[:, :3, 3] = p[0, :3, 3]
        P.append(p)
    return np.concatenate(P)


@pytest.mark.parametrize("n_streams", [1, 2])
@pytest.mark.parametrize("case", ["obj", "views_obj", "views"])
def test_refine_device_segmented_shared_translation_is_unshared(scene, dev, meshes, gmeshes, stack, n_streams, case):
    from foundationpose_amd import ops
    from foundationpose_amd.predict_pose_refine import ObjectIndex
    pred = _trained(dev, n_streams=n_streams)
    lengths_all = ([40, 2, 45], [43, 45]) if case != "views" else ([30, 2, 40],)
    for lengths in lengths_all:
        N, S = int(np.sum(lengths)), len(lengths)
        seg_view = [0, 2, 1][:S] if case != "views" else [1, 0, 2]
        names = ("can", "box", "can")[:S] if case != "views" else ("can",)
        mset, _, diam = _set(names, meshes, gmeshes, dev)
        dt = ops.object_diameters(diam, dev)
        P = torch.as_tensor(_segment_hyps(scene, lengths, seed=200 + N), device=dev)
        hv = np.repeat(seg_view, lengths)
        obj = np.repeat(np.arange(S), lengths)
        if case == "obj":
            args = (stack["rgb_t"][0], stack["xyz_t"][0], P, stack["Ks"][0], 480, 640, mset, dt, 2)
            kw = dict(obj=ObjectIndex(obj, dev))
        else:
            vt = ops.Views(stack["Ks"], hv, dev)
            args = (stack["rgb_t"], stack["xyz_t"], P, None, 480, 640, mset, dt, 2)
            kw = dict(views=vt, obj=ObjectIndex(obj, dev, view=hv) if case == "views_obj" else None)
        parts = pred.sub.parts(N, dev)
        got = [t.clone() for t in pred.refine_device(*args, shared_translation=ops.Segments(lengths, dev), **kw)]
        ref = pred.refine_device(*args, shared_translation=False, **kw)
        for g, r in zip(got, ref):
            assert torch.equal(g, r), (case, lengths, parts, (g - r).abs().max())


# ------------------------------------------------------------------ 5. the scorer over several views
def test_predict_objects_views_is_per_view_predict_objects(scene, dev, meshes, gmeshes, stack):
    from foundationpose_amd import ops
    names = ("can", "box", "torus", "can")
    view = [0, 1, 0, 2]
    counts = [40, 36, 33, 34]
    mset, _, diam = _set(names, meshes, gmeshes, dev)
    dt = ops.object_diameters(diam, dev)
    P = [_poses(scene, n, seed=80 + k, max_trans=0.03, max_rot_deg=90) for k, n in enumerate(counts)]
    seg = ops.Segments(counts, dev)
    vt = ops.Views(stack["Ks"], np.repeat(view, counts), dev)
    pred = _scorer(dev)
    got = pred.predict_objects(stack["rgb_t"], stack["depth_t"], None, np.concatenate(P), mset, dt, seg, views=vt)
    for v in range(3):
        ks = [k for k in range(len(names)) if view[k] == v]
        mv, _, dv = _set([names[k] for k in ks], meshes, gmeshes, dev)
        sv = ops.Segments([counts[k] for k in ks], dev)
        ref = pred.predict_objects(stack["rgb_t"][v], stack["depth_t"][v], stack["Ks"][v], np.concatenate([P[k] for k in ks]), mv,
                                   ops.object_diameters(dv, dev), sv)
        for j, k in enumerate(ks):
            a, b = seg.rows(k)
            ra, rb = sv.rows(j)
            assert torch.equal(got[a:b], ref[ra:rb]), (k, (got[a:b] - ref[ra:rb]).abs().max())
    with pytest.raises(ValueError, match="views need"):
        pred.predict_objects(stack["rgb_t"][0], stack["depth_t"][0], None, np.concatenate(P), mset, dt, seg, views=vt)


# ------------------------------------------------------------------ 6. the estimator
# Score tolerance of an estimator of 10 hypotheses (the encoder's split-K small-call path in its own register() call, the large-call
# kernels inside the batched call), as in test_gpu_register_objects.py: measured on MI355X with the seeded random-weight scorer below
# on this scene (camera 2, the vcol can, 2 refine iterations), largest |score difference| 3.19 with the same best hypothesis and poses
# 1.1e-5 m / 1.4e-4 rad apart.
SMALL_SCORE_TOL = 4.0


def _check(batched, ref, small=()):
    for k, ((p, st), (rp, rst)) in enumerate(zip(batched, ref)):
        if k in small:
            ok, err = _close(torch.as_tensor(p), torch.as_tensor(rp))
            dscore = (st["scores"] - rst["scores"]).abs().max().item()
            print(f"small estimator {k}: pose |dt| {err[0]:.3g} m, |dR| {err[1]:.3g} rad, |d score| max {dscore:.3g}, best id "
                  f"{st['best_id']} / {rst['best_id']}")
            assert ok, (k, err)
            assert st["best_id"] == rst["best_id"]
            assert dscore <= SMALL_SCORE_TOL
            continue
        assert np.array_equal(p, rp), (k, np.abs(p - rp).max())
        if rst is None:
            assert st is None
            continue
        for key in ("H", "W", "ob_id", "best_id"):
            assert st[key] == rst[key], (k, key)
        for key in ("K", "ob_mask"):
            assert np.array_equal(st[key], rst[key]), (k, key)
        for key in ("pose_last", "poses", "scores"):
            assert torch.equal(st[key], rst[key]), (k, key, (st[key] - rst[key]).abs().max())


def test_register_views_is_per_estimator_register(scene, dev, objects):
    """three cameras with different K; camera 0 sees the box and the torus, camera 1 the vcol can and the box (one object in two
    cameras: two estimators on one mesh), camera 2 the vcol can.  Identity symmetry: 252 hypotheses, two-fold: 126, four-fold: 50.
    Then an empty mask and a mask of fewer than 4 valid depths, an estimator cut to 10 hypotheses, and track_views right after"""
    from amp_util import geodesic
    from foundationpose_amd import engine
    from foundationpose_amd.estimater import FoundationPose, register_views, track_views
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    from foundationpose_amd.weights import DEFAULT_REFINE_CFG, trained_refiner_state_dict
    Ks = _Ks(scene)
    cams = [("box", "torus"), ("vcol", "box"), ("vcol",)]
    rgbs, depths, cam_masks = [], [], []
    for c, names in enumerate(cams):
        gt = np.stack([scene["gt"].copy() for _ in names])
        for k in range(len(names)):
            gt[k, 0, 3] += (-0.07 + 0.14 * k) + 0.01 * c
            gt[k, 2, 3] += 0.02 * c
            if k or c:
                gt[k, :3, :3] = _poses(scene, 1, seed=95 + 3 * c + k, max_rot_deg=50)[0, :3, :3]
        rgb, depth, masks = _frame(dict(scene, K=Ks[c]), objects, names, gt)
        rgbs.append(rgb)
        depths.append(depth)
        cam_masks.append(masks)
    refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
    scorer = _scorer(dev)
    syms = dict(box=None, torus=np.stack([np.eye(4), _zrot(180)]), vcol=np.stack([_zrot(a) for a in (0, 90, 180, 270)]))
    views, ests, masks = [], [], []
    for c, names in enumerate(cams):
        for k, name in enumerate(names):
            views.append(c)
            masks.append(cam_masks[c][k])
            ests.append(FoundationPose(model_pts=objects[name].vertices, model_normals=objects[name].vertex_normals, mesh=objects[name],
                                       symmetry_tfs=syms[name], scorer=scorer, refiner=refiner, device=dev))
    counts = [int(e.rot_grid.shape[0]) for e in ests]
    assert counts[0] == counts[3] == 252 and counts[1] < 252 and counts[2] == counts[4] < counts[1] and min(counts) >= 32, counts
    ids = [3, 7, 11, 3, 11]

    def solo(masks_):
        return [(e.register(K=Ks[v], rgb=rgbs[v], depth=depths[v], ob_mask=m, ob_id=i, iteration=2),
                 _state(e) if (np.asarray(m) > 0).sum() >= 4 else None) for e, v, m, i in zip(ests, views, masks_, ids)]

    def batched(masks_):
        poses = register_views(ests, views, rgbs, depths, Ks, masks_, ob_ids=ids, iteration=2)
        return [(p, _state(e) if (np.asarray(m) > 0).sum() >= 4 else None) for p, e, m in zip(poses, ests, masks_)]

    # (a) ragged counts over three cameras, one object in two of them
    got = batched(masks)
    _check(got, solo(masks))
    # (b) an empty mask and a mask of three valid depths: register()'s fallback pose, the state untouched, the others unchanged
    few = np.zeros_like(masks[2])
    rr, cc = np.nonzero((masks[2] > 0) & (depths[1] >= 0.001))
    mid = len(rr) // 2                                       # three neighbours inside the object: they survive the erosion
    few[rr[mid:mid + 3], cc[mid:mid + 3]] = 1
    cut = [masks[0], np.zeros_like(masks[1]), few, masks[3], masks[4]]
    before = [_state(ests[1]), _state(ests[2])]
    got_b = batched(cut)
    for e, b in zip(ests[1:3], before):
        assert torch.equal(e.poses, b["poses"]) and int(e.best_id) == b["best_id"]
    _check(got_b, solo(cut))
    assert np.array_equal(got_b[1][0], np.eye(4)) and not np.array_equal(got_b[2][0], np.eye(4))
    _check([got_b[k] for k in (0, 3, 4)], [got[k] for k in (0, 3, 4)])
    # (c) an estimator of 10 hypotheses: the split-K small-call path in its own register(), so it is held to the gates
    ests[4].rot_grid = ests[4].rot_grid[:10].clone()
    got_c = batched(masks)
    _check(got_c, solo(masks), small=(4,))
    _check(got_c[:4], got[:4])
    # track_views right after register_views stays within track_one's gates, on one kernel family as in
    # test_gpu_multi_view.py::test_track_views_is_per_estimator_track_one (without the override the five-hypothesis call and the
    # one-hypothesis calls take different split-K pieces: measured 7.2e-5 m / 1.9e-3 rad apart here)
    register_views(ests, views, rgbs, depths, Ks, masks, ob_ids=ids, iteration=2)
    start = [e.pose_last.clone() for e in ests]
    with engine.overrides(SPLITK_MAX_HYPS=0, HEADS_TWO_STREAMS_MAX_HYPS=0):
        many = np.stack(track_views(ests, views, rgbs, depths, Ks, iteration=2))
        one = []
        for e, v, s in zip(ests, views, start):
            e.pose_last = s.clone()
            one.append(e.track_one(rgbs[v], depths[v], Ks[v], iteration=2))
    one = np.stack(one)
    dR = geodesic(many[:, :3, :3], one[:, :3, :3])
    dt = np.linalg.norm(many[:, :3, 3].astype(np.float64) - one[:, :3, 3].astype(np.float64), axis=1)
    print(f"track_views after register_views vs track_one: |dt| max {dt.max():.3g} m, |dR| max {dR.max():.3g} rad")
    assert dt.max() <= 1e-4 and dR.max() <= 1e-3, (dt, dR)
