"""GPU: fp_vsd_counts and fp_mspd (BOP's visible surface discrepancy and maximum symmetry-aware projection distance of pose batches)
against the numpy restatement of their definitions (tests/bop_errors_model.py): every integer of the count table equal, MSPD bit-equal;
what the kernels may write, their replay stability, the scene's renders, and the layers above (FoundationPose.bop_errors /
hypothesis_report, scripts/run_ycb_video.py --bop_scores).  Each test prints its figures before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import bop_errors_model as bm
from test_gpu_multi_object import dev  # noqa: F401
from test_gpu_pose_errors import _estimator, _points, _pose_sets, _symmetries
from test_pose_errors_host import HALF_TURN, _tf

pytestmark = pytest.mark.gpu

# a delta and thresholds that float32 holds exactly, so that pixels can sit exactly on them: delta = 2^-6, thr[t] = (t + 1) / 128
DELTA = 0.015625
THR16 = (np.arange(16, dtype=np.float64) + 1) / 128


def _random_maps(N, G, h, w, H, W, origin, T, seed):
    """seeded maps (not renders): est (N,h,w), gt (G,h,w), obs and fac (H,W) with zeros (whole blocks of them, as in a frame that is
    mostly background), holes, negatives and NaN, and pixels placed exactly on delta and on each threshold (where fac is 1, so that
    the float32 products are the values themselves)"""
    rng = np.random.default_rng(seed)
    x0, y0 = origin
    fac = rng.uniform(1.0, 1.3, (H, W)).astype(np.float32)
    obs = rng.uniform(0.4, 1.5, (H, W)).astype(np.float32)
    r = rng.random((H, W))
    obs[r < 0.10] = 0.0
    obs[(r >= 0.10) & (r < 0.13)] = -0.5
    obs[(r >= 0.13) & (r < 0.16)] = np.nan
    win = np.abs(np.nan_to_num(obs[y0:y0 + h, x0:x0 + w], nan=0.7))

    def layer(n, spread):
        m = win[None] + np.float32(spread) * rng.standard_normal((n, h, w), dtype=np.float32)
        np.maximum(m, np.float32(0.05), out=m)
        keep = rng.random((n, (h + 7) // 8, (w + 15) // 16)) < 0.4           # 8 x 16 blocks: 60 % of them empty
        keep = np.repeat(np.repeat(keep, 8, 1), 16, 2)[:, :h, :w]
        q = rng.random((n, h, w), dtype=np.float32)
        m[~keep | (q > 0.9)] = 0.0
        m[q < 0.01] = -0.3
        m[(q >= 0.01) & (q < 0.02)] = np.nan
        m[(q >= 0.02) & (q < 0.022)] = np.inf
        return m

    gt, est = layer(G, 0.02), layer(N, 0.04)
    # exact placements in the window's first pixels, as far as there is room: (obs, gt, est) at fac = 1
    exact = [(0.5, 0.5 + DELTA, 0.5), (0.5, np.nextafter(np.float32(0.5 + DELTA), np.float32(1)), 0.5), (0.5, 0.5, 0.5 + DELTA),
             (0.5, 0.5, np.nextafter(np.float32(0.5 + DELTA), np.float32(1)))]
    for t in range(T):
        exact += [(0.0, 0.5 + THR16[t], 0.5), (0.0, 0.5, np.nextafter(np.float32(0.5 + THR16[t]), np.float32(0)))]
    for i, (o, g, e) in enumerate(exact[:h * w]):
        y, x = divmod(i * 7919 % (h * w), w)                                 # scattered over the window, deterministic
        fac[y0 + y, x0 + x], obs[y0 + y, x0 + x] = 1.0, o
        gt[:, y, x], est[:, y, x] = g, e
    return est, gt, obs, fac


def _vsd_c(dev, est, gt, obs, fac, delta, thr, gt_index=None, origin=(0, 0), out=None):
    """through the C ABI with a factor table and thresholds of the test's own (ops.vsd_counts builds both from K and the diameter)"""
    from foundationpose_amd import _lib
    t = [a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev) for a in (est, gt, obs, fac)]
    gi = None if gt_index is None else torch.as_tensor(np.asarray(gt_index, np.int32), device=dev)
    N, h, w = t[0].shape
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    if out is None:
        out = torch.full((N, 4 + len(thr)), 12345, dtype=torch.int32, device=dev)       # whatever it held must not matter
    st = _lib.lib().fp_vsd_counts(C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()), C.c_void_p(0 if gi is None else gi.data_ptr()),
                                  int(t[1].shape[0]), N, h, w, C.c_void_p(t[2].data_ptr()), C.c_void_p(t[3].data_ptr()), int(t[2].shape[0]),
                                  int(t[2].shape[1]), int(origin[0]), int(origin[1]), float(delta), thr.ctypes.data_as(C.c_void_p), len(thr),
                                  C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st, "fp_vsd_counts")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ 1. the VSD kernel against the restatement
# (h, w, H, W, origin): full frames of 1 x 1, 7 x 13, 480 x 640, 481 x 643; an unaligned window and an aligned one in a larger frame
SHAPES = {"1x1": (1, 1, 1, 1, (0, 0)), "7x13": (7, 13, 7, 13, (0, 0)), "480x640": (480, 640, 480, 640, (0, 0)),
          "481x643": (481, 643, 481, 643, (0, 0)), "window@3,5": (37, 52, 64, 80, (3, 5)), "window@8,5": (37, 52, 64, 80, (8, 5)),
          "window-ragged": (30, 41, 64, 80, (4, 0))}
BATCHES = [(1, 1, None), (5, 1, None), (5, 5, None), (252, 1, None), (7, 3, [0, 2, 1, 3, 2, -1, 0])]


def _cases():
    for name in SHAPES:
        big = name in ("480x640", "481x643")
        for N, G, gi in BATCHES:
            for T in (1, 10, 16):
                if big and not ((N == 252 and T == 10 and name == "480x640") or (N in (5, 7) and (T == 10 or G == 1))):
                    continue                 # the full frames: every batch form with T = 10, T = 1 and 16 with (5, 1), 252 once
                yield pytest.param(name, N, G, gi, T, id=f"{name}-N{N}-G{G}-T{T}")


@pytest.mark.parametrize("name,N,G,gi,T", list(_cases()))
def test_every_integer_equals_the_restatement(dev, name, N, G, gi, T):
    h, w, H, W, origin = SHAPES[name]
    est, gt, obs, fac = _random_maps(N, G, h, w, H, W, origin, T, seed=1000 * N + 10 * T + G + len(name))
    thr = THR16[:T].astype(np.float32)
    got = _vsd_c(dev, est, gt, obs, fac, DELTA, thr, gi, origin).cpu().numpy()
    ref = bm.vsd_counts(est, gt, obs, fac, DELTA, thr, gi, origin)
    bad = np.argwhere(got != ref)
    print(f"{name} N={N} G={G} T={T}: row 0 {got[0].tolist()}, {len(bad)} of {got.size} integers differ")
    assert got.dtype == np.int32 and got.shape == (N, 4 + T) and len(bad) == 0, (bad[:10], got[bad[:10, 0]], ref[bad[:10, 0]])
    if gi is not None:
        assert (got[[3, 5]] == -1).all() and (got[[0, 1, 2, 4, 6]] >= 0).all()
    if h * w >= 2 * (4 + 2 * T):        # the placements exist: the maps are not all background
        assert (got[got[:, 0] >= 0][:, :4] > 0).all()


def test_pixels_on_the_bounds(dev):
    """one row of pixels at fac = 1, by hand: (Dm - Do) <= delta holds on delta and fails one ulp above; dist >= thr holds on thr and
    fails one ulp below"""
    up = lambda v: np.nextafter(np.float32(v), np.float32(9))      # noqa: E731
    dn = lambda v: np.nextafter(np.float32(v), np.float32(0))      # noqa: E731
    #            obs  gt              est
    px = [(0.5, 0.5 + DELTA, 0.5 + DELTA),        # both on delta: visible, dist 0
          (0.5, up(0.5 + DELTA), 0.5),            # gt one ulp beyond delta: not visible; est visible alone
          (0.5, 0.5, up(0.5 + DELTA)),            # est beyond delta but kept by the visible gt: inter, dist just over delta
          (0.0, 0.625, 0.5),                      # no measurement: both visible, dist = 16/128 exactly: every threshold counts it
          (0.0, 0.5, dn(0.5 + 1 / 128)),          # dist one ulp under thr[0]: no threshold counts it
          (np.nan, 0.5 + 2 / 128, 0.5),           # NaN is no measurement: dist = 2/128: thr[0], thr[1]
          (0.0, 0.0, 0.0)]
    obs, gt, est = (np.asarray([p[i] for p in px], np.float32)[None] for i in range(3))
    got = _vsd_c(dev, est[None], gt[None], obs, np.ones_like(obs), DELTA, THR16.astype(np.float32)).cpu().numpy()[0]
    print("by hand:", got.tolist())
    assert got.tolist() == [5, 6, 5, 6] + [3, 3] + [1] * 14
    assert np.array_equal(got, bm.vsd_counts(est[None], gt[None], obs, np.ones_like(obs), DELTA, THR16.astype(np.float32))[0])


# ------------------------------------------------------------------ 2. what it writes, and the same values every time
def test_writes_nothing_outside_the_table_and_ignores_what_it_held(dev):
    h, w, N, T = 33, 44, 5, 10
    est, gt, obs, fac = _random_maps(N, 1, h, w, h, w, (0, 0), T, seed=5)
    thr = THR16[:T].astype(np.float32)
    ref = bm.vsd_counts(est, gt, obs, fac, DELTA, thr)
    for poison in (-7, 0, 2 ** 30):
        arena = torch.full((64 + N * (4 + T) + 64,), poison, dtype=torch.int32, device=dev)
        out = arena[64:64 + N * (4 + T)].view(N, 4 + T)
        _vsd_c(dev, est, gt, obs, fac, DELTA, thr, out=out)
        a = arena.cpu().numpy()
        assert (a[:64] == poison).all() and (a[64 + N * (4 + T):] == poison).all()
        assert np.array_equal(a[64:64 + N * (4 + T)].reshape(N, 4 + T), ref), poison
    # the inputs are read only: the maps hold what they held
    t = [torch.as_tensor(a, device=dev) for a in (est, gt)]
    keep = [x.clone() for x in t]
    _vsd_c(dev, t[0], t[1], obs, fac, DELTA, thr)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(t, keep))


def test_rows_replays_graph_and_empty_batch(scene, dev):
    from foundationpose_amd import ops
    H, W, N, T = 96, 128, 7, 10
    est, gt, obs, _ = _random_maps(N, N, H, W, H, W, (0, 0), T, seed=9)
    K = np.array([[150.0, 0, 60.5], [0, 149.0, 50.25], [0, 0, 1]])
    fac = bm.dist_factor(K, H, W)
    ref = bm.vsd_counts(est, gt, obs, fac, bm.BOP_DELTA, bm.thresholds(bm.BOP_TAUS, 0.2))
    e, g, o = (torch.as_tensor(a, device=dev) for a in (est, gt, obs))
    batch = ops.vsd_counts(e, g, o, K, 0.2).cpu().numpy()
    assert np.array_equal(batch, ref) and batch.dtype == np.int32
    assert np.array_equal(ops.vsd_counts(e, g, o, K, 0.2).cpu().numpy(), batch)
    for k in range(N):                       # row k of the batch = the call on map k alone, pairwise and through an index
        assert np.array_equal(ops.vsd_counts(e[k:k + 1], g[k:k + 1], o, K, 0.2).cpu().numpy(), batch[k:k + 1]), k
    gi = torch.arange(N, dtype=torch.int32, device=dev).flip(0).contiguous()
    assert np.array_equal(ops.vsd_counts(e.flip(0).contiguous(), g, o, K, 0.2, gt_index=gi).cpu().numpy(), batch[::-1])
    rows = ops.VsdCounts.rows(torch.as_tensor(batch))
    assert np.array_equal(np.stack([r.errors() for r in rows]), bm.vsd_from_counts(ref))
    # a captured graph owns its output; the thresholds and the factor are fixed at capture
    out = torch.zeros((N, 4 + T), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.vsd_counts(e, g, o, K, 0.2, out=out)              # warm-up outside the capture (uploads the factor)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.vsd_counts(e, g, o, K, 0.2, out=out)
    for _ in range(3):
        out.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), batch)
    e.copy_(e.flip(0).contiguous())          # new maps in the graph's input buffer: the replay counts them
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), bm.vsd_counts(est[::-1], gt, obs, fac, bm.BOP_DELTA, bm.thresholds(bm.BOP_TAUS, 0.2)))
    # N == 0: nothing happens, an empty table comes back
    empty = ops.vsd_counts(e[:0], g[:1], o, K, 0.2)
    assert tuple(empty.shape) == (0, 14) and empty.dtype == torch.int32
    # the checks only device tensors reach
    from foundationpose_amd import _lib
    for kw, msg in ((dict(est_depth=e.double()), "est_depth: expected dtype"), (dict(gt_depth=g.transpose(1, 2)), "gt_depth must be"),
                    (dict(gt_depth=torch.zeros(N, H, 2 * W, device=dev)[:, :, ::2]), "gt_depth: tensor must be contiguous"),
                    (dict(obs_depth=o.t()), "not inside"), (dict(obs_depth=torch.zeros(H, 2 * W, device=dev)[:, ::2]), "obs_depth: tensor must be contiguous"),
                    (dict(gt_index=gi.long()), "gt_index: expected dtype"), (dict(gt_index=gi.cpu()), "gt_index: expected a CUDA"),
                    (dict(out=torch.zeros(N, 14, device=dev)), "out: expected dtype"),
                    (dict(out=torch.zeros(N, 13, dtype=torch.int32, device=dev)), rf"out must be \({N}, 14\)")):
        args = dict(est_depth=e, gt_depth=g, obs_depth=o, K=K, diameter=0.2)
        args.update(kw)
        with pytest.raises(_lib.FpAmdError, match=msg):
            ops.vsd_counts(**args)


# ------------------------------------------------------------------ 3. the scene's renders
def _render(handle, poses, K, dev):
    from foundationpose_amd import ops
    p = torch.as_tensor(np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 4, 4), device=dev)
    return ops.render_crops(handle, p, None, K, 480, 640, (480, 640), normalize_xyz=False, want=("depth",))["depth"]


def test_scene_renders(scene, dev):
    """the GPU's own full-frame renders of the 252 grid poses and the ground truth through the kernel: equal to the restatement on
    those same renders; against the restatement on the CPU oracle's renders the counts may differ by at most the number of pixels
    where a comparison is decided by less than 2e-5 m of depth (render floats agree to 1e-5 m and two renders meet in a comparison),
    counted per column here"""
    from foundationpose_amd import ops
    from foundationpose_amd.Utils import get_mesh_handle, make_mesh_tensors
    from oracle import ops as oo
    handle = get_mesh_handle(make_mesh_tensors(scene["mesh"], device=dev))
    K, diam = scene["K"], scene["diameter"]
    est, gt = _render(handle, scene["poses"], K, dev), _render(handle, scene["gt"], K, dev)
    obs = np.asarray(scene["depth"], np.float32)
    got = ops.vsd_counts(est, gt, torch.as_tensor(obs, device=dev), K, diam).cpu().numpy()
    fac, thr = bm.dist_factor(K, 480, 640), bm.thresholds(bm.BOP_TAUS, diam)
    est_d, gt_d = est.cpu().numpy(), gt.cpu().numpy()
    ref = bm.vsd_counts(est_d, gt_d, obs, fac, bm.BOP_DELTA, thr)
    print("scene, device renders: rows 0..2", got[:3].tolist(), "integers that differ:", int((got != ref).sum()))
    assert np.array_equal(got, ref)
    assert np.array_equal(ops.VsdCounts.rows(got)[0].errors(), bm.vsd_from_counts(ref)[0])
    # the ground truth against itself
    same = ops.vsd_counts(gt, gt, torch.as_tensor(obs, device=dev), K, diam).cpu().numpy()[0]
    assert same[0] == same[1] == same[2] == same[3] == int((gt_d > 0).sum()) and (same[4:] == 0).all()
    # the CPU oracle's renders
    est_o = oo.render_crops(scene["mesh_np"], scene["poses"], None, K, 480, 640, (480, 640), normalize_xyz=False, want=("depth",))["depth"]
    gt_o = oo.render_crops(scene["mesh_np"], np.asarray(scene["gt"], np.float32)[None], None, K, 480, 640, (480, 640), normalize_xyz=False,
                           want=("depth",))["depth"]
    print("largest |device render - oracle render|:", float(np.abs(est_d - est_o).max()), float(np.abs(gt_d - gt_o).max()))
    ref_o = bm.vsd_counts(est_o, gt_o, obs, fac, bm.BOP_DELTA, thr)
    margin = np.float64(2e-5) * fac.astype(np.float64)
    Do = np.where(obs > 0, obs, 0).astype(np.float64) * fac
    Dg = gt_o[0].astype(np.float64) * fac
    allowed = np.zeros_like(ref_o)
    with np.errstate(invalid="ignore"):
        cg = (Do > 0) & (Dg > 0) & (np.abs((Dg - Do) - bm.BOP_DELTA) <= margin)
        cover_g = (gt_o[0] > 0) != (gt_d[0] > 0)
        for n in range(len(est_o)):
            De = est_o[n].astype(np.float64) * fac
            ce = (Do > 0) & (De > 0) & (np.abs((De - Do) - bm.BOP_DELTA) <= margin)
            vis_any = cg | ce | cover_g | ((est_o[n] > 0) != (est_d[n] > 0))
            allowed[n, 0] = (cg | cover_g).sum()
            allowed[n, 1:4] = vis_any.sum()
            dist = np.abs(Dg - De)
            for t in range(len(thr)):
                allowed[n, 4 + t] = (vis_any | ((Dg > 0) & (De > 0) & (np.abs(dist - float(thr[t])) <= margin))).sum()
    diff = np.abs(got.astype(np.int64) - ref_o)
    print("device renders against oracle renders: largest difference per column", diff.max(0).tolist(), "allowed", allowed.max(0).tolist(),
          "rows that differ:", int((diff > 0).any(1).sum()))
    assert (diff <= allowed).all(), np.argwhere(diff > allowed)


# ------------------------------------------------------------------ 4. MSPD
K_YCBV = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])


def _mspd(dev, pts, poses, gts, gi, sym, out=None):
    from foundationpose_amd import ops
    g = None if gi is None else torch.as_tensor(np.asarray(gi, np.int32), device=dev)
    return ops.mspd(torch.as_tensor(pts, device=dev), torch.as_tensor(poses, device=dev), gts, K_YCBV, gt_index=g, symmetry_tfs=sym, out=out)


def _bit_equal(got, ref, what):
    same = (got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))
    finite = ~np.isnan(ref)
    print(f"{what}: {int((~same).sum())} of {len(ref)} rows differ, {int((~finite).sum())} NaN; finite range {np.nanmin(ref) if finite.any() else None} .. "
          f"{np.nanmax(ref) if finite.any() else None} px")
    assert got.dtype == np.float64 and same.all(), (what, np.argwhere(~same)[:5], got[~same][:5], ref[~same][:5])


@pytest.mark.parametrize("N,P,S,G", [(1, 1, 0, 1), (3, 255, 1, 1), (3, 257, 3, 3), (252, 2501, 0, 1), (252, 2501, 6, 252), (5, 10007, 2, 1)])
def test_mspd_bit_equal(dev, N, P, S, G):
    pts, sym = _points(P, 3 * P + N), _symmetries(S, N)
    poses, gts = _pose_sets(N, G, 2000 + N + P)
    got = _mspd(dev, pts, poses, gts, None, sym).cpu().numpy()
    _bit_equal(got, bm.mspd(pts, poses, gts, K_YCBV, None, sym), f"N={N} P={P} S={S} G={G}")
    assert got.shape == (N,)
    if S == 1:      # S_0 = I: the same as no symmetry set
        assert np.array_equal(got.view(np.uint64), _mspd(dev, pts, poses, gts, None, None).cpu().numpy().view(np.uint64))


def test_mspd_nan_rows_index_and_arena(dev):
    P = 300
    pts, sym = _points(P, 31), _symmetries(3, 32)
    poses, gts = _pose_sets(8, 2, 33)
    poses[1, 0, 3] = np.nan
    poses[2, 1, 1] = np.inf
    poses[3, 2, 3] = 0.01              # the camera plane cuts the object
    poses[4, 2, 3] = -0.6              # behind the camera
    gi = [0, 0, 1, 1, 0, 2, -1, 1]
    sentinel = -1.25e300
    arena = torch.full((64 + 8 + 64,), sentinel, dtype=torch.float64, device=dev)
    out = arena[64:72]
    r = _mspd(dev, pts, poses, gts, gi, sym, out=out)
    assert r.data_ptr() == out.data_ptr()
    a = arena.cpu().numpy()
    assert (a[:64] == sentinel).all() and (a[72:] == sentinel).all()
    got = a[64:72]
    assert np.isfinite(got[[0, 7]]).all() and np.isnan(got[1:7]).all(), got
    _bit_equal(got, bm.mspd(pts, poses, gts, K_YCBV, gi, sym), "NaN rows")
    # a ground truth behind the camera, a symmetry that is not finite: every row that uses them
    gts2 = gts.copy()
    gts2[1, 2, 3] = -0.5
    good = _pose_sets(8, 2, 33)[0]
    got = _mspd(dev, pts, good, gts2, [0, 1] * 4, None).cpu().numpy()
    assert np.isfinite(got[0::2]).all() and np.isnan(got[1::2]).all()
    sym[2, 0, 3] = np.nan
    assert np.isnan(_mspd(dev, pts, good, gts, [0, 1] * 4, sym).cpu().numpy()).all()
    # rows alone = rows in the batch; N == 0
    batch = _mspd(dev, pts, good, gts, [0, 1] * 4, _symmetries(3, 32)).cpu().numpy()
    for k in (0, 3, 7):
        one = _mspd(dev, pts, good[k:k + 1], gts[k % 2:k % 2 + 1], None, _symmetries(3, 32)).cpu().numpy()
        assert np.array_equal(one.view(np.uint64), batch[k:k + 1].view(np.uint64))
    assert tuple(_mspd(dev, pts, good[:0], gts[:1], None, None).shape) == (0,)
    from foundationpose_amd import _lib, ops
    with pytest.raises(_lib.FpAmdError, match=r"out must be \(8,\)"):
        _mspd(dev, pts, good, gts[:1], None, None, out=torch.zeros(9, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.FpAmdError, match="out: expected dtype"):
        _mspd(dev, pts, good, gts[:1], None, None, out=torch.zeros(8, device=dev))
    with pytest.raises(_lib.FpAmdError, match="poses: expected dtype"):
        ops.mspd(torch.as_tensor(pts, device=dev), torch.as_tensor(good, device=dev).double(), gts[:1], K_YCBV)


def test_mspd_graph_replay(dev):
    from foundationpose_amd import ops
    P, N = 2501, 7
    pts, sym = _points(P, 21), _symmetries(3, 22)
    poses, gts = _pose_sets(N, N, 23)
    ref = bm.mspd(pts, poses, gts, K_YCBV, None, sym)
    pts_t, poses_t = torch.as_tensor(pts, device=dev), torch.as_tensor(poses, device=dev)
    gt_t, sym_t = torch.as_tensor(gts, device=dev), torch.as_tensor(sym, device=dev)
    out = torch.zeros(N, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.mspd(pts_t, poses_t, gt_t, K_YCBV, symmetry_tfs=sym_t, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mspd(pts_t, poses_t, gt_t, K_YCBV, symmetry_tfs=sym_t, out=out)
    for _ in range(3):
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        _bit_equal(out.cpu().numpy(), ref, "graph replay")


# ------------------------------------------------------------------ 5. the estimator
def test_estimator_bop_errors(scene, dev):
    from foundationpose_amd import ops
    from foundationpose_amd.Utils import get_mesh_handle
    shift = (0.03, -0.02, 0.05)
    mesh = scene["mesh"].copy()
    mesh.vertices = np.asarray(mesh.vertices) + np.asarray(shift)           # a mesh whose model_center is not 0
    gt = np.asarray(scene["gt"], np.float64) @ _tf(np.eye(3), -np.asarray(shift))   # the same object in the camera, in the shifted mesh's frame
    est = _estimator(mesh, dev)
    K, raw = scene["K"], np.asarray(scene["depth"], np.float32)
    with pytest.raises(RuntimeError, match="no registration"):
        est.bop_errors(gt, raw, K)
    est.register(K, scene["rgb"], scene["depth"], scene["mask"], iteration=2)
    e = est.bop_errors(gt, raw, K)
    assert sorted(e) == ["counts", "mspd", "mssd", "vsd"] and all(v.is_cuda for v in e.values())
    assert tuple(e["vsd"].shape) == (252, 10) and e["vsd"].dtype == torch.float64 and tuple(e["counts"].shape) == (252, 14)
    assert tuple(e["mssd"].shape) == (252,) and tuple(e["mspd"].shape) == (252,) and e["mspd"].dtype == torch.float64
    # VSD: the restatement on device renders made here, with the ground truth in the centred frame rounded to float32 once
    gt_c = gt @ _tf(np.eye(3), est.model_center)
    handle = get_mesh_handle(est.mesh_tensors)
    est_d = _render(handle, est.poses.cpu().numpy(), K, dev).cpu().numpy()
    gt_d = _render(handle, gt_c.astype(np.float32), K, dev).cpu().numpy()
    ref = bm.vsd_counts(est_d, gt_d, raw, bm.dist_factor(K, 480, 640), bm.BOP_DELTA, bm.thresholds(bm.BOP_TAUS, est.diameter))
    counts, vsd = e["counts"].cpu().numpy(), e["vsd"].cpu().numpy()
    print("estimator: counts of the returned pose", counts[0].tolist(), "vsd", vsd[0].tolist())
    print("mssd / diameter, mspd of the returned pose:", float(e["mssd"][0]) / est.diameter, float(e["mspd"][0]))
    assert np.array_equal(counts, ref)
    assert np.array_equal(vsd.view(np.uint64), bm.vsd_from_counts(ref).view(np.uint64))
    # MSSD is pose_errors' column, MSPD the restatement's
    table = est.pose_errors(gt).cpu().numpy()
    assert np.array_equal(e["mssd"].cpu().numpy().view(np.uint64), table[:, 3].view(np.uint64))
    _bit_equal(e["mspd"].cpu().numpy(), bm.mspd(est.pts.cpu().numpy(), est.poses.cpu().numpy(), gt_c[None], K), "estimator mspd")
    # the chunk changes nothing; a pose list of the caller's, and one ground truth per pose
    for chunk in (5, 252):
        c = est.bop_errors(gt, raw, K, chunk=chunk)
        assert all(torch.equal(c[k], e[k]) for k in ("counts", "mssd", "mspd")) and torch.equal(c["vsd"].view(torch.int64), e["vsd"].view(torch.int64))
    few = est.bop_errors(np.stack([gt] * 3), raw, K, poses=est.poses[[0, 100, 251]], taus=(bm.BOP_TAUS[1], bm.BOP_TAUS[5]), chunk=2)
    assert np.array_equal(few["counts"].cpu().numpy(), counts[[0, 100, 251]][:, [0, 1, 2, 3, 5, 9]])
    assert torch.equal(few["mspd"], e["mspd"][[0, 100, 251]])
    with pytest.raises(ValueError, match="2 ground truths for 252 poses"):
        est.bop_errors(np.stack([gt] * 2), raw, K)
    # the report: best rank = argmin of the mean over taus / of the pixel distance
    mean = e["vsd"].mean(dim=1).cpu().numpy()
    for metric, col in (("vsd", mean), ("mspd", e["mspd"].cpu().numpy())):
        rep = est.hypothesis_report(gt, metric=metric, depth=raw, K=K)
        k = int(np.argmin(col))
        print("hypothesis_report", rep)
        assert rep["best_rank"] == k and rep["best_err"] == col[k] and rep["top_err"] == col[0] and rep["n"] == 252 and rep["metric"] == metric
        assert rep["top_score"] == float(est.scores[0]) and rep["best_score"] == float(est.scores[k])
    assert est.hypothesis_report(gt)["metric"] == "adds"                     # the present call as it was
    # a half turn about the can's axis with the turn in the symmetry set: nothing to MSSD and MSPD
    sym_est = _estimator(scene["mesh"], dev, symmetry_tfs=np.stack([np.eye(4), HALF_TURN]))
    g0 = np.asarray(scene["gt"], np.float64)
    flipped = torch.as_tensor((g0 @ HALF_TURN @ _tf(np.eye(3), sym_est.model_center)).astype(np.float32), device=dev)[None]
    f = sym_est.bop_errors(g0, raw, K, poses=flipped)
    print("half turn: mssd", float(f["mssd"][0]), "mspd", float(f["mspd"][0]), "vsd", f["vsd"][0].tolist())
    assert float(f["mssd"][0]) < 1e-6 and float(f["mspd"][0]) < 1e-2 and float(f["vsd"][0, 0]) < 0.05
    assert ops.VsdCounts.rows(e["counts"])[0].errors().tolist() == vsd[0].tolist()


# ------------------------------------------------------------------ 6. the script
def test_run_ycb_video_bop_scores(tmp_path, dev):
    import glob
    import importlib.util
    import os

    import yaml
    from foundationpose_amd import vis
    from foundationpose_amd.datareader import YcbVideoReader
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_ycb_video", os.path.join(root, "scripts", "run_ycb_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    plain = mod.main(["--synthetic", "2", "--est_refine_iter", "1", "--debug_dir", str(tmp_path / "a")])
    full = mod.main(["--synthetic", "2", "--est_refine_iter", "1", "--bop_scores", "--debug_dir", str(tmp_path / "b")])
    both = mod.main(["--synthetic", "2", "--est_refine_iter", "1", "--bop_scores", "--hypothesis_errors", "--debug_dir", str(tmp_path / "c")])
    assert sorted(plain) == ["ADDS_AUC", "ADDS_mean_m", "ADD_AUC", "ADD_mean_m", "n"]              # exactly today's keys
    assert {k: full[k] for k in plain} == plain
    keys = ["AR", "AR_MSPD", "AR_MSSD", "AR_VSD"]
    assert sorted(set(full) - set(plain)) == keys + ["bop_errors"]
    print({k: full[k] for k in keys})
    assert all(0.0 <= full[k] <= 1.0 for k in keys)
    errs = full["bop_errors"]
    assert len(errs["vsd"]) == len(errs["mspd"]) == len(errs["mssd_over_diameter"]) == full["n"] == 2 and len(errs["vsd"][0]) == 10
    assert {k: full[k] for k in keys} == vis.bop_average_recall(np.asarray(errs["vsd"]), errs["mssd_over_diameter"], errs["mspd"], 640)
    # with the hypotheses: the same scores (row 0 of the batch is the returned pose) and the VSD-oracle rank
    assert {k: both[k] for k in keys} == {k: full[k] for k in keys} and both["bop_errors"] == errs
    assert len(both["vsd_best_rank"]) == 2 and all(0 <= r < 252 for r in both["vsd_best_rank"]) and "best_rank_hist" in both
    # the errors recomputed here from the poses the script wrote: an estimator of this test's own on the same data
    res = yaml.safe_load(open(tmp_path / "b" / "ycbv_res.yml"))
    video_dir = sorted(glob.glob(str(tmp_path / "b" / "synthetic_bop" / "test" / "*")))[0]
    reader = YcbVideoReader(video_dir, zfar=1.5, models_dir=str(tmp_path / "b" / "synthetic_bop" / "models"))
    ob_id = reader.ob_ids[0]
    mesh = reader.get_gt_mesh(ob_id)
    est = _estimator(mesh, dev, symmetry_tfs=reader.symmetry_tfs[ob_id])
    vsd, mssd, mspd = [], [], []
    for i in range(len(reader)):
        pose = np.asarray(res[reader.get_video_id()][reader.id_strs[i]][int(ob_id)], np.float64)
        centred = torch.as_tensor((pose @ _tf(np.eye(3), est.model_center)).astype(np.float32), device=dev)[None]
        gt = reader.get_gt_pose(i, ob_id, mask=reader.get_mask(i, ob_id))
        e = est.bop_errors(gt, reader.get_depth(i), reader.get_K(i), poses=centred)
        vsd.append(e["vsd"][0].cpu().numpy()); mssd.append(float(e["mssd"][0]) / est.diameter); mspd.append(float(e["mspd"][0]))
    print("recomputed:", np.asarray(vsd).tolist(), mssd, mspd, "script:", errs)
    # the script's pose passed through float32 `pose @ T(-centre)` and back: the errors agree to that rounding (1e-6 of a diameter, 1e-3
    # of a pixel, a handful of the ~30 000 visible pixels), and the recalls are equal unless an error lies that close to a threshold
    assert np.allclose(mssd, errs["mssd_over_diameter"], rtol=0, atol=1e-5) and np.allclose(mspd, errs["mspd"], rtol=0, atol=1e-2)
    assert np.allclose(vsd, errs["vsd"], rtol=0, atol=1e-3)
    again = vis.bop_average_recall(np.asarray(vsd), mssd, mspd, 640)
    near = sum(int(np.sum(np.abs(np.asarray(v, np.float64).reshape(-1, 1) - np.asarray(th)) <= tol))
               for v, th, tol in ((vsd, vis.BOP_THETAS, 1e-3), (mssd, vis.BOP_THETAS, 1e-5), (mspd, vis.BOP_THETAS_PX, 1e-2)))
    print("recalls recomputed:", again, "errors within the rounding of a threshold:", near)
    if near == 0:
        assert again == {k: full[k] for k in keys}
    assert all(abs(again[k] - full[k]) <= near / 20.0 for k in keys)
