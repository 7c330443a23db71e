"""CPU: the depth-agreement check without a GPU -- fp_depth_agreement's argument errors through ctypes, the host record
ops.DepthAgreement, the numpy restatement the GPU tests compare the kernel with (tests/agreement_model.py), and the tolerance checks of
every new keyword, which refuse a bad value before any device work."""
import ctypes as C
import math

import numpy as np
import pytest

from agreement_model import classify, counts


def test_argument_errors_are_reported_without_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(16)

    def call(dc=p, xyz=p, tf=p, view=None, V=1, H=480, W=640, N=4, oh=160, ow=160, tol=0.01, out=p):
        return lib.fp_depth_agreement(dc, xyz, tf, view, V, H, W, N, oh, ow, tol, out, None)

    bad = [dict(dc=None), dict(xyz=None), dict(tf=None), dict(out=None), dict(oh=0), dict(ow=0), dict(H=0), dict(W=-3), dict(V=0),
           dict(N=65536), dict(N=-1), dict(V=3), dict(tol=-1e-6), dict(tol=float("nan")), dict(tol=float("inf")),
           dict(oh=2048, ow=1024)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.fp_last_error().startswith(b"fp_depth_agreement"), (kw, lib.fp_last_error())
    assert b"view is NULL" in (call(V=3), lib.fp_last_error())[1]
    assert b"tol" in (call(tol=-1.0), lib.fp_last_error())[1]
    # N == 0 does nothing (the N-sized tensors of an empty batch may be NULL); a view table with V > 1 is fine
    assert call(N=0) == 0 and call(N=0, dc=None, tf=None, out=None) == 0
    assert call(N=0, view=p, V=3) == 0 and call(N=0, tol=0.0) == 0


def test_depth_agreement_record():
    from foundationpose_amd.ops import DepthAgreement
    r = DepthAgreement(100, 80, 50, 10)
    assert (r.model, r.valid, r.agree, r.behind, r.front) == (100, 80, 50, 10, 20)
    assert r.valid_frac == 0.8 and r.agree_frac == 50 / 80 and r.behind_frac == 10 / 80
    z = DepthAgreement(0, 0, 0, 0)
    assert math.isnan(z.valid_frac) and math.isnan(z.agree_frac) and math.isnan(z.behind_frac) and z.front == 0
    off = DepthAgreement(300, 0, 0, 0)          # the model is drawn but nothing is observed there
    assert off.valid_frac == 0.0 and math.isnan(off.agree_frac) and math.isnan(off.behind_frac)
    rows = DepthAgreement.rows(np.asarray([[5, 4, 3, 1], [0, 0, 0, 0]], dtype=np.int32))
    assert rows == [DepthAgreement(5, 4, 3, 1), DepthAgreement(0, 0, 0, 0)]
    assert all(type(x) is int for x in rows[0])


def _one(zr, zo, tol):
    """one pixel through the restatement, as the host record of its counts: (model, valid, agree, behind, front) as 0 / 1"""
    from foundationpose_amd.ops import DepthAgreement
    m = [bool(x.item()) for x in classify(np.float32(zr), np.float32(zo), tol)]
    r = DepthAgreement.rows(counts(np.float32([zr]), np.float32([zo]), tol))[0]
    assert tuple(r) == tuple(int(x) for x in m)
    return tuple(r) + (r.front,)


def test_model_at_the_tolerance_edges():
    tol = np.float32(2.0 ** -7)                  # 7.8 mm: zr +- tol and their differences to zr are exact in float32 (checked)
    zr = np.float32(0.75)
    up, down = zr + tol, zr - tol
    assert up - zr == tol and zr - down == tol
    assert _one(zr, up, tol) == (1, 1, 1, 0, 0)          # exactly +tol: agree
    assert _one(zr, down, tol) == (1, 1, 1, 0, 0)        # exactly -tol: agree
    assert _one(zr, np.nextafter(up, np.float32(9)), tol) == (1, 1, 0, 1, 0)       # just past +tol: behind
    assert _one(zr, np.nextafter(down, np.float32(0)), tol) == (1, 1, 0, 0, 1)    # just past -tol: in front
    # the REFINE threshold: z_o just below 0.001 is no observation, at 0.001 it is one
    zr = np.float32(0.001)
    below = np.nextafter(np.float32(0.001), np.float32(0))
    assert _one(zr, below, tol) == (1, 0, 0, 0, 0)
    assert _one(zr, np.float32(0.001), tol) == (1, 1, 1, 0, 0)
    # no model pixel where the render draws nothing (0) or has a negative depth, whatever is observed
    assert _one(0.0, 0.75, tol) == (0, 0, 0, 0, 0) and _one(-0.5, 0.75, tol) == (0, 0, 0, 0, 0)
    assert _one(0.75, 0.0, tol) == (1, 0, 0, 0, 0)


def test_model_differences_are_float32():
    """z_o - z_r rounded to float32 (z_o more than twice z_r, so the difference is inexact): with tol = that float32 difference the
    pixel agrees, while the exact (float64) difference lies beyond tol and would count it behind"""
    rng = np.random.default_rng(0)
    for _ in range(1000):
        zr = np.float32(rng.uniform(0.2, 0.4))
        zo = np.float32(rng.uniform(0.9, 1.5))
        d32 = zo - zr
        if np.float64(zo) - np.float64(zr) > np.float64(d32):
            break
    else:
        pytest.fail("no inexact float32 difference found")
    tol = d32
    assert _one(zr, zo, tol) == (1, 1, 1, 0, 0)
    d64 = np.float64(zo) - np.float64(zr)
    assert d64 > np.float64(tol)                  # the float64 classification would say behind
    # and the tolerance is the float32 the C ABI receives: 0.01 as a float32 is below 0.01
    zr = np.float32(0.5)
    assert _one(zr, zr + np.float32(0.01), 0.01) == (1, 1, 1, 0, 0)


def test_model_counts_by_hypothesis():
    zr = np.zeros((2, 3, 4), np.float32)
    zo = np.zeros((2, 3, 4), np.float32)
    zr[0, :2] = 0.75                          # 8 model pixels
    zo[0, 0] = 0.75                           # 4 agree
    zo[0, 1, :2] = 0.9                        # 2 behind
    zo[0, 1, 2] = 0.5                         # 1 in front, 1 not observed
    zr[1, 2, 3] = 0.6
    zo[1] = 0.6                               # 1 agrees; the 11 others are not the model's
    from foundationpose_amd.ops import DepthAgreement
    rows = DepthAgreement.rows(counts(zr, zo, 0.01))
    assert rows == [DepthAgreement(8, 7, 4, 2), DepthAgreement(1, 1, 1, 0)] and [r.front for r in rows] == [1, 0]


def test_keywords_refuse_bad_tolerances_before_device_work():
    import torch
    from foundationpose_amd import estimater, ops
    from foundationpose_amd.estimater import FoundationPose, track_objects, track_views
    from foundationpose_amd.graphs import GraphedTracker
    est = object.__new__(FoundationPose)          # no state at all: anything past the check would raise something else
    for bad in (-0.001, float("nan"), float("inf"), "x", -1):
        with pytest.raises(ValueError, match="tolerance"):
            est.track_one(None, None, None, 2, agreement_tol=bad)
        with pytest.raises(ValueError, match="tolerance"):
            track_objects([est], None, None, None, agreement_tol=bad)
        with pytest.raises(ValueError, match="tolerance"):
            track_views([est], [0], [None], [None], [None], agreement_tol=bad)
        with pytest.raises(ValueError, match="tolerance"):
            estimater.depth_agreement([est], None, None, tol=bad)
        with pytest.raises(ValueError, match="tolerance"):
            GraphedTracker(None, None, None, None, 480, 640, agreement_tol=bad)
        with pytest.raises(ValueError, match="tolerance"):
            ops.depth_agreement(torch.zeros(1, 2, 2), torch.zeros(2, 2, 3), torch.zeros(1, 3, 3), bad)
    # a CPU tensor with a good tolerance gets to the device checks, and is refused there
    from foundationpose_amd import _lib
    with pytest.raises(_lib.FpAmdError, match="CUDA"):
        ops.depth_agreement(torch.zeros(1, 2, 2), torch.zeros(2, 2, 3), torch.zeros(1, 3, 3), 0.01)
    # defaults: no keyword, no check (the estimator starts without a record)
    assert FoundationPose.track_one.__defaults__[-1] is None


class _Est:
    """what depth_agreement reads before it touches a device"""

    def __init__(self, refiner):
        self.refiner, self.pose_last, self.device = refiner, object(), "cpu"


def test_depth_agreement_refusals_without_device():
    """one broken rule per call; a stub has no mesh, so anything past the checks would raise AttributeError instead"""
    from foundationpose_amd.estimater import depth_agreement
    r = object()
    a, b = _Est(r), _Est(r)
    depth, K = np.zeros((4, 6), np.float32), np.eye(3)
    two = dict(depths=[depth, depth], Ks=[K, K])
    with pytest.raises(ValueError, match="depth_agreement: no estimators"):
        depth_agreement([], depth, K)
    with pytest.raises(ValueError, match="depth_agreement: no estimators"):
        depth_agreement([], views=[], **two)
    for kw in (dict(depths=depth, Ks=K), dict(views=[0, 1], **two)):
        with pytest.raises(ValueError, match="depth_agreement: the estimators must share one refiner"):
            depth_agreement([a, _Est(object())], **kw)
        with pytest.raises(ValueError, match="depth_agreement: an estimator is listed twice"):
            depth_agreement([a, a], **kw)
        unreg = _Est(r)
        unreg.pose_last = None
        with pytest.raises(RuntimeError, match="depth_agreement: estimator 1 is not registered"):
            depth_agreement([a, unreg], **kw)
        for bad in (-0.001, float("nan"), float("inf"), "x"):
            with pytest.raises(ValueError, match="tolerance"):
                depth_agreement([a, b], tol=bad, **kw)
    with pytest.raises(ValueError, match="depth_agreement: 2 estimators but 1 view indices"):
        depth_agreement([a, b], views=[0], **two)
    with pytest.raises(ValueError, match="one of each per view"):
        depth_agreement([a, b], [depth, depth], [K], views=[0, 1])
    with pytest.raises(ValueError, match="views frame 2, outside 0..1"):
        depth_agreement([a, b], views=[0, 2], **two)
    with pytest.raises(ValueError, match="views frame -1, outside 0..1"):
        depth_agreement([a, b], views=[-1, 0], **two)
    with pytest.raises(ValueError, match="one H x W"):
        depth_agreement([a, b], [depth, np.zeros((5, 6), np.float32)], [K, K], views=[0, 1])
