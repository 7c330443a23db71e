"""CPU: the crop stage with a view table (several camera frames per refine call) -- argument errors of the C ABI, reported without a GPU,
the (view, object) grouping of the two-pose quirk on hand-made indices, and the refusals of ops.Views and track_views that need no
device."""
import ctypes as C

import numpy as np
import pytest

P16 = C.c_void_p(16)     # a made-up device address: every check below fails before anything is read


def test_views_entry_points_report_argument_errors_without_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    # crop windows: NULL K table, V < 1, view NULL with V > 1, obj NULL with several objects
    crop = lambda Ks, view, V, obj, N=4, diam=P16, M=2: lib.fp_crop_windows(P16 if N else None, None, Ks, view, V, 0.0, diam, obj, M, 1.2,
                                                                            160, 160, N, P16 if N else None, P16 if N else None, None)
    assert crop(None, P16, 2, P16) == -1
    assert b"fp_crop_windows: need the K table" in lib.fp_last_error()
    assert crop(P16, P16, 0, P16) == -1
    assert b"V >= 1 views (V=0)" in lib.fp_last_error()
    assert crop(P16, None, 3, P16) == -1
    assert b"view is NULL but there are 3 views" in lib.fp_last_error()
    assert crop(P16, P16, 3, None) == -1
    assert b"obj is NULL but there are 2 objects" in lib.fp_last_error()
    # a view table goes with the diameter table: Ks with a scalar diameter is refused and says so
    assert crop(P16, P16, 2, None, diam=None, M=0) == -1
    assert b"fp_crop_windows: a view table (Ks) with a scalar diameter" in lib.fp_last_error()
    # render: NULL set, unknown flags, NULL K table, missing view index
    args = lambda Ks, view, V, flags: (None, None, None, None, 0.0, P16, P16, None, Ks, view, V, 480, 640, 4, 160, 160, 0.8, 0.5, 0.001,
                                       flags, None, None, None, None, None, None, None, None, 0, None)
    assert lib.fp_render_crops(*args(P16, P16, 2, 1)) == -1 and b"fp_render_crops: NULL mesh set" in lib.fp_last_error()
    assert lib.fp_render_crops(*args(P16, P16, 2, 0x40)) == -1
    assert b"fp_render_crops: unknown flag bits 0x40" in lib.fp_last_error()
    # warp: unknown flags, NULL K table, V < 1, missing view index, unknown mode
    wargs = lambda Ks, view, V, flags, mode: (P16, P16, P16, P16, None, Ks, view, V, P16, 0.0, P16, P16, 2, flags, mode, 480, 640, 4,
                                              160, 160, P16, None)
    assert lib.fp_warp_crops(*wargs(P16, P16, 2, 0x10, 0)) == -1
    assert b"fp_warp_crops: unknown flag bits 0x10" in lib.fp_last_error()
    assert lib.fp_warp_crops(*wargs(None, P16, 2, 1, 0)) == -1 and b"need the K table" in lib.fp_last_error()
    assert lib.fp_warp_crops(*wargs(P16, P16, 0, 1, 0)) == -1 and b"(V=0)" in lib.fp_last_error()
    assert lib.fp_warp_crops(*wargs(P16, None, 2, 1, 0)) == -1 and b"view is NULL but there are 2 views" in lib.fp_last_error()
    assert lib.fp_warp_crops(*wargs(P16, P16, 2, 1, 7)) == -1 and b"fp_warp_crops: unknown mode 7" in lib.fp_last_error()
    # pose update: NULL K table, missing view index, unknown rot_rep / trans_rep
    pargs = lambda Ks, view, V, rr, tr: (P16, P16, P16, rr, 1, None, 0.35, 0.0, P16, P16, 2, 8, P16, None, None, tr, None, Ks, view, V,
                                         P16, 160.0, None)
    assert lib.fp_pose_update(*pargs(None, P16, 2, 0, 0)) == -1 and b"fp_pose_update: need the K table" in lib.fp_last_error()
    assert lib.fp_pose_update(*pargs(P16, None, 2, 0, 0)) == -1 and b"view is NULL but there are 2 views" in lib.fp_last_error()
    assert lib.fp_pose_update(*pargs(P16, P16, 2, 5, 0)) == -1 and b"unknown rot_rep 5" in lib.fp_last_error()
    assert lib.fp_pose_update(*pargs(P16, P16, 2, 0, 9)) == -1 and b"unknown trans_rep 9" in lib.fp_last_error()
    # the batched ingest: V < 1, NULL K table
    assert lib.fp_depth_erode_frames(P16, P16, 480, 640, 0, 2, 0.001, 0.8, 100.0, None) == -1
    assert b"fp_depth_erode_frames: V=0" in lib.fp_last_error()
    assert lib.fp_depth_bilateral_frames(P16, P16, 480, 640, 0, 2, 100.0, 2.0, 1e5, None) == -1
    assert b"fp_depth_bilateral_frames: V=0" in lib.fp_last_error()
    assert lib.fp_depth_to_xyz_frames(P16, None, 1e9, 0, P16, 480, 640, 2, None) == -1
    assert b"fp_depth_to_xyz_frames: NULL K table" in lib.fp_last_error()
    # N == 0 after valid tables is a no-op
    assert crop(P16, P16, 2, P16, N=0) == 0


def test_quirk_is_grouped_per_view_and_object():
    from foundationpose_amd.predict_pose_refine import parts_for_pairs, two_pose_pairs
    # two views x one object x one hypothesis: two reference calls of ONE pose each -- no pair (a per-object grouping pairs them)
    assert two_pose_pairs([0, 0], [0, 1]) == []
    assert two_pose_pairs([0, 0]) == [(0, 1)]
    # two views x one object x two hypotheses: one pair per view
    assert two_pose_pairs([0, 0, 0, 0], [0, 0, 1, 1]) == [(0, 1), (2, 3)]
    assert two_pose_pairs([0, 0, 0, 0], [0, 1, 0, 1]) == [(0, 2), (1, 3)]
    # interleaved rows of (view, object): groups of exactly two pair up, a group of three or one does not
    view = [1, 0, 1, 2, 0, 1, 2, 0, 1]
    obj = [0, 1, 1, 0, 1, 0, 0, 0, 1]
    # groups: (1,0): 0,5   (0,1): 1,4   (1,1): 2,8   (2,0): 3,6   (0,0): 7
    assert two_pose_pairs(obj, view) == [(0, 5), (1, 4), (2, 8), (3, 6)]
    with pytest.raises(ValueError, match="view indices"):
        two_pose_pairs([0, 0, 0], [0, 1])
    # the pairs keep working with parts_for_pairs: a pair straddling parts merges them
    assert parts_for_pairs([(0, 5), (5, 9)], two_pose_pairs(obj, view)) == [(0, 9)]
    assert parts_for_pairs([(0, 2), (2, 4)], two_pose_pairs([0, 0, 0, 0], [0, 0, 1, 1])) == [(0, 2), (2, 4)]


def test_views_and_track_views_refusals_without_device():
    from foundationpose_amd import _lib, ops
    from foundationpose_amd.estimater import track_views
    K = np.eye(3)
    with pytest.raises(_lib.FpAmdError, match="need V >= 1"):
        ops.Views([], None, "cpu")
    with pytest.raises(_lib.FpAmdError, match="3x3"):
        ops.Views([np.eye(2)], None, "cpu")
    with pytest.raises(_lib.FpAmdError, match="2 views need a per-hypothesis view index"):
        ops.Views([K, K], None, "cpu")
    with pytest.raises(_lib.FpAmdError, match="outside 0..1"):
        ops.Views([K, K], [0, 2], "cpu")
    with pytest.raises(_lib.FpAmdError, match="outside 0..1"):
        ops.Views([K, K], [-1, 0], "cpu")
    # the tables hold exactly the values the single-view paths pass (f64, and f64 -> f32)
    Kx = np.array([[600.3, 0.1, 320.7], [0, 601.9, 240.2], [0, 0, 1]])
    vt = ops.Views([K, Kx], [1, 0, 1], "cpu")
    assert vt.V == 2 and len(vt) == 3 and vt.K64.dtype.is_floating_point
    assert np.array_equal(vt.K64.numpy()[1], Kx.reshape(9)) and np.array_equal(vt.K32.numpy()[1], Kx.reshape(9).astype(np.float32))
    assert vt.dev.tolist() == [1, 0, 1] and vt.pairs == [(0, 2)]
    sub = vt.rows(1, 3)
    assert sub.dev.tolist() == [0, 1] and sub.V == 2

    class _Est:
        def __init__(self, refiner):
            self.refiner, self.pose_last, self.device = refiner, object(), "cpu"
    r = object()
    a, b = _Est(r), _Est(r)
    rgb, depth = np.zeros((4, 6, 3), np.uint8), np.zeros((4, 6), np.float32)
    with pytest.raises(ValueError, match="no estimators"):
        track_views([], [], [rgb], [depth], [K])
    with pytest.raises(ValueError, match="views frame 2, outside 0..1"):
        track_views([a, b], [0, 2], [rgb, rgb], [depth, depth], [K, K])
    with pytest.raises(ValueError, match="one H x W"):
        track_views([a, b], [0, 1], [rgb, np.zeros((5, 6, 3), np.uint8)], [depth, depth], [K, K])
    with pytest.raises(ValueError, match="one of each per view"):
        track_views([a, b], [0, 1], [rgb, rgb], [depth], [K, K])
    with pytest.raises(ValueError, match="listed twice"):
        track_views([a, a], [0, 1], [rgb, rgb], [depth, depth], [K, K])
    with pytest.raises(ValueError, match="share one refiner"):
        track_views([a, _Est(object())], [0, 1], [rgb, rgb], [depth, depth], [K, K])
    a.pose_last = None
    with pytest.raises(RuntimeError, match="estimator 0 is not registered"):
        track_views([a, b], [0, 1], [rgb, rgb], [depth, depth], [K, K])
