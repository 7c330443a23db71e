"""CPU: registration in several camera streams -- argument errors of fp_mask_depth_stats and fp_replicate_segments_f16 reported
without a GPU, the refusals of register_views and refine_device that need no device, and the host function that cuts a segment
table into the pieces of each hypothesis sub-batch."""
import ctypes as C
import types

import numpy as np
import pytest

P16 = C.c_void_p(16)     # a made-up device address: every check below fails before anything is read


def test_new_entry_points_report_argument_errors_without_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    # mask statistics: depth, masks, view, V, M, H, W, min_depth, out
    assert lib.fp_mask_depth_stats(P16, P16, P16, 1, 0, 480, 640, 0.001, P16, None) == 0               # nothing to do
    assert lib.fp_mask_depth_stats(P16, P16, P16, 1, -1, 480, 640, 0.001, P16, None) == -1
    assert b"fp_mask_depth_stats: M < 0" in lib.fp_last_error()
    assert lib.fp_mask_depth_stats(P16, None, P16, 1, 3, 480, 640, 0.001, P16, None) == -1
    assert b"fp_mask_depth_stats: NULL tensor" in lib.fp_last_error()
    assert lib.fp_mask_depth_stats(P16, P16, P16, 0, 3, 480, 640, 0.001, P16, None) == -1
    assert b"fp_mask_depth_stats: bad frame size (V=0" in lib.fp_last_error()
    assert lib.fp_mask_depth_stats(P16, P16, None, 2, 3, 480, 640, 0.001, P16, None) == -1
    assert b"2 frames need a per-mask view index" in lib.fp_last_error()
    for bad in (0.0, -0.001, float("inf"), float("nan")):
        assert lib.fp_mask_depth_stats(P16, P16, P16, 1, 3, 480, 640, bad, P16, None) == -1
        assert b"min_depth must be positive and finite" in lib.fp_last_error()
    assert lib.fp_mask_depth_stats(P16, P16, P16, 1, 3, 65536, 65536, 0.001, P16, None) == -1
    assert b"H * W too large" in lib.fp_last_error()
    assert lib.fp_mask_depth_stats(P16, C.c_void_p(17), P16, 1, 3, 480, 640, 0.001, P16, None) == -1
    assert b"4-byte aligned" in lib.fp_last_error()
    # segmented replication: buf, offsets, segments, images, pixels, channels, pixel stride, image stride
    assert lib.fp_replicate_segments_f16(P16, P16, 0, 10, 100, 128, 256, 25600, None) == 0                # nothing to do
    assert lib.fp_replicate_segments_f16(P16, P16, -1, 10, 100, 128, 256, 25600, None) == -1
    assert b"negative size" in lib.fp_last_error()
    assert lib.fp_replicate_segments_f16(P16, None, 2, 10, 100, 128, 256, 25600, None) == -1
    assert b"fp_replicate_segments_f16: NULL tensor" in lib.fp_last_error()
    assert lib.fp_replicate_segments_f16(P16, P16, 11, 10, 100, 128, 256, 25600, None) == -1
    assert b"11 segments but 10 images" in lib.fp_last_error()
    assert lib.fp_replicate_segments_f16(P16, P16, 2, 10, 100, 100, 256, 25600, None) == -1
    assert b"multiples of 8" in lib.fp_last_error()
    assert lib.fp_replicate_segments_f16(P16, P16, 2, 10, 100, 128, 64, 25600, None) == -1               # pixel stride < channels
    assert b"bad strides" in lib.fp_last_error()
    assert lib.fp_replicate_segments_f16(P16, P16, 2, 10, 100, 128, 256, 2560, None) == -1               # images overlap
    assert b"bad strides" in lib.fp_last_error()
    assert lib.fp_replicate_segments_f16(C.c_void_p(24), P16, 2, 10, 100, 128, 256, 25600, None) == -1
    assert b"16-byte aligned" in lib.fp_last_error()


def test_segment_pieces_on_hand_made_tables():
    from foundationpose_amd.predict_pose_refine import segment_pieces
    off = [0, 3, 5, 9]                                       # segments of 3, 2 (exactly two rows) and 4
    assert segment_pieces(off, 0, 9) == [(0, 3), (3, 5), (5, 9)]
    # a segment straddling the part boundary: each part gets its piece of it, relative to its first row
    assert segment_pieces(off, 0, 4) == [(0, 3), (3, 4)]
    assert segment_pieces(off, 4, 9) == [(0, 1), (1, 5)]     # a one-row piece, then the last segment
    assert segment_pieces(off, 2, 7) == [(0, 1), (1, 3), (3, 5)]
    assert segment_pieces(off, 4, 5) == [(0, 1)]             # a part of one row
    assert segment_pieces(off, 5, 5) == []
    # empty segments take no rows and give no piece
    off2 = [0, 0, 2, 2, 2, 3, 3]
    assert segment_pieces(off2, 0, 3) == [(0, 2), (2, 3)]
    assert segment_pieces(off2, 1, 3) == [(0, 1), (1, 2)]
    # the pieces of consecutive parts tile the call
    from foundationpose_amd import ops
    lengths = [0, 1, 2, 31, 0, 252, 126, 2, 1]
    off3 = ops.Segments(lengths, "cpu").offsets
    total = int(off3[-1])
    for cut in ([0, total], [0, 100, total], [0, 1, 2, 3, 208, 300, total]):
        rows = []
        for a, b in zip(cut[:-1], cut[1:]):
            for s, e in segment_pieces(off3, a, b):
                assert 0 <= s < e <= b - a
                rows += list(range(a + s, a + e))
        assert rows == list(range(total))


def test_refine_device_refusals_without_device():
    import torch
    from foundationpose_amd import ops
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    stub = types.SimpleNamespace(plan=lambda: None)
    K = np.eye(3)
    poses = torch.zeros((4, 4, 4))
    vt = ops.Views([K, K], [0, 0, 1, 1], "cpu")
    with pytest.raises(ValueError, match="shared_translation \\(registration\\) is not supported with views"):
        PoseRefinePredictor.refine_device(stub, None, None, poses, None, 8, 8, None, None, 1, shared_translation=True, views=vt)
    with pytest.raises(ValueError, match="segments cover 5"):
        PoseRefinePredictor.refine_device(stub, None, None, poses, None, 8, 8, None, None, 1,
                                          shared_translation=ops.Segments([2, 3], "cpu"), views=vt)


class _Est:
    def __init__(self, refiner, scorer):
        self.refiner, self.scorer, self.device, self.glctx = refiner, scorer, "cpu", None


def test_register_views_refusals_without_device():
    from foundationpose_amd.estimater import register_views
    K = np.eye(3)
    r, s = object(), object()
    a, b = _Est(r, s), _Est(r, s)
    rgb, depth, m = np.zeros((4, 6, 3), np.uint8), np.zeros((4, 6), np.float32), np.ones((4, 6), np.uint8)
    two = dict(rgbs=[rgb, rgb], depths=[depth, depth], Ks=[K, K])
    with pytest.raises(ValueError, match="no estimators"):
        register_views([], [], [rgb], [depth], [K], [])
    with pytest.raises(ValueError, match="2 estimators but 1 view indices"):
        register_views([a, b], [0], ob_masks=[m, m], **two)
    with pytest.raises(ValueError, match="2 estimators but 1 masks"):
        register_views([a, b], [0, 1], ob_masks=[m], **two)
    with pytest.raises(ValueError, match="2 estimators but 3 object ids"):
        register_views([a, b], [0, 1], ob_masks=[m, m], ob_ids=[1, 2, 3], **two)
    with pytest.raises(ValueError, match="one of each per view"):
        register_views([a, b], [0, 1], [rgb, rgb], [depth], [K, K], [m, m])
    with pytest.raises(ValueError, match="one of each per view"):
        register_views([a, b], [0, 1], [rgb, rgb], [depth, depth], [K], [m, m])
    with pytest.raises(ValueError, match="views frame 2, outside 0..1"):
        register_views([a, b], [0, 2], ob_masks=[m, m], **two)
    with pytest.raises(ValueError, match="views frame -1, outside 0..1"):
        register_views([a, b], [-1, 0], ob_masks=[m, m], **two)
    with pytest.raises(ValueError, match="one H x W"):
        register_views([a, b], [0, 1], [rgb, np.zeros((5, 6, 3), np.uint8)], [depth, depth], [K, K], [m, m])
    with pytest.raises(ValueError, match="mask 1 has shape"):
        register_views([a, b], [0, 1], ob_masks=[m, m[:3]], **two)
    with pytest.raises(ValueError, match="listed twice"):
        register_views([a, a], [0, 1], ob_masks=[m, m], **two)
    with pytest.raises(ValueError, match="share one refiner"):
        register_views([a, _Est(object(), s)], [0, 1], ob_masks=[m, m], **two)
    with pytest.raises(ValueError, match="share one scorer"):
        register_views([a, _Est(r, object())], [0, 1], ob_masks=[m, m], **two)


def test_translation_from_stats_empty_cases():
    from foundationpose_amd.estimater import translation_from_stats
    K = np.array([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]])
    assert np.array_equal(translation_from_stats(K, [-1, -1, -1, -1], 0, np.nan, np.nan), np.zeros(3))
    assert np.array_equal(translation_from_stats(K, [3, 9, 4, 7], 0, np.nan, np.nan), np.zeros(3))
    c = translation_from_stats(K, [238, 242, 318, 322], 2, np.float32(0.5), np.float32(0.7))
    assert np.allclose(c, [0, 0, 0.6])
