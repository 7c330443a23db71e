"""CPU: the host side of registering several objects in one call -- the ragged segment table (ops.Segments), the argument checks of
fp_attention_segments_f16_fwd (reported through fp_last_error before anything touches a GPU) and register_objects' preconditions."""
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)


def test_segments_offsets_and_bounds():
    from foundationpose_amd import ops
    seg = ops.Segments([3, 0, 5, 1], "cpu")
    assert seg.B == len(seg) == 4 and seg.total == 9 and seg.max_S == 5
    assert seg.offsets.tolist() == [0, 3, 3, 8, 9]
    assert seg.dev.tolist() == [0, 3, 3, 8, 9] and str(seg.dev.dtype) == "torch.int32"
    assert [seg.rows(k) for k in range(4)] == [(0, 3), (3, 3), (3, 8), (8, 9)]
    assert seg.row_ids().tolist() == [0, 0, 0, 2, 2, 2, 2, 2, 3]
    empty = ops.Segments([0, 0], "cpu")
    assert empty.total == 0 and empty.max_S == 0 and empty.row_ids().numel() == 0


def test_segments_validation():
    from foundationpose_amd import ops
    with pytest.raises(ValueError, match="negative"):
        ops.Segments([4, -1, 2], "cpu")
    with pytest.raises(ValueError, match="no segments"):
        ops.Segments([], "cpu")
    with pytest.raises(ValueError, match="integers"):
        ops.Segments([1.5, 2.0], "cpu")
    with pytest.raises(ValueError, match="int32"):
        ops.Segments([2 ** 30, 2 ** 30, 2 ** 30], "cpu")


def test_segmented_attention_argument_errors_are_reported_without_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(16)
    f = lib.fp_attention_segments_f16_fwd
    assert f(p, p, p, 2, 10, 4, 128, 2, None) == -1                      # unknown flag
    assert b"fp_attention_segments_f16_fwd" in lib.fp_last_error() and b"flags" in lib.fp_last_error()
    assert f(p, p, p, 2, 10, 4, 64, 0, None) == -1 and b"head_dim=64" in lib.fp_last_error()
    assert f(p, p, p, -1, 10, 4, 128, 0, None) == -1 and b"negative" in lib.fp_last_error()
    assert f(p, p, p, 2, -3, 4, 128, 0, None) == -1 and b"negative" in lib.fp_last_error()
    assert f(None, p, p, 2, 10, 4, 128, 0, None) == -1 and b"NULL" in lib.fp_last_error()
    assert f(p, p, None, 2, 10, 4, 128, 1, None) == -1 and b"NULL" in lib.fp_last_error()
    assert f(C.c_void_p(24), p, p, 2, 10, 4, 128, 0, None) == -1 and b"unaligned" in lib.fp_last_error()
    assert f(p, p, C.c_void_p(18), 2, 10, 4, 128, 0, None) == -1 and b"unaligned" in lib.fp_last_error()
    assert f(p, p, p, 2, 10, 0, 128, 0, None) == -1 and b"head count" in lib.fp_last_error()
    assert f(p, p, p, 0, 10, 4, 128, 1, None) == 0                        # nothing to do
    assert f(p, p, p, 3, 0, 4, 128, 1, None) == 0                         # every segment empty


def test_segmented_attention_binding_checks_shapes():
    import torch
    from foundationpose_amd import _lib, ops
    seg = ops.Segments([2, 3], "cpu")
    with pytest.raises(_lib.FpAmdError, match="CUDA"):
        ops.attention_f16_segments(torch.zeros((5, 3 * 512), dtype=torch.float16), seg, 4)


class _Est:
    """what register_objects reads before it touches a device"""

    def __init__(self, refiner, scorer):
        self.refiner, self.scorer = refiner, scorer


def test_register_objects_preconditions():
    from foundationpose_amd.estimater import register_objects
    r, s = object(), object()
    a, b = _Est(r, s), _Est(r, s)
    m = np.ones((4, 4), np.uint8)
    K = np.eye(3)
    with pytest.raises(ValueError, match="no estimators"):
        register_objects([], K, None, None, [])
    with pytest.raises(ValueError, match="masks"):
        register_objects([a, b], K, None, None, [m])
    with pytest.raises(ValueError, match="object ids"):
        register_objects([a, b], K, None, None, [m, m], ob_ids=[1])
    with pytest.raises(ValueError, match="one refiner"):
        register_objects([a, _Est(object(), s)], K, None, None, [m, m])
    with pytest.raises(ValueError, match="one scorer"):
        register_objects([a, _Est(r, object())], K, None, None, [m, m])
    with pytest.raises(ValueError, match="twice"):
        register_objects([a, b, a], K, None, None, [m, m, m])
