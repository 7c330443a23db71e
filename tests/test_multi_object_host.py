"""CPU: the crop stage with an object table (several objects per refine call) -- argument errors of the C ABI, reported without a GPU,
the per-object grouping of the two-pose quirk on hand-made object indices, and track_objects' refusals that need no device."""
import ctypes as C

import numpy as np
import pytest


def _fake_mesh(lib, V, T):
    """an fp_mesh descriptor over made-up device addresses (fp_mesh_create only records them)"""
    h = C.c_void_p()
    assert lib.fp_mesh_create(C.c_void_p(16), C.c_void_p(32), C.c_void_p(48), None, None, None, C.c_void_p(64), V, T, 0, 0,
                              C.byref(h)) == 0
    return h


def test_mesh_set_argument_errors_are_reported_without_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    s = C.c_void_p()
    m1, m2 = _fake_mesh(lib, 100, 200), _fake_mesh(lib, 40000, 70000)
    try:
        arr = (C.c_void_p * 2)(m1.value, m2.value)
        assert lib.fp_mesh_set_create(arr, 0, C.byref(s)) == -1 and b"empty set" in lib.fp_last_error()
        assert not s.value
        assert lib.fp_mesh_set_create(None, 2, C.byref(s)) == -1 and b"meshes is NULL" in lib.fp_last_error()
        assert lib.fp_mesh_set_create(arr, 2, None) == -1 and b"out is NULL" in lib.fp_last_error()
        holes = (C.c_void_p * 2)(m1.value, None)
        assert lib.fp_mesh_set_create(holes, 2, C.byref(s)) == -1 and b"mesh 1 is NULL" in lib.fp_last_error()
        huge = _fake_mesh(lib, 10, (1 << 26) + 1)
        try:
            assert lib.fp_mesh_set_create((C.c_void_p * 1)(huge.value), 1, C.byref(s)) == -1
            assert b"mesh 0 has V=10, T=67108865" in lib.fp_last_error()
        finally:
            lib.fp_mesh_destroy(huge)
        # a NULL set is refused by the render and sized as nothing
        P = C.c_void_p(16)
        render = lambda mesh, set_, obj, diam, flags, K=P, Ks=None, view=None, V=0: lib.fp_render_crops(
            mesh, set_, obj, diam, 0.0, P, None, K, Ks, view, V, 480, 640, 4, 160, 160, 0.8, 0.5, 0.001, flags, None, None, None, None,
            None, None, None, None, 0, None)
        assert render(None, None, None, None, 1) == -1
        assert b"NULL mesh set" in lib.fp_last_error() and b"and NULL mesh" in lib.fp_last_error()     # neither a mesh nor a set
        assert lib.fp_mesh_set_workspace_bytes(None, 4, 160, 160) == 0
        # both a mesh and a set (made-up set handle: refused before it is read)
        assert render(m1, P, None, None, 1) == -1 and b"both a mesh and a mesh set" in lib.fp_last_error()
        # the per-object diameter table: no diameters, no objects, obj NULL with several objects, unknown flags
        crop = lambda K, Ks, view, V, diam, obj, M: lib.fp_crop_windows(P, K, Ks, view, V, 0.0, diam, obj, M, 1.2, 160, 160, 4, P, P, None)
        assert crop(None, None, None, 0, None, P, 2) == -1
        assert b"fp_crop_windows: need the diameters" in lib.fp_last_error()
        assert crop(None, None, None, 0, P, None, 3) == -1
        assert b"obj is NULL but there are 3 objects" in lib.fp_last_error()
        # the camera: K and a view table, or neither
        assert crop(P, P, P, 2, P, P, 2) == -1 and b"fp_crop_windows: both K and a view table" in lib.fp_last_error()
        assert crop(None, None, None, 0, P, P, 2) == -1 and b"fp_crop_windows: neither K nor a view table" in lib.fp_last_error()
        assert lib.fp_warp_crops(None, None, None, None, None, None, None, 0, None, 0.0, P, None, 2, 1, 0, 480, 640, 4, 160, 160,
                                 None, None) == -1
        assert b"fp_warp_crops: obj is NULL" in lib.fp_last_error()
        assert lib.fp_warp_crops(None, None, None, None, None, None, None, 0, None, 0.0, P, None, 0, 1, 0, 480, 640, 4, 160, 160,
                                 None, None) == -1
        assert lib.fp_warp_crops(P, P, None, P, P, None, None, 0, P, 0.0, P, P, 2, 1, 7, 480, 640, 4, 160, 160, P, None) == -1
        assert b"fp_warp_crops: unknown mode 7" in lib.fp_last_error()
        assert lib.fp_pose_update(P, P, P, 0, 1, None, 0.35, 0.0, P, None, 4, 8, P, None, None, 0, None, None, None, 0, None, 0.0,
                                  None) == -1
        assert b"fp_pose_update: obj is NULL but there are 4 objects" in lib.fp_last_error()
        assert lib.fp_pose_update(P, P, P, 5, 1, None, 0.35, 0.0, P, P, 4, 8, P, None, None, 0, None, None, None, 0, None, 0.0,
                                  None) == -1
        assert b"fp_pose_update: unknown rot_rep 5" in lib.fp_last_error()
        # nothing to do
        assert lib.fp_pose_update(None, None, None, 0, 1, None, 0.35, 0.0, P, None, 1, 0, None, None, None, 0, None, None, None, 0,
                                  None, 0.0, None) == 0
        # a real set needs the device table; without a GPU its creation fails loudly, with one the render checks obj
        st = lib.fp_mesh_set_create(arr, 2, C.byref(s))
        if st != 0:
            assert b"fp_mesh_set_create: device table of 2 meshes" in lib.fp_last_error() and not s.value
        else:
            try:
                # sized by the largest V and T of the set; T > 65535: 32-bit triangle lists
                assert lib.fp_mesh_set_workspace_bytes(s, 4, 160, 160) == lib.fp_workspace_bytes(4, 40000, 70000, 160, 160)
                assert render(None, s, None, P, 1) == -1
                assert b"obj is NULL but the set has 2 meshes" in lib.fp_last_error()
                assert render(None, s, P, None, 1) == -1
                assert b"FP_FLAG_NORMALIZE_XYZ needs the diameters" in lib.fp_last_error()
                assert render(None, s, P, None, 0x10000) == -1
                assert b"unknown flag bits" in lib.fp_last_error()
            finally:
                lib.fp_mesh_set_destroy(s)
    finally:
        lib.fp_mesh_destroy(m1)
        lib.fp_mesh_destroy(m2)


@pytest.mark.parametrize("obj,pairs", [
    ([0, 1, 2, 0, 1, 2], [(0, 3), (1, 4), (2, 5)]),    # three objects interleaved, two hypotheses each
    ([0, 0], [(0, 1)]),                                # the single-object quirk: one object, exactly two poses
    ([0, 1], []),                                      # two objects x one hypothesis: never paired across objects
    ([3, 1, 3, 2, 2, 2], [(0, 2)]),                    # interleaved; object 2 has three hypotheses, object 1 one
    ([1, 0, 0, 1, 2], [(0, 3), (1, 2)]),
    ([], []),
])
def test_two_pose_pairs(obj, pairs):
    from foundationpose_amd.predict_pose_refine import two_pose_pairs
    assert two_pose_pairs(obj) == pairs


def test_parts_keep_quirk_pairs_together():
    from foundationpose_amd.predict_pose_refine import parts_for_pairs, two_pose_pairs
    parts = [(0, 32), (32, 64)]
    assert parts_for_pairs(parts, []) == parts
    assert parts_for_pairs(parts, [(0, 1), (32, 33)]) == parts
    assert parts_for_pairs(parts, [(31, 32)]) == [(0, 64)]         # a pair across the boundary: one part
    obj = [k for k in range(32) for _ in range(2)]                  # 32 objects x 2 hypotheses, object-major
    assert parts_for_pairs(parts, two_pose_pairs(obj)) == parts
    obj = list(range(32)) * 2                                       # the same interleaved: every pair straddles
    assert parts_for_pairs(parts, two_pose_pairs(obj)) == [(0, 64)]


class _Est:
    """what track_objects reads before it touches a device"""

    def __init__(self, refiner):
        self.refiner, self.pose_last, self.device = refiner, object(), "cpu"


def test_track_objects_refusals_without_device():
    """one broken rule per call; a stub has no mesh, so anything past the checks would raise AttributeError instead"""
    from foundationpose_amd.estimater import track_objects
    r = object()
    a, b = _Est(r), _Est(r)
    rgb, depth, K = np.zeros((4, 6, 3), np.uint8), np.zeros((4, 6), np.float32), np.eye(3)
    with pytest.raises(ValueError, match="track_objects: no estimators"):
        track_objects([], rgb, depth, K)
    with pytest.raises(ValueError, match="track_objects: the estimators must share one refiner"):
        track_objects([a, _Est(object())], rgb, depth, K)
    with pytest.raises(ValueError, match="track_objects: an estimator is listed twice"):
        track_objects([a, b, a], rgb, depth, K)
    b.pose_last = None
    with pytest.raises(RuntimeError, match="track_objects: estimator 1 is not registered"):
        track_objects([a, b], rgb, depth, K)
