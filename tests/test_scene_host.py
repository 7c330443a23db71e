"""Host: crops.Scene without a device -- rows / take cut the object index, the view table and the quirk pairs together, the diameter is
a float or the table, and the constructor refuses what refine_device and predict_objects refused."""
import itertools

import numpy as np
import pytest
import torch

N, M, V = 7, 3, 2


def _interleaved(k, seed):
    rng = np.random.default_rng(seed)
    idx = np.concatenate([np.arange(k), rng.integers(0, k, N - k)])
    rng.shuffle(idx)
    return idx.astype(np.int64)


@pytest.fixture(scope="module")
def call():
    from foundationpose_amd import ops
    from foundationpose_amd.crops import Scene
    from foundationpose_amd.predict_pose_refine import ObjectIndex, two_pose_pairs
    obj, view = _interleaved(M, 3), _interleaved(V, 4)
    vt = ops.Views([np.eye(3), 2 * np.eye(3)], view, "cpu")
    diam = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    pairs = two_pose_pairs(obj, view)
    assert pairs, "the seeds give at least one (view, object) group of exactly two rows"
    scene = Scene("mesh", diam, None, 480, 640, N, obj=ObjectIndex(obj, "cpu", view=view), views=vt, who="test")
    return dict(scene=scene, obj=obj, view=view, pairs=pairs, vt=vt, diam=diam)


def _same(s, obj, view):
    assert s.n == len(obj) and s.obj.dtype == torch.int32 and s.views.dev.dtype == torch.int32
    assert np.array_equal(s.obj.numpy(), obj) and np.array_equal(s.views.host, view) and np.array_equal(s.views.dev.numpy(), view)


def _pairs_by_hand(pairs, a, b):
    """what PairRows.pair_rows gives: the pairs whose first row lies in a..b, relative to a"""
    return [(i - a, j - a) for i, j in pairs if a <= i < b]


def test_rows_cut_object_index_view_table_and_pairs_together(call):
    s = call["scene"]
    _same(s, call["obj"], call["view"])
    assert s.pair_list == call["pairs"] and s.grouped
    for a, b in itertools.combinations(range(N + 1), 2):
        r = s.rows(a, b)
        _same(r, call["obj"][a:b], call["view"][a:b])
        assert r.obj.data_ptr() == s.obj[a:].data_ptr() and r.views.dev.data_ptr() == s.views.dev[a:].data_ptr()      # nothing copied
        assert r.mesh is s.mesh and r.diameter is s.diameter and r.views.K64 is s.views.K64 and (r.H, r.W) == (480, 640)
        want = _pairs_by_hand(call["pairs"], a, b)
        got = r.pairs
        assert (got is None and not want) or [tuple(p) for p in got.tolist()] == want, (a, b)
        for c, d in itertools.combinations(range(b - a + 1), 2):      # rows of rows
            rr = r.rows(c, d)
            _same(rr, call["obj"][a + c:a + d], call["view"][a + c:a + d])
            want = _pairs_by_hand(call["pairs"], a + c, a + d)
            assert (rr.pairs is None and not want) or [tuple(p) for p in rr.pairs.tolist()] == want, (a, b, c, d)


@pytest.mark.parametrize("idx", [[0, 0, 3, 3, 3], [6, 2, 4, 0], [5], list(range(N))], ids=["repeats", "out_of_order", "one", "all"])
def test_take_gathers_object_index_and_view_table(call, idx):
    s = call["scene"]
    t = s.take(idx)
    _same(t, call["obj"][idx], call["view"][idx])
    assert t.pairs is None and t.mesh is s.mesh and t.diameter is s.diameter and t.views.K32 is s.views.K32
    _same(s.take(idx, torch.as_tensor(idx)), call["obj"][idx], call["view"][idx])
    # take of a rows: indices into the rows
    r = s.rows(1, 6)
    sub = [i % 5 for i in idx]
    _same(r.take(sub), call["obj"][1:6][sub], call["view"][1:6][sub])


def test_plain_scene_and_diameter_form(call):
    from foundationpose_amd.crops import Scene
    s = Scene("mesh", np.float32(0.25), np.eye(3), 480, 640, 2)
    assert isinstance(s.diameter, float) and s.diameter == 0.25 and not s.grouped and s.pairs is None and s.pair_list == []
    r = s.rows(0, 1)
    assert r.obj is None and r.views is None and r.n == 1 and r.diameter == 0.25 and s.take([1, 1]).n == 2
    assert call["scene"].diameter is call["diam"] and call["scene"].rows(2, 4).diameter is call["diam"]      # the table, as given
    # a bare device index: no quirk rows of its own, and none borrowed from the views
    bare = Scene("mesh", call["diam"], None, 8, 8, N, obj=torch.as_tensor(call["obj"].astype(np.int32)), views=call["vt"])
    assert bare.grouped and bare.pairs is None and bare.pair_list == [] and np.array_equal(bare.rows(2, 5).obj.numpy(), call["obj"][2:5])
    # views alone: the quirk per view
    only = Scene("mesh", call["diam"], None, 8, 8, N, views=call["vt"])
    assert only.pair_list == call["vt"].pairs and only.rows(0, N).obj is None


def test_constructor_refusals(call):
    from foundationpose_amd import ops
    from foundationpose_amd.crops import Scene
    from foundationpose_amd.predict_pose_refine import ObjectIndex
    obj, view, vt, d = call["obj"], call["view"], call["vt"], call["diam"]
    with pytest.raises(ValueError, match="^refine_device: 7 poses but an object index of 6$"):
        Scene("mesh", d, None, 8, 8, N, obj=ObjectIndex(obj[:6], "cpu"), who="refine_device")
    with pytest.raises(ValueError, match="^predict_objects: views must be an ops.Views$"):
        Scene("mesh", d, None, 8, 8, N, views=view, who="predict_objects")
    with pytest.raises(ValueError, match="^predict_objects: 5 poses but a view index of 7$"):
        Scene("mesh", d, None, 8, 8, 5, views=vt, who="predict_objects")
    for bad in (ObjectIndex(obj, "cpu"), ObjectIndex(obj, "cpu", view=view[::-1])):
        with pytest.raises(ValueError, match="^refine_device: with views, the ObjectIndex must be built with view=views.host "
                                             "\\(the two-pose quirk is grouped per \\(view, object\\)\\)$"):
            Scene("mesh", d, None, 8, 8, N, obj=bad, views=vt, who="refine_device")
    # one view without an index counts as view 0 everywhere
    one = ops.Views([np.eye(3)], None, "cpu")
    assert Scene("mesh", d, None, 8, 8, N, obj=ObjectIndex(obj, "cpu", view=np.zeros(N)), views=one).views is one
    with pytest.raises(ValueError, match="must be built with view=views.host"):
        Scene("mesh", d, None, 8, 8, N, obj=ObjectIndex(obj, "cpu", view=view), views=one)
