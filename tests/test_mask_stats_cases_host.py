"""CPU: the numpy restatement of fp_mask_depth_stats (tests/mask_stats_model.py) on the generated cases of tests/mask_stats_cases.py.
It reproduces the torch statistics the GPU suite already trusts (_ref_stats of tests/test_gpu_register_views.py) and
guess_translation's centre; every case reaches the path it names; and each wrong reading of the definition changes an output on a
named case, so the same cases can tell a wrong kernel from the right one (tests/test_gpu_mask_stats_edges.py)."""
import types

import numpy as np
import pytest
import torch

import mask_stats_cases as mc
import mask_stats_model as mm

CASES = mc.cases()
BY_NAME = {c["name"]: c for c in CASES}
# the wrong variant -> the case that is there to catch it
CAUGHT_BY = dict(gt_min_depth="at_min_depth", nan_counted="invalid_and_three_valid", box_over_valid="n_3",
                 upper_median_only="two_values_even", ranks_over_box="frame_33x65")


def _rows(c, variant=None):
    return mm.mask_stats(c["depth"], c["masks"], c["view"], c["min_depth"], variant)


def test_cases_cover_what_the_issue_lists():
    assert len({c["name"] for c in CASES}) == len(CASES) and all(c["targets"] for c in CASES)
    assert {c["depth"].shape[1:] for c in CASES} >= set(mc.FRAMES)
    assert {len(c["masks"]) for c in CASES} >= {1, 12, 70}
    assert {float(c["min_depth"]) for c in CASES} == {float(np.float32(x)) for x in (0.001, 0.5, 1e-6)}
    assert any(c["view"] is None for c in CASES) and any(c["view"] is not None and c["view"].min() < 0 for c in CASES)
    assert any(c["view"] is not None and c["view"].max() >= c["depth"].shape[0] for c in CASES)
    assert any((c["depth"].shape[1] * c["depth"].shape[2]) % 4 == 0 and c["depth"].shape[2] % 4 for c in CASES)
    assert {int(v) for c in CASES for v in np.unique(c["masks"])} >= {0, 1, 128, 255}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_case_reaches_its_target(c):
    assert c["reach"](_rows(c)), c["targets"]


def test_restatement_is_the_torch_sort_and_guess_translation():
    """the rows with min_depth = 0.001 and a view inside the stack (the threshold and the frames _ref_stats and guess_translation
    know), bit for bit; the frames of 481 x 643 through three masks each (the torch reference is the slow side)"""
    from foundationpose_amd.estimater import FoundationPose, translation_from_stats
    from test_gpu_register_views import _ref_stats
    K = np.array([[572.4, 1.5, 25.1], [0, 573.6, 19.4], [0, 0, 1]])
    stub = types.SimpleNamespace(device=torch.device("cpu"))
    compared = 0
    for c in CASES:
        if c["min_depth"] != mc.MIN_DEPTH:
            continue
        box, n, lo, hi = mm.host(_rows(c))
        big = c["depth"].shape[1] * c["depth"].shape[2] > 100000
        for m in range(len(c["masks"])):
            v = 0 if c["view"] is None else int(c["view"][m])
            if not 0 <= v < len(c["depth"]) or (big and m % 5):
                continue
            d, mk = torch.as_tensor(c["depth"][v]), torch.as_tensor(c["masks"][m])
            rb, rn, rlo, rhi = _ref_stats(d, mk)
            assert list(box[m]) == rb and n[m] == rn, (c["name"], m)
            if rn:
                assert lo[m].view(np.int32) == rlo.view(np.int32) and hi[m].view(np.int32) == rhi.view(np.int32), (c["name"], m)
            else:
                assert np.isnan(lo[m]) and np.isnan(hi[m])
            with np.errstate(over="ignore", invalid="ignore"):
                ref = FoundationPose.guess_translation(stub, depth=d, mask=c["masks"][m], K=K)
                got = translation_from_stats(K, box[m], n[m], lo[m], hi[m])
            assert np.array_equal(got, ref, equal_nan=True), (c["name"], m, got, ref)
            compared += 1
    assert compared > 150


@pytest.mark.parametrize("variant", mm.VARIANTS)
def test_each_wrong_variant_changes_an_output_on_its_named_case(variant):
    c = BY_NAME[CAUGHT_BY[variant]]
    assert not np.array_equal(_rows(c, variant), _rows(c)), f"{variant} is not told apart by {c['name']}: {c['targets']}"


def test_out_of_range_view_and_empty_rows_are_the_header_s():
    c = BY_NAME["frame_6x10"]
    rows = _rows(c)
    for m, v in enumerate(c["view"]):
        if not 0 <= v < 3 or not c["masks"][m].any():
            assert rows[m].tolist() == [-1, -1, -1, -1, 0, mm.NAN_BITS, mm.NAN_BITS, 0]
