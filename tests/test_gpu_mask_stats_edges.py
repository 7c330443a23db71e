"""GPU: fp_mask_depth_stats (k_mask_depth_stats of csrc/frame_ops.hip, a 1024-thread radix select) against the numpy restatement of
tests/mask_stats_model.py on the generated cases of tests/mask_stats_cases.py -- depth sets in which each digit of the select
decides, depths at and around min_depth, +inf medians, invalid depths of every kind, views outside the stack, frames whose rows are
not 4-byte aligned, mask words with only their last byte set (tests/test_mask_stats_cases_host.py shows on the CPU that every case
reaches its target and that the cases tell wrong variants from the right one).  All eight integers of every row, bit for bit.

A record of the run is merged into $FP_GEOMETRY_REPORT_DIR/pose_update_edges.json when that variable names a directory (nothing is
written otherwise); the record of the MI355X run is committed as profiles/pose_update_edges.json."""
import json
import os

import numpy as np
import pytest
import torch

import mask_stats_cases as mc
import mask_stats_model as mm

pytestmark = pytest.mark.gpu

CASES = mc.cases()
PAD = 4096
POISON = -7
REPORT = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("FP_GEOMETRY_REPORT_DIR")
    if REPORT and out:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "pose_update_edges.json")
        merged = {}
        if os.path.exists(path):
            try:
                with open(path) as f:
                    merged = json.load(f)
            except Exception:
                merged = {}
        merged.update(REPORT)
        with open(path, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)


def _run(c, dev, rows=None):
    """one launch over the case's masks (or over masks `rows`), `out` inside a poisoned arena -> ((M,8) int32, arena intact)"""
    import ctypes as C
    from foundationpose_amd import _lib, ops
    d = torch.as_tensor(c["depth"], device=dev)
    sel = slice(None) if rows is None else rows
    mk = torch.as_tensor(np.ascontiguousarray(c["masks"][sel]), device=dev)
    vw = None if c["view"] is None else torch.as_tensor(np.ascontiguousarray(c["view"][sel]), device=dev)
    V, H, W = d.shape
    M = int(mk.shape[0])
    buf = torch.full((M * 8 + 2 * PAD,), POISON, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    st = _lib.lib().fp_mask_depth_stats(p(d), p(mk), p(vw), V, M, H, W, float(c["min_depth"]), C.c_void_p(buf[PAD:].data_ptr()), ops._stream(d))
    _lib.check(st, "fp_mask_depth_stats")
    torch.cuda.synchronize()
    intact = bool((buf[:PAD] == POISON).all()) and bool((buf[PAD + M * 8:] == POISON).all())
    return buf[PAD:PAD + M * 8].view(M, 8).cpu().numpy(), intact


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_row_is_the_restatement_in_a_poisoned_arena(c, dev):
    """all eight integers of every row; guard words around `out` stay; a second call gives the same bits; and through
    ops.mask_depth_stats (the path the product takes) the same table"""
    from foundationpose_amd import ops
    ref = mm.mask_stats(c["depth"], c["masks"], c["view"], c["min_depth"])
    out, intact = _run(c, dev)
    assert intact, "a write outside out"
    bad = np.flatnonzero((out != ref).any(axis=1))
    REPORT.setdefault("mask_depth_stats", {})[c["name"]] = dict(rows=int(len(ref)), rows_that_differ=[int(b) for b in bad])
    assert bad.size == 0, (c["name"], [(int(b), out[b].tolist(), ref[b].tolist()) for b in bad[:5]])
    again, _ = _run(c, dev)
    assert np.array_equal(again, out)
    vw = None if c["view"] is None else torch.as_tensor(c["view"], device=dev)
    via_ops = ops.mask_depth_stats(torch.as_tensor(c["depth"], device=dev), torch.as_tensor(c["masks"], device=dev), vw, float(c["min_depth"]))
    assert np.array_equal(via_ops.cpu().numpy(), ref)


@pytest.mark.parametrize("name", ["frame_6x10", "frame_33x65", "frame_64x64", "m_70"])
def test_one_launch_over_all_masks_equals_per_mask_launches(name, dev):
    c = {c["name"]: c for c in CASES}[name]
    whole, _ = _run(c, dev)
    for m in range(len(c["masks"])):
        one, intact = _run(c, dev, rows=slice(m, m + 1))
        assert intact and np.array_equal(one[0], whole[m]), (name, m)


def test_misaligned_masks_are_refused_not_misread(dev):
    """H * W % 4 == 0 reads four mask bytes per load: a masks tensor one byte off a 4-byte boundary is an argument error"""
    from foundationpose_amd import _lib, ops
    c = {c["name"]: c for c in CASES}["frame_6x10"]
    M, H, W = c["masks"].shape
    assert (H * W) % 4 == 0
    raw = torch.zeros(M * H * W + 4, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 4 == 0
    off = raw[1:1 + M * H * W].view(M, H, W)
    off.copy_(torch.as_tensor(c["masks"], device=dev))
    assert off.is_contiguous() and off.data_ptr() % 4 == 1
    with pytest.raises(_lib.FpAmdError, match="4-byte aligned"):
        ops.mask_depth_stats(torch.as_tensor(c["depth"], device=dev), off, torch.as_tensor(c["view"], device=dev))
    # a frame whose H * W is no multiple of 4 is read byte by byte: any offset is fine there
    c = {c["name"]: c for c in CASES}["frame_33x65"]
    M, H, W = c["masks"].shape
    raw = torch.zeros(M * H * W + 4, dtype=torch.uint8, device=dev)
    off = raw[1:1 + M * H * W].view(M, H, W)
    off.copy_(torch.as_tensor(c["masks"], device=dev))
    out = ops.mask_depth_stats(torch.as_tensor(c["depth"], device=dev), off, torch.as_tensor(c["view"], device=dev))
    assert np.array_equal(out.cpu().numpy(), mm.mask_stats(c["depth"], c["masks"], c["view"], c["min_depth"]))
