"""CPU: the float64 model of the attention kernels' arithmetic (amp_util.attention_blockwise_ref) and the gate the GPU tests
hold fp_attention_f16_fwd / fp_attention_segments_f16_fwd to (amp_util.ATT_GATE, tests/test_gpu_amp.py section 1).  The gate
has to pass summation-order noise -- the same model evaluated with fp32 sums -- and reject every neighbouring policy: P held
in bf16 or not rounded, key blocks of 32 instead of 64, the global row maximum instead of the running one, fp16 scores left
unrounded, a dropped key, unmasked tail keys.  None of these changes is visible to an absolute bound of a few fp16 ulps of
the output."""
import functools
import math

import numpy as np
import pytest
import torch

from amp_util import ATT_GATE, assert_equal_up_to_flips, attention_blockwise_ref, attention_operands, flip_report
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

H = 4
DISTS = ("peaked", "diffuse", "late_max")


@functools.lru_cache(maxsize=None)
def _case(S, dist, fp16_scores):
    qkv = attention_operands(1, S, H, dist, seed=S)
    return (qkv,) + attention_blockwise_ref(qkv, H, fp16_scores=fp16_scores)


def test_attention_model_is_softmax_attention():
    """unrounded P in one block is softmax(q k^T / sqrt(hd)) v itself (before the output rounding)"""
    S = 70
    qkv = attention_operands(2, S, H, "peaked", seed=3)
    out, _, _ = attention_blockwise_ref(qkv, H, block=S, p_round=None)
    q, k, v = (qkv.double().reshape(2, S, 3, H, 128)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(128), dim=-1) @ v).permute(0, 2, 1, 3).reshape(2, S, H * 128)
    np.testing.assert_array_equal(out.numpy(), ref.float().half().float().numpy())


@pytest.mark.parametrize("S", [37, 64, 130])
def test_attention_model_with_one_block_is_the_flash_oracle(S):
    """block >= S: one maximum per row, the order of oracle.nets_amp.attention_flash (which sums in fp32)"""
    from oracle import nets_amp
    qkv = attention_operands(2, S, H, "peaked", seed=S + 1)
    ref, mag, _ = attention_blockwise_ref(qkv, H, block=max(S, 64))
    assert_equal_up_to_flips(nets_amp.attention_flash(qkv, H).numpy(), ref.numpy(), mag.numpy(), what=f"flash S={S}", **ATT_GATE)


@pytest.mark.parametrize("fp16_scores", [False, True])
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("S", [37, 65, 130, 400])
def test_attention_gate_accepts_fp32_summation_order(S, dist, fp16_scores):
    qkv, ref, mag, slack = _case(S, dist, fp16_scores)
    out32, _, _ = attention_blockwise_ref(qkv, H, fp16_scores=fp16_scores, dtype=torch.float32)
    assert_equal_up_to_flips(out32.numpy(), ref.numpy(), mag.numpy(), slack=slack.numpy(), what=(S, dist, fp16_scores), **ATT_GATE)


VARIANTS = {
    "p_bf16": dict(p_round="bf16"),
    "p_unrounded": dict(p_round=None),
    "block32": dict(block=32),
    "global_max": dict(block=1 << 20),
    "scores_unrounded": dict(round_scores=False),
    "last_key_dropped": dict(drop_last=True),
    "tail_unmasked": dict(unmask_tail=True),
}


# S = 130, 400: partial last blocks of 2 keys (the kernel's half block) and of 16 keys; the default policy has no score rounding
@pytest.mark.parametrize("variant,S,dist,fp16_scores", [
    (v, S, d, f) for v in VARIANTS for S in (130, 400) for d in DISTS for f in (False, True) if f or v != "scores_unrounded"])
def test_attention_gate_rejects_other_policies(variant, S, dist, fp16_scores):
    qkv, ref, mag, slack = _case(S, dist, fp16_scores)
    out, _, _ = attention_blockwise_ref(qkv, H, fp16_scores=fp16_scores, **VARIANTS[variant])
    rep = flip_report(out.numpy(), ref.numpy(), mag.numpy(), slack.numpy())
    # rejected with room to spare: at least twice the gate's fraction of deviating outputs, or twice its ulps
    assert rep["frac"] > 2 * ATT_GATE["max_frac"] or rep["max_ulps"] > 2 * ATT_GATE["max_ulps"], rep
