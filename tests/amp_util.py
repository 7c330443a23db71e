"""Helpers of the fp16-policy parity tests: torch-CPU emulation of one op of the autocast sequence with explicit
roundings (same definitions as oracle/nets_amp.py), and the comparison "equal up to fp32-summation-order flips":
two fp32 accumulations of the same fp16 products differ in the last bits, so a value that lies within that distance
of an fp16 rounding boundary comes out one fp16 ulp apart (measured: ~0.3 % of the outputs of a 3x3 convolution,
tests/test_oracle_amp_golden.py).  Anything beyond one ulp of the LARGEST intermediate of the op, or more than a few
per cent of flipped elements, is a different arithmetic."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def r16(x):
    return x.to(torch.float16).to(torch.float32)


def ulp16(x):
    """fp16 ulp at the magnitude of x (np array or tensor -> np array)"""
    ax = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(ax)) - 10)


def flip_report(out, ref, mag=None, slack=None):
    """-> dict(frac mismatched, max error in ulps of `mag` (default: max(|out|,|ref|)), max abs).  `slack`: elementwise
    absolute error that fp32 accumulation itself may carry into the value BEFORE it is rounded (~1e-6 x sum |a_k b_k| for
    a dot product): a result that cancels to a small number has a tiny fp16 ulp but the full accumulation error."""
    out = np.asarray(out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    m = np.maximum(np.abs(out), np.abs(ref)) if mag is None else np.maximum(np.asarray(mag, dtype=np.float64), np.maximum(np.abs(out), np.abs(ref)))
    d = np.abs(out - ref)
    dd = d if slack is None else np.maximum(d - np.asarray(slack, dtype=np.float64), 0.0)
    return dict(frac=float(np.mean(d > 0)), max_ulps=float((dd / ulp16(m)).max()), max_abs=float(d.max()),
                rel_rms=float(np.sqrt(np.mean(d ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30)))


def assert_equal_up_to_flips(out, ref, mag=None, max_frac=0.03, max_ulps=1.0, what="", slack=None):
    rep = flip_report(out, ref, mag, slack)
    assert np.isfinite(np.asarray(out, dtype=np.float64)).all(), what
    assert rep["max_ulps"] <= max_ulps + 1e-6 and rep["frac"] <= max_frac, (what, rep)
    return rep


def conv_amp_ref(x16, w16, bias, bn, stride, residual=None, relu=True):
    """autocast op sequence of conv (+bias) (+eval BN as scale/shift) (+identity) (+ReLU) on fp16-valued fp32 tensors.
    bias: f32 (already fp16-representable) | None; bn: (scale, shift) | None.  -> (result, magnitude of the largest
    intermediate per element, fp32-accumulation slack per element).  The convolution itself is evaluated in float64
    (products of fp16 values are exact, and the CPU backend's float32 path may pick a Winograd algorithm for 3x3
    kernels whose error is far above an fp32 dot product's)."""
    pad = (w16.shape[-1] - 1) // 2
    acc = F.conv2d(x16.double(), w16.double(), None, stride=stride, padding=pad)
    slack = (1e-6 * F.conv2d(x16.double().abs(), w16.double().abs(), None, stride=stride, padding=pad)).float()
    y = r16(acc.float())
    mag = y.abs()
    if bias is not None:
        y = r16(y + bias[None, :, None, None])
        mag = torch.maximum(mag, y.abs())
    if bn is not None:
        y = r16(y * bn[0][None, :, None, None] + bn[1][None, :, None, None])
        mag = torch.maximum(mag, y.abs())
        slack = slack * bn[0].abs()[None, :, None, None]
    if residual is not None:
        mag = torch.maximum(mag, residual.abs())
        y = r16(y + residual)
        mag = torch.maximum(mag, y.abs())
    if relu:
        y = F.relu(y)
    return y, mag, slack


# the gate of fp_attention_f16_fwd / fp_attention_segments_f16_fwd against attention_blockwise_ref.  Measured on the MI355X over
# the 198 cases of tests/test_gpu_amp.py section 1 (S = 1..1000, H = 1, 4, 8, both score policies): at most 0.9 % of the outputs
# flipped, by at most 2 ulps of `mag`; the same model summed in fp32 on the CPU: 1.8 %, 1 ulp.  The nearest neighbouring policy
# (key blocks of 32) flips >= 8.4 % (tests/test_attention_model.py), the others 11-96 %.
ATT_GATE = dict(max_frac=0.03, max_ulps=3.0)


def _round_p(e, p_round):
    if p_round == "fp16":
        return e.to(torch.float16).to(e.dtype)
    if p_round == "bf16":
        return e.to(torch.bfloat16).to(e.dtype)
    assert p_round is None, p_round
    return e


def attention_blockwise_ref(qkv, n_heads, fp16_scores=False, block=64, dtype=torch.float64, p_round="fp16",
                            round_scores=True, drop_last=False, unmask_tail=False):
    """model of the arithmetic of fp_attention_f16_fwd (csrc/attention.hip): qkv (B, S, 3 D) fp16 values -> (out, mag, slack),
    each (B, S, D).  Evaluated in `dtype` (float64: the yardstick; float32: the same order of operations with fp32 sums).
      scores: default  q.k exact, 1/sqrt(hd) inside the exponent;
              fp16_scores  qs = fp16(fp32(q) * fp32(sqrt(1/hd))), s = fp16(qs.k);
      per query the keys are walked in blocks of `block` (the last one holds the remainder): running maximum m, the
      accumulators rescaled by alpha = exp(m_old - m_new) when it grows, P = fp16(exp(s - m)) into o += P v, the UNROUNDED
      exponentials into l; out = fp16(o / l).
    mag = sum(P |v|) / l: the ulp scale of the comparison.  slack: fp16_scores only -- a score whose fp32 accumulation
    (~1e-6 x sum |qs k|) can land on either side of an fp16 rounding boundary is one score ulp uncertain; slack bounds what
    that ulp moves the output by (dP (|v| + |out|) / l per such key).  The default policy has no rounding before the
    exponent and gets zero slack.
    Neighbouring policies, only to show that the gate rejects them: p_round "bf16" | None (P not rounded), round_scores=False,
    drop_last (the last key missing), unmask_tail (the last block padded to `block` keys with copies of the last key, as the
    kernel's clamped staging reads would give it unmasked)."""
    qkv = torch.as_tensor(qkv).float()
    Bn, S, D3 = qkv.shape
    D = D3 // 3
    hd = D // n_heads
    assert D == n_heads * hd and D3 == 3 * D, (qkv.shape, n_heads)
    q, k, v = (t.reshape(Bn, S, n_heads, hd).permute(0, 2, 1, 3) for t in qkv.split(D, dim=-1))   # (B, H, S, hd) fp32
    if fp16_scores:
        qs = r16(q * torch.tensor(math.sqrt(1.0 / hd), dtype=torch.float32))   # fp32 product, rounded to fp16
        acc = qs.to(dtype) @ k.to(dtype).transpose(-1, -2)
        s = r16(acc).to(dtype) if round_scores else acc
        scale = 1.0
        eps = 1e-6 * (qs.abs().double() @ k.abs().double().transpose(-1, -2))
        a64 = acc.double()
        marked = (r16(a64 - eps) != r16(a64 + eps)).double()
        su = torch.from_numpy(ulp16(s.double().numpy()))
    else:
        s = q.to(dtype) @ k.to(dtype).transpose(-1, -2)
        scale = 1.0 / math.sqrt(hd)
        marked = None
    s_all, vv = s, v.to(dtype)
    if drop_last:
        assert S >= 2
        s, vv = s[..., :S - 1], vv[..., :S - 1, :]
    Sk = s.shape[-1]
    if unmask_tail and Sk % block:
        pad = block - Sk % block
        s = torch.cat([s, s[..., -1:].expand(*s.shape[:-1], pad)], dim=-1)
        vv = torch.cat([vv, vv[..., -1:, :].expand(*vv.shape[:-2], pad, hd)], dim=-2)
        Sk += pad
    m = torch.full(s.shape[:-1], -math.inf, dtype=dtype)
    l = torch.zeros(s.shape[:-1], dtype=dtype)
    o = torch.zeros(s.shape[:-1] + (hd,), dtype=dtype)
    ma = torch.zeros_like(o)
    for k0 in range(0, Sk, block):
        sb = s[..., k0:k0 + block]
        mn = torch.maximum(m, sb.amax(dim=-1))
        alpha = torch.exp((m - mn) * scale)
        e = torch.exp((sb - mn[..., None]) * scale)
        p = _round_p(e, p_round)
        l = l * alpha + e.sum(dim=-1)
        o = o * alpha[..., None] + p @ vv[..., k0:k0 + block, :]
        ma = ma * alpha[..., None] + p @ vv[..., k0:k0 + block, :].abs()
        m = mn
    y = o / l[..., None]
    out = r16(y.float())
    mag = (ma / l[..., None]).float()
    if marked is None:
        slack = torch.zeros_like(out)
    else:
        s64 = s_all.double()
        pg = torch.exp(s64 - s64.amax(dim=-1, keepdim=True))                  # exponentials against the global maximum
        w = marked * pg * torch.expm1(su)                                      # what one score ulp moves each of them by
        slack = ((w @ v.double().abs() + w.sum(dim=-1, keepdim=True) * y.double().abs()) / pg.sum(dim=-1, keepdim=True)).float()
    heads = lambda t: t.permute(0, 2, 1, 3).reshape(Bn, S, D)
    return heads(out), heads(mag), heads(slack)


def attention_operands(B, S, H, dist, seed, hd=128):
    """(B, S, 3 H hd) fp16 values of the attention tests.  dist: "peaked" (x 1.5: a few keys carry a query), "diffuse"
    (x 0.5: every key carries weight), "late_max" (x 0.5 plus a shared direction in q and in the keys of the last 64-key
    block: every query's maximum lies in the final, possibly partial, block, so the alpha rescale runs at the tail)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((B, S, 3, H, hd), generator=g) * (1.5 if dist == "peaked" else 0.5)
    if dist == "late_max":
        u = torch.randint(0, 2, (H, hd), generator=g).float() * 2 - 1
        x[:, :, 0] += 0.5 * u
        x[:, (S - 1) // 64 * 64:, 1] += 0.5 * u
    else:
        assert dist in ("peaked", "diffuse"), dist
    return r16(x.reshape(B, S, 3 * H * hd))


def geodesic(Ra, Rb):
    """rotation angle of Ra Rb^T via atan2(sin, cos): well conditioned near 0, unlike arccos of a float32 trace"""
    D = Ra.astype(np.float64) @ Rb.astype(np.float64).transpose(0, 2, 1)
    s = 0.5 * np.linalg.norm(np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], 1), axis=1)
    c = (np.trace(D, axis1=1, axis2=2) - 1) / 2
    return np.arctan2(s, c)


def kendall_tau(a, b):
    """Kendall rank correlation of two score vectors (O(n^2), n = 252)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    sa = np.sign(a[:, None] - a[None, :])
    sb = np.sign(b[:, None] - b[None, :])
    n = len(a)
    return float((sa * sb).sum() / (n * (n - 1)))
