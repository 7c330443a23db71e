"""GPU: the shifted-window 3x3 convolution (csrc/conv_sw.hip) on both MFMA shapes of its main loop -- v_mfma_f32_16x16x32_f16 (round 7,
engine.CONV_MFMA_16X16X32) and v_mfma_f32_32x32x16_f16 -- through ops.igemm_f16, the shape selected by the engine switch.  Each output
is held to the float64-accumulating emulation of the autocast sequence (amp_util.conv_amp_ref) with the caps of
tests/test_gpu_amp.py::test_igemm_conv3x3_policy: equal up to summation-order flips.  The two shapes sum a k-step's 32 products in
another order, so they differ from each other by such flips as well; the new shape may not flip MORE than the old one on the same
inputs, beyond what two independent draws of that flip fraction differ by at the tested element count."""
import math

import pytest
import torch
import torch.nn.functional as F

from amp_util import assert_equal_up_to_flips, conv_amp_ref, r16
# the parity report of tests/test_gpu_amp.py and the module fixture that writes (merges) it: autouse here as well
from test_gpu_amp import REPORT, _write_report  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _padded_nhwc(x_nchw, dev):
    B, Cc, H, W = x_nchw.shape
    buf = torch.zeros((B, H + 2, W + 2, Cc), dtype=torch.float16, device=dev)
    buf[:, 1:1 + H, 1:1 + W, :] = x_nchw.permute(0, 2, 3, 1).to(dev)
    return buf


def _bn(g, C):
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    mean, var = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    scale = w / torch.sqrt(var + 1e-5)
    return scale, b - mean * scale


# (B, H, C, residual, BatchNorm, tile-packed weights as well): the smallest shapes that reach every path of the kernel
#   3 x 40 x 40, 128 -> 128: ten 512 x 128 tiles, tiles crossing image rows and images, a ragged last tile (4800 = 9 x 512 + 192)
#   5 x 20 x 20, 512 -> 512: four channel tiles per pixel tile, 16 channel chunks, the 22-pixel padded width
#   1 x 8 x 8, 128 -> 128:   one partial tile with clamped rows (below two tiles of rows the call stays on the generic kernel: the
#                            switch must not change it)
#   2 x 40 x 40, 256 -> 256: plain and tile-packed weights, the two weight staging paths of the 512 x 128 tile
#   2 x 20 x 20, 256 -> 256: fewer than two 512-row tiles and N % 256 == 0: the 256 x 256 tile (four wave columns, plain weights)
CASES = [(3, 40, 128, True, True, False), (5, 20, 512, True, False, False), (1, 8, 128, True, True, False),
         (2, 40, 256, True, True, True), (2, 20, 256, True, True, False)]


@pytest.mark.parametrize("B,H,C,res,bn,packed", CASES)
def test_conv_sw_both_mfma_shapes_follow_the_policy(dev, B, H, C, res, bn, packed):
    from foundationpose_amd import engine, ops
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + C + H)
    x = F.relu(r16(torch.randn((B, C, H, H), generator=g) * 0.5))
    w = r16(torch.randn((C, C, 3, 3), generator=g) * (1.0 / (3 * C ** 0.5)) + torch.arange(C)[:, None, None, None] * 1e-5)
    bias = r16(torch.randn(C, generator=g) * 0.1)
    sb = _bn(g, C) if bn else None
    r = r16(torch.randn((B, C, H, H), generator=g) * 0.5) if res else None
    ref, mag, slack = conv_amp_ref(x, w, bias, sb, 1, residual=r)          # once per case, shared by every run below
    xb = _padded_nhwc(x.half(), dev)
    wk = w.half().permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous().to(dev)
    rb = _padded_nhwc(r.half(), dev) if res else None
    gin = ops.IgemmGeom.image(H, H, 1, C, stride=1, offset=0)
    gout = ops.IgemmGeom.image(H, H, 1, C)
    tiles = ops.pack_conv3x3_tiles(wk, C, C) if packed else None
    # the caps of test_igemm_conv3x3_policy: every rounding point of the sequence can flip independently (conv, + bias, BatchNorm,
    # + identity), and a flip before BatchNorm is scaled by |scale| <= 2.1 on its way out
    cap = (2.0 + (2.2 if bn else 0.0)) + (1.0 if res else 0.0)
    n = ref.numel()
    for wt, wname in ((None, "plain"),) + (((tiles, "tile-packed"),) if packed else ()):
        frac, outs = {}, {}
        for s16 in (False, True):
            y = torch.zeros((B, H + 2, H + 2, C), dtype=torch.float16, device=dev)
            with engine.overrides(CONV_MFMA_16X16X32=s16):
                ops.igemm_f16(xb, gin, wk, bias.to(dev), y, gout, B * H * H, C, C, 9, relu=True, residual=rb, r_geom=gout if res else None,
                              bn_scale=sb[0].to(dev) if bn else None, bn_shift=sb[1].to(dev) if bn else None, conv_rounding=True, w_tiles=wt)
            out = y[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float().cpu()
            shape = "16x16x32" if s16 else "32x32x16"
            rep = assert_equal_up_to_flips(out.numpy(), ref.numpy(), mag.numpy(), max_frac=0.03, max_ulps=cap,
                                           what=f"conv3x3 {shape} {wname}", slack=slack.numpy())
            print(f"conv_sw {shape} {wname} B{B} H{H} {C}->{C}: {rep}")
            REPORT.setdefault("kernel_flip_rates", {})[f"conv_sw mfma {shape} {wname} B{B} H{H} {C}->{C}"] = rep
            frac[s16], outs[s16] = rep["frac"], out
            assert float(y[:, 0].abs().max()) == 0 and float(y[:, :, 0].abs().max()) == 0      # the zero border stays zero
            assert float(y[:, -1].abs().max()) == 0 and float(y[:, :, -1].abs().max()) == 0
        # Flips are rare, near-independent events of probability p per element, so a measured fraction over n elements has the
        # binomial standard deviation sqrt(p (1 - p) / n), and the difference of two such draws sqrt(2) times that.  The new shape's
        # fraction may exceed the old one's by four of those (p from the OLD shape's measurement, at least one element in n).
        p = max(frac[False], 1.0 / n)
        bound = frac[False] + 4.0 * math.sqrt(2.0 * p * (1.0 - p) / n)
        print(f"   flip fractions: 32x32x16 {frac[False]:.3e}, 16x16x32 {frac[True]:.3e}, bound {bound:.3e} (n = {n})")
        assert frac[True] <= bound, (wname, frac, bound)
        if B * H * H < 2 * 256:       # not a shifted-window launch: the switch changes nothing
            assert torch.equal(outs[False], outs[True])
        if wt is not None:            # the two weight paths are the same convolution, on either shape
            for s16 in (False, True):
                assert torch.equal(outs[s16], plain[s16]), s16
        plain = outs


def test_mfma_shape_flags_exclude_each_other(dev):
    from foundationpose_amd import _lib, ops
    import ctypes as C
    ep = ops.IgemmEpilogue()
    ep.flags = ops.IGEMM_MFMA_16X16X32 | ops.IGEMM_MFMA_32X32X16
    G = ops.IgemmGeom.matrix(512)
    st = _lib.lib().fp_igemm_f16_fwd(C.c_void_p(16), C.byref(G), C.c_void_p(16), C.c_void_p(16), C.byref(G), 4, 128, 512, 1, C.byref(ep), None)
    assert st == -1 and b"exclude each other" in _lib.lib().fp_last_error()
