"""GPU: the epilogue bodies fp_igemm_f16_fwd compiles per layer kind (csrc/igemm_epilogue.h ig_epilogue_spec, chosen by
igemm.hip ig_epilogue_mode) return the bits of the generic body, which reads the layer kind at run time.

Every launch runs twice, the two runs differing only in engine.overrides(SPECIALIZED_EPILOGUE=...), i.e. in FP_IGEMM_EPILOGUE_GENERIC,
and the WHOLE output buffer -- the zero border of a padded tensor included -- and the positional second output are compared bit for
bit (as int16: -0 and +0, and two NaNs, are different / equal as their bits are).  There is no tolerance to choose: the two bodies are
specified to do the same arithmetic in the same order.  Each shape runs over {bias, none} x {BatchNorm, none} x {residual, none} x
{ReLU, none}; the combinations the library has no body for run the generic one on both sides and must be equal all the more.

Shapes: the smallest that reach each kernel and path, after tests/test_gpu_conv_sw16.py."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from amp_util import r16

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


def _bn(g, Cn):
    w, b = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g) * 0.1
    mean, var = torch.randn(Cn, generator=g) * 0.1, torch.rand(Cn, generator=g) + 0.5
    scale = w / torch.sqrt(var + 1e-5)
    return scale, b - mean * scale


# name: (images, output height = width, Cin, Cout, stride, both MFMA shapes, kind)
#   sw128:    ten 512 x 128 tiles crossing image rows and images, a ragged last tile (4800 = 9 x 512 + 192: the generic body inside a
#             specialised launch)
#   sw512:    four channel tiles per pixel tile
#   sw256:    plain and tile-packed weights
#   sw256x256: fewer than two 512-row tiles, N % 256 == 0: the 256 x 256 tile
#   s2_64:    stride 2, 64 -> 128: k_igemm_f16<256, 128> (two workgroups per CU)
#   s2_256:   stride 2, 256 -> 512: k_igemm_pp<256, 256>
#   concat:   4 images written side by side along C into a 256-channel buffer of 2 (bsplit = 2, cgroup = 128): rows of the second
#             channel group lie BELOW the tile's first row in memory
#   tokens:   the token layer: output without border, positional table and second output
SHAPES = {
    "sw128": (3, 40, 128, 128, 1, True, "plain"),
    "sw512": (5, 20, 512, 512, 1, True, "plain"),
    "sw256": (2, 40, 256, 256, 1, True, "packed"),
    "sw256x256": (2, 20, 256, 256, 1, True, "plain"),
    "s2_64": (2, 40, 64, 128, 2, False, "plain"),
    "s2_256": (2, 20, 256, 512, 2, False, "plain"),
    "concat": (4, 40, 128, 128, 1, True, "concat"),
    "tokens": (3, 20, 512, 512, 1, True, "tokens"),
}


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("name", list(SHAPES))
def test_layer_kind_bodies_return_the_generic_bits(dev, name):
    from foundationpose_amd import engine, ops
    B, H, Cin, Cout, stride, both, kind = SHAPES[name]
    g = torch.Generator(device="cpu").manual_seed(sum(map(ord, name)) * 7 + Cin)
    Hin = H * stride
    x = F.relu(r16(torch.randn((B, Cin, Hin, Hin), generator=g) * 0.5))
    w = r16(torch.randn((Cout, Cin, 3, 3), generator=g) * (1.0 / (3 * Cin ** 0.5)))
    bias = r16(torch.randn(Cout, generator=g) * 0.1).to(dev)
    scale, shift = (t.to(dev) for t in _bn(g, Cout))
    r = r16(torch.randn((B, Cout, H, H), generator=g) * 0.5)
    xb = _padded_nhwc(x.half(), dev)
    rb = _padded_nhwc(r.half(), dev)
    wk = w.half().permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().to(dev)
    G = ops.IgemmGeom.image
    gin = G(H, H, 1, Cin, stride=stride, offset=0)
    gres = G(H, H, 1, Cout)
    pe = y_pe_shape = None
    if kind == "concat":
        gout, yshape = G(H, H, 1, 2 * Cout, bsplit=B // 2, cgroup=Cout), (B // 2, H + 2, H + 2, 2 * Cout)
    elif kind == "tokens":
        gout, yshape = G(H, H, 0, Cout), (B, H * H, Cout)
        pe = (torch.randn((H * H, Cout), generator=g) * 0.5).to(dev)
        y_pe_shape = yshape
    else:
        gout, yshape = G(H, H, 1, Cout), (B, H + 2, H + 2, Cout)
    weights = [None] + ([ops.pack_conv3x3_tiles(wk, Cout, Cin)] if kind == "packed" else [])

    def run(spec, s16, wt, has_bias, has_bn, has_res, relu):
        # a border the kernel has to leave alone: zero, as every product buffer; y_pe starts from a pattern the kernel must overwrite
        y = torch.zeros(yshape, dtype=torch.float16, device=dev)
        y_pe = torch.full(y_pe_shape, -7.0, dtype=torch.float16, device=dev) if y_pe_shape else None
        with engine.overrides(SPECIALIZED_EPILOGUE=spec, CONV_MFMA_16X16X32=s16):
            ops.igemm_f16(xb, gin, wk, bias if has_bias else None, y, gout, B * H * H, Cout, Cin, 9, relu=relu,
                          residual=rb if has_res else None, r_geom=gres if has_res else None, bn_scale=scale if has_bn else None,
                          bn_shift=shift if has_bn else None, conv_rounding=True, pe=pe, y_pe=y_pe, w_tiles=wt)
        return y, y_pe

    checked = 0
    for s16 in ((False, True) if both else (True,)):
        for wt in weights:
            for combo in range(16):
                flags = [bool(combo >> k & 1) for k in range(4)]       # bias, BatchNorm, residual, ReLU
                y0, p0 = run(False, s16, wt, *flags)
                y1, p1 = run(True, s16, wt, *flags)
                what = (name, "16x16x32" if s16 else "32x32x16", "packed" if wt is not None else "plain", flags)
                assert float(y0.float().abs().max()) > 0, what           # the launch wrote something
                assert torch.equal(_bits(y1), _bits(y0)), what
                if p0 is not None:
                    assert float((p0.float() + 7.0).abs().max()) > 0, what
                    assert torch.equal(_bits(p1), _bits(p0)), what
                checked += 1
    print(f"{name}: {checked} launches pairs equal bit for bit")


def test_generic_epilogue_flag_is_a_known_flag(dev):
    """both settings of the bit pass the flag check (the launches above run under _lib.check); the next free bit is still refused"""
    from foundationpose_amd import _lib, ops
    assert ops.IGEMM_EPILOGUE_GENERIC == 64
    Gm = ops.IgemmGeom.matrix(512)
    x = torch.zeros((128, 512), dtype=torch.float16, device=dev)
    wm = torch.zeros((128, 512), dtype=torch.float16, device=dev)
    y = torch.ones((128, 128), dtype=torch.float16, device=dev)
    Gy = ops.IgemmGeom.matrix(128)
    for flags, ok in ((0, True), (ops.IGEMM_EPILOGUE_GENERIC, True), (ops.IGEMM_EPILOGUE_GENERIC | 128, False)):
        ep = ops.IgemmEpilogue()
        ep.flags = flags
        st = _lib.lib().fp_igemm_f16_fwd(C.c_void_p(x.data_ptr()), C.byref(Gm), C.c_void_p(wm.data_ptr()), C.c_void_p(y.data_ptr()),
                                         C.byref(Gy), 128, 128, 512, 1, C.byref(ep), None)
        if ok:
            assert st == 0, (flags, _lib.lib().fp_last_error())
        else:
            assert st == -1 and b"unknown flags" in _lib.lib().fp_last_error()
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0
