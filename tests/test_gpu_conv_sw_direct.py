"""GPU: k_conv_sw_direct (csrc/conv_sw.hip, csrc/igemm_epilogue.h ig_epilogue_direct), the 512 x 128 tile of the shifted-window 3x3
convolution stored straight from its accumulators, against the kernel it takes the launches of (k_conv_sw, the same launch with
direct_store=False) and against the policy's reference.

The two kernels form the same products in the same k order per output element and run the same epilogue statements; what differs is
which MFMA operand is the pixels.  The ISA does not promise that an MFMA sums alike with its operands exchanged; on the MI355X it was
measured to, on every launch of this file, so the two arms are held to EQUAL BITS over the whole allocation (guards and border included).
Each arm is also held to amp_util.conv_amp_ref with the caps of tests/test_gpu_conv_sw16.py.

Every launch runs on guarded buffers as in tests/test_gpu_conv_sw_tile_boundary.py: canaries in front of and behind output and residual,
a zero border that must stay zero, the residual buffer left as it was.

Shapes: 128 -> 128 at 40 x 40, B = 4 (6400 rows: twelve whole tiles and a ragged one of 256 rows), 256 -> 256 at 40 x 40, B = 2 (two channel
tiles), 512 -> 512 at 20 x 20, B = 6 (four channel tiles, sixteen channel chunks); the four layer kinds; plain and tile-packed weights."""
import numpy as np
import pytest
import torch

from amp_util import assert_equal_up_to_flips, conv_amp_ref
from test_gpu_conv_sw_tile_boundary import GUARD, _bits, _border_is_zero, _guarded, _guards_intact, _layer, _padded_into

pytestmark = pytest.mark.gpu

SHAPES = [(4, 40, 128), (2, 40, 256), (6, 20, 512)]
KINDS = [(False, False), (False, True), (True, False), (True, True)]          # (BatchNorm, residual)
MAX_FRAC = 0.03


def _cap(bn, res):
    """tests/test_gpu_conv_sw16.py: conv, + bias: 2.0; BatchNorm, a flip in front of it scaled by |scale| <= 2.1: 2.2; + identity: 1.0"""
    return 2.0 + (2.2 if bn else 0.0) + (1.0 if res else 0.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


_LAYERS, _REFS, _PACKS = {}, {}, {}


def _operands(B, H, C):
    """one layer per shape, shared by every test of the file and left unchanged"""
    key = (B, H, C)
    if key not in _LAYERS:
        _LAYERS[key] = _layer(B, H, C, C, 11 * B + C + H)[1:]
    return _LAYERS[key]


def _ref(B, H, C, bn, res):
    key = (B, H, C, bn, res)
    if key not in _REFS:
        x, w, bias, sb, r = _operands(B, H, C)
        _REFS[key] = conv_amp_ref(x, w, bias, sb if bn else None, 1, residual=r if res else None)
    return _REFS[key]


def _weights(dev, B, H, C):
    """-> (plain (C, 9 C) fp16, the pack of k_conv_sw, the pack of k_conv_sw_direct), built once per shape"""
    from foundationpose_amd import ops
    key = (B, H, C)
    if key not in _PACKS:
        w = _operands(B, H, C)[1]
        wk = w.half().permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous().to(dev)
        _PACKS[key] = (wk, ops.pack_conv3x3_tiles(wk, C, C), ops.pack_conv3x3_tiles_direct(wk, C, C))
    return _PACKS[key]


def _launch(dev, shape, bn, res, direct, packed, flip=False, gout=None, yshape=None, pe=None, w_tiles="match"):
    """one guarded launch of the shape's layer.  direct: the arm; packed: with the tile pack of that arm (w_tiles="old" / "direct" forces a
    layout).  Checks guards and residual.  -> (whole output allocation, output view, y_pe or None)"""
    from foundationpose_amd import ops
    B, H, C = shape
    x, w, bias, sb, r = _operands(B, H, C)
    if flip:
        x, r = x.flip(0), r.flip(0)
    wk, t_old, t_new = _weights(dev, B, H, C)
    G = ops.IgemmGeom.image
    xf, xb = _guarded((B, H + 2, H + 2, C), dev)
    _padded_into(xb, x.half())
    rf = rb = r_before = None
    if res:
        rf, rb = _guarded((B, H + 2, H + 2, C), dev)
        _padded_into(rb, r.half())
        r_before = rf.clone()
    gout = gout if gout is not None else G(H, H, 1, C)
    yf, y = _guarded(yshape or (B, H + 2, H + 2, C), dev)
    pf = y_pe = None
    if pe is not None:
        pf, y_pe = _guarded(yshape, dev, fill=-7.0)
    tiles, tiles_direct = None, False
    if packed:
        tiles_direct = direct if w_tiles == "match" else (w_tiles == "direct")
        tiles = t_new if tiles_direct else t_old
    ops.igemm_f16(xb, G(H, H, 1, C, stride=1, offset=0), wk, bias.to(dev), y, gout, B * H * H, C, C, 9, relu=True, residual=rb,
                  r_geom=G(H, H, 1, C) if res else None, bn_scale=sb[0].to(dev) if bn else None, bn_shift=sb[1].to(dev) if bn else None,
                  conv_rounding=True, pe=pe, y_pe=y_pe, w_tiles=tiles, direct_store=direct, w_tiles_direct=tiles_direct)
    torch.cuda.synchronize()
    assert _guards_intact(yf), "the launch wrote in front of or behind the output"
    assert pf is None or _guards_intact(pf), "the launch wrote in front of or behind the second output"
    assert rf is None or torch.equal(_bits(rf), _bits(r_before)), "the launch changed the residual buffer or its guards"
    assert _guards_intact(xf)
    return yf, y, y_pe


def _nchw(y):
    return y[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).float().cpu()


@pytest.mark.parametrize("bn,res", KINDS, ids=["conv", "conv-res", "bn", "bn-res"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-%dx%d-C%d" % (s[0], s[1], s[1], s[2]))
def test_direct_arm_returns_the_old_arms_bits_and_follows_the_policy(dev, shape, bn, res):
    ref, mag, slack = _ref(*shape, bn, res)
    outs = {}
    for packed in (False, True):
        for direct in (False, True):
            yf, y, _ = _launch(dev, shape, bn, res, direct, packed)
            assert _border_is_zero(y) and float(y.float().abs().max()) > 0
            outs[direct, packed] = yf
    old = outs[False, False]
    for key, yf in outs.items():
        ndiff = int((_bits(yf) != _bits(old)).sum())
        print(f"conv_sw direct={key[0]} packed={key[1]} {shape} bn={bn} res={res}: {ndiff} of {yf.numel()} values differ from the old arm, plain weights")
    for key, yf in outs.items():
        assert torch.equal(_bits(yf), _bits(old)), key
    B, H, C = shape
    y = outs[True, True][GUARD:-GUARD].view(B, H + 2, H + 2, C)
    rep = assert_equal_up_to_flips(_nchw(y).numpy(), ref.numpy(), mag.numpy(), max_frac=MAX_FRAC, max_ulps=_cap(bn, res),
                                   what=f"conv_sw direct {shape}", slack=slack.numpy())
    print(f"conv_sw direct {shape} bn={bn} res={res}: {rep}")


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "tile-packed"])
@pytest.mark.parametrize("shape", [(4, 40, 128), (6, 20, 512)], ids=["B4-40x40-C128", "B6-20x20-C512"])
def test_direct_output_does_not_depend_on_the_tile_phase(dev, shape, packed):
    """the same images in reversed order: every image at another tile phase (another q0, other row crossings, another place in the row
    tables, for (4, 40, 128) another share of the ragged tile): the same bits per image"""
    B = shape[0]
    _, y0, _ = _launch(dev, shape, True, True, True, packed)
    _, y1, _ = _launch(dev, shape, True, True, True, packed, flip=True)
    for b in range(B):
        a, c = y0[b, 1:-1, 1:-1], y1[B - 1 - b, 1:-1, 1:-1]
        assert torch.equal(_bits(a), _bits(c)), f"image {b}: {int((_bits(a) != _bits(c)).sum())} of {a.numel()} values differ between the two tile phases"


def test_direct_output_written_concat_style_with_the_residual_in_the_plain_grid(dev):
    """image b -> image b % 2 of the buffer, channels (b // 2) * C ...: rows of the second group lie below the tile's first row, and a
    pixel's 64 channels of a wave are half a 256-byte line of the wider buffer"""
    from foundationpose_amd import ops
    shape = B, H, C = (4, 40, 128)
    gout, yshape = ops.IgemmGeom.image(H, H, 1, 2 * C, bsplit=B // 2, cgroup=C), (B // 2, H + 2, H + 2, 2 * C)
    yf_new, y, _ = _launch(dev, shape, True, True, True, True, gout=gout, yshape=yshape)
    yf_old, _, _ = _launch(dev, shape, True, True, False, True, gout=gout, yshape=yshape)
    assert _border_is_zero(y)
    assert torch.equal(_bits(yf_new), _bits(yf_old))
    ref, mag, slack = _ref(*shape, True, True)
    out = torch.stack([y[b % 2, 1:-1, 1:-1, (b // 2) * C:(b // 2 + 1) * C] for b in range(B)]).permute(0, 3, 1, 2).float().cpu()
    rep = assert_equal_up_to_flips(out.numpy(), ref.numpy(), mag.numpy(), max_frac=MAX_FRAC, max_ulps=_cap(True, True), what="conv_sw direct concat",
                                   slack=slack.numpy())
    print(f"conv_sw direct concat: {rep}")


@pytest.mark.parametrize("N,Cin", [(128, 64), (256, 128), (512, 512)])
def test_direct_pack_equals_its_numpy_restatement(dev, N, Cin):
    """include/fp_amd.h: w_tiles[((bn * nk + s) * 128 + r) * 32 + 8 pc + e] = w[128 bn + rho(r)][tap * Cin + 32 cc + 8 (pc ^ ((r >> 2) & 3)) + e],
    s = 9 cc + tap -- compared chunk by chunk; and the old entry point still writes its own layout (rho = identity)"""
    from foundationpose_amd import ops
    from test_conv_sw_direct_model import rho
    g = torch.Generator(device="cpu").manual_seed(N + Cin)
    w = torch.randn((N, 9 * Cin), generator=g).half()
    got_new = ops.pack_conv3x3_tiles_direct(w.to(dev), N, Cin).cpu().view(torch.int16).numpy().reshape(N // 128, 9 * (Cin // 32), 128, 4, 8)
    got_old = ops.pack_conv3x3_tiles(w.to(dev), N, Cin).cpu().view(torch.int16).numpy().reshape(N // 128, 9 * (Cin // 32), 128, 4, 8)
    wn = w.view(torch.int16).numpy().reshape(N // 128, 128, 9, Cin // 32, 4, 8)          # [bn][row][tap][cc][chunk][e]
    r = np.arange(128)
    perm = np.array([rho(int(i)) for i in r])
    for pc in range(4):
        lc = pc ^ ((r >> 2) & 3)                                                          # the chunk LDS position pc of row r holds
        for name, got, src in (("direct", got_new, perm), ("old", got_old, r)):
            want = wn[:, src, :, :, lc, :]                                                # [row][bn][tap][cc][e]
            want = want.transpose(1, 3, 2, 0, 4).reshape(N // 128, 9 * (Cin // 32), 128, 8)   # [bn][s = 9 cc + tap][row][e]
            assert np.array_equal(got[:, :, :, pc, :], want), (name, pc)


def test_launcher_refuses_a_pack_of_the_other_layout(dev):
    from foundationpose_amd._lib import FpAmdError
    shape = (4, 40, 128)
    with pytest.raises(FpAmdError, match="w_tiles is in the layout"):
        _launch(dev, shape, True, True, True, True, w_tiles="old")          # k_conv_sw_direct, the pack of k_conv_sw
    with pytest.raises(FpAmdError, match="w_tiles is in the layout"):
        _launch(dev, shape, True, True, False, True, w_tiles="direct")      # k_conv_sw, the pack of k_conv_sw_direct
    # the flag without a pack
    from foundationpose_amd import _lib, ops
    import ctypes as C
    ep = ops.IgemmEpilogue()
    ep.flags = ops.IGEMM_W_TILES_DIRECT
    G = ops.IgemmGeom.matrix(512)
    st = _lib.lib().fp_igemm_f16_fwd(C.c_void_p(16), C.byref(G), C.c_void_p(16), C.c_void_p(16), C.byref(G), 4, 128, 512, 1, C.byref(ep), None)
    assert st == -1 and b"FP_IGEMM_W_TILES_DIRECT without w_tiles" in _lib.lib().fp_last_error()


def test_positional_kind_and_the_256_tile_stay_on_the_old_kernel(dev):
    """with the switch on and the pack of k_conv_sw -- which k_conv_sw_direct would refuse -- both launches run, and return the bits of the
    switch-off launch: the token layer (residual + positional second output) and a launch of fewer than two 512-row tiles with
    N % 256 == 0 (the 256 x 256 tile)"""
    from foundationpose_amd import ops
    shape = B, H, C = (6, 20, 512)
    g = torch.Generator(device="cpu").manual_seed(5)
    pe = (torch.randn((H * H, C), generator=g) * 0.5).to(dev)
    gout, yshape = ops.IgemmGeom.image(H, H, 0, C), (B, H * H, C)
    a = _launch(dev, shape, True, True, True, True, gout=gout, yshape=yshape, pe=pe, w_tiles="old")
    b = _launch(dev, shape, True, True, False, True, gout=gout, yshape=yshape, pe=pe, w_tiles="old")
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[2]), _bits(b[2]))
    assert float(a[1].float().abs().max()) > 0
    small = (2, 20, 256)                                                     # 800 rows
    a = _launch(dev, small, True, True, True, True, w_tiles="old")
    b = _launch(dev, small, True, True, False, True, w_tiles="old")
    assert torch.equal(_bits(a[0]), _bits(b[0])) and float(a[1].float().abs().max()) > 0
