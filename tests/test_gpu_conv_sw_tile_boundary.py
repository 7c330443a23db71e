"""GPU: the tile boundaries of the shifted-window 3x3 convolution (csrc/conv_sw.hip): the prologue that sends a tile's first operand DMAs
ahead of everything else, and the residual epilogue that fetches the residual rows in groups under the transposition
(csrc/igemm_epilogue.h, ig_epilogue_spec).

 1. An image's output does not depend on where its tile starts.  The reduction order per output element is fixed by the k order, so the
    same images in reversed order -- every image at another tile phase: another q0, other row crossings, another clamp at the end of the
    tensor -- must return the same bits.  A wrong patch offset, fragment row or residual offset shows up here.
 2. Output and residual in DIFFERENT geometries through the interleaved residual fetch: the output written concat-style (bsplit, cgroup)
    and as tokens with the positional second output, the residual in the plain padded grid; held to amp_util.conv_amp_ref with the caps of
    tests/test_gpu_conv_sw16.py (the policy gate: equal up to summation-order flips).
 3. The launch leaves what it must not touch: the zero border, guard words in front of and behind the output, and the whole residual buffer
    with its guards.  Every launch of this file runs on guarded buffers and is checked for it.

Shapes: the smallest that reach the 512 x 128 tile (two whole tiles of rows), a ragged last tile and several channel tiles."""
import pytest
import torch
import torch.nn.functional as F

from amp_util import assert_equal_up_to_flips, conv_amp_ref, r16

pytestmark = pytest.mark.gpu

GUARD = 4096                       # halves in front of and behind a buffer (8 KiB: the buffer stays 16-byte aligned)
CANARY = -1234.0                   # fp16-exact, nothing a layer of these tests produces


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _guarded(shape, dev, fill=0.0):
    """-> (whole allocation, view of `shape` between two guards)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float16, device=dev)
    view = flat[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return flat, view


def _guards_intact(flat):
    return bool((flat[:GUARD] == CANARY).all()) and bool((flat[-GUARD:] == CANARY).all())


def _padded_into(view, x_nchw):
    view[:, 1:-1, 1:-1, :] = x_nchw.permute(0, 2, 3, 1).to(view.device)


def _bn(g, Cn):
    w, b = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g) * 0.1
    mean, var = torch.randn(Cn, generator=g) * 0.1, torch.rand(Cn, generator=g) + 0.5
    scale = w / torch.sqrt(var + 1e-5)
    return scale, b - mean * scale


def _bits(t):
    return t.contiguous().view(torch.int16)


def _layer(B, H, Cin, Cout, seed):
    """fp16-valued operands of one residual BatchNorm layer (CPU, fp32)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = F.relu(r16(torch.randn((B, Cin, H, H), generator=g) * 0.5))
    w = r16(torch.randn((Cout, Cin, 3, 3), generator=g) * (1.0 / (3 * Cin ** 0.5)))
    bias = r16(torch.randn(Cout, generator=g) * 0.1)
    sb = _bn(g, Cout)
    r = r16(torch.randn((B, Cout, H, H), generator=g) * 0.5)
    return g, x, w, bias, sb, r


def _launch(dev, x, w, bias, sb, r, gout, yshape, wt=False, pe=None, relu=True):
    """one guarded launch; x, r: (B, C, H, H) fp16-valued.  Checks the guards and that the residual buffer is left as it was.
    -> (y, y_pe or None)"""
    from foundationpose_amd import ops
    B, Cin, H, _ = x.shape
    Cout = w.shape[0]
    G = ops.IgemmGeom.image
    xf, xb = _guarded((B, H + 2, H + 2, Cin), dev)
    rf, rb = _guarded((B, H + 2, H + 2, Cout), dev)
    _padded_into(xb, x.half())
    _padded_into(rb, r.half())
    r_before = rf.clone()
    wk = w.half().permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().to(dev)
    tiles = ops.pack_conv3x3_tiles(wk, Cout, Cin) if wt else None
    yf, y = _guarded(yshape, dev)
    pf = y_pe = None
    if pe is not None:
        pf, y_pe = _guarded(yshape, dev, fill=-7.0)
    ops.igemm_f16(xb, G(H, H, 1, Cin, stride=1, offset=0), wk, bias.to(dev), y, gout, B * H * H, Cout, Cin, 9, relu=relu, residual=rb,
                  r_geom=G(H, H, 1, Cout), bn_scale=sb[0].to(dev), bn_shift=sb[1].to(dev), conv_rounding=True, pe=pe, y_pe=y_pe, w_tiles=tiles)
    torch.cuda.synchronize()
    assert _guards_intact(yf), "the launch wrote in front of or behind the output"
    assert pf is None or _guards_intact(pf), "the launch wrote in front of or behind the second output"
    assert torch.equal(_bits(rf), _bits(r_before)), "the launch changed the residual buffer or its guards"
    assert _guards_intact(xf)
    return y, y_pe


def _border_is_zero(y):
    return all(float(t.abs().max()) == 0 for t in (y[:, 0], y[:, -1], y[:, :, 0], y[:, :, -1]))


# (B, H, C): 128 -> 128 at 40 x 40, B = 4: 6400 rows = 12 whole 512-row tiles and a ragged one of 256;
#            512 -> 512 at 20 x 20, B = 6: 2400 rows = 4.7 pixel tiles x 4 channel tiles (bn > 0, wpk_base, 16 channel chunks).
# Below 2 x 512 rows a launch takes another path, so B >= 4 / B >= 6 is what gives two whole tiles.
@pytest.mark.parametrize("wt", [False, True], ids=["plain", "tile-packed"])
@pytest.mark.parametrize("B,H,C", [(4, 40, 128), (6, 20, 512)])
def test_output_does_not_depend_on_the_tile_phase(dev, B, H, C, wt):
    from foundationpose_amd import ops
    _, x, w, bias, sb, r = _layer(B, H, C, C, 97 * B + C + H)
    gout = ops.IgemmGeom.image(H, H, 1, C)
    yshape = (B, H + 2, H + 2, C)
    y0, _ = _launch(dev, x, w, bias, sb, r, gout, yshape, wt)
    y1, _ = _launch(dev, x.flip(0), w, bias, sb, r.flip(0), gout, yshape, wt)
    assert float(y0.float().abs().max()) > 0 and _border_is_zero(y0) and _border_is_zero(y1)
    for b in range(B):
        a, c = y0[b, 1:-1, 1:-1], y1[B - 1 - b, 1:-1, 1:-1]
        assert torch.equal(_bits(a), _bits(c)), f"image {b}: {int((_bits(a) != _bits(c)).sum())} of {a.numel()} values differ between the two tile phases"


# the caps of tests/test_gpu_conv_sw16.py (test_igemm_conv3x3_policy's): every rounding point of the sequence can flip independently (conv,
# + bias: 2.0; BatchNorm, a flip in front of it scaled by |scale| <= 2.1: 2.2; + identity: 1.0), at most 3 % of the elements
CAP_BN_RES, MAX_FRAC = 2.0 + 2.2 + 1.0, 0.03


@pytest.mark.parametrize("kind", ["concat", "tokens"])
def test_residual_and_output_in_different_geometries(dev, kind):
    """SHAPES["concat"] / SHAPES["tokens"] of tests/test_gpu_igemm_epilogue_modes.py"""
    from foundationpose_amd import ops
    B, H, C = (4, 40, 128) if kind == "concat" else (3, 20, 512)
    g, x, w, bias, sb, r = _layer(B, H, C, C, 31 * B + C + H + len(kind))
    ref, mag, slack = conv_amp_ref(x, w, bias, sb, 1, residual=r)
    G = ops.IgemmGeom.image
    if kind == "concat":
        # image b -> image b % 2 of the buffer, channels (b // 2) * C ...: rows of the second group lie below the tile's first row
        y, _ = _launch(dev, x, w, bias, sb, r, G(H, H, 1, 2 * C, bsplit=B // 2, cgroup=C), (B // 2, H + 2, H + 2, 2 * C))
        assert _border_is_zero(y)
        out = torch.stack([y[b % 2, 1:-1, 1:-1, (b // 2) * C:(b // 2 + 1) * C] for b in range(B)]).permute(0, 3, 1, 2).float().cpu()
    else:
        pe = (torch.randn((H * H, C), generator=g) * 0.5).to(dev)
        y, y_pe = _launch(dev, x, w, bias, sb, r, G(H, H, 0, C), (B, H * H, C), pe=pe)
        out = y.view(B, H, H, C).permute(0, 3, 1, 2).float().cpu()
        # the second output is one rounding of the first + the table row: exact given y
        want = (y.float() + pe[None]).half()
        assert torch.equal(_bits(y_pe), _bits(want)), f"{int((_bits(y_pe) != _bits(want)).sum())} values of the positional output differ"
    rep = assert_equal_up_to_flips(out.numpy(), ref.numpy(), mag.numpy(), max_frac=MAX_FRAC, max_ulps=CAP_BN_RES, what=f"conv_sw {kind}",
                                   slack=slack.numpy())
    print(f"conv_sw {kind} B{B} H{H} {C}->{C}: {rep}")


def test_launch_leaves_borders_guards_and_residual_alone(dev):
    """3 x 40 x 40, 128 -> 128: ten tiles, the last one ragged (4800 = 9 x 512 + 192: the generic body inside a layer-kind launch).  The
    output buffer starts from zero, and whole buffers are compared: everything outside the interiors is still what it was."""
    from foundationpose_amd import ops
    B, H, C = 3, 40, 128
    _, x, w, bias, sb, r = _layer(B, H, C, C, 4242)
    y, _ = _launch(dev, x, w, bias, sb, r, ops.IgemmGeom.image(H, H, 1, C), (B, H + 2, H + 2, C))       # guards and residual: in _launch
    assert _border_is_zero(y)
    inner = torch.zeros_like(y)
    inner[:, 1:-1, 1:-1] = y[:, 1:-1, 1:-1]
    assert torch.equal(_bits(inner), _bits(y))
    assert float(y.float().abs().max()) > 0 and bool(torch.isfinite(y.float()).all())
    # ... and without ReLU the interior has negative values: the launch wrote it, not the zero fill
    y2, _ = _launch(dev, x, w, bias, sb, r, ops.IgemmGeom.image(H, H, 1, C), (B, H + 2, H + 2, C), relu=False)
    assert _border_is_zero(y2) and float(y2.float().min()) < 0
    assert torch.equal(F.relu(y2.float()), y.float())            # as values: max(-0, 0) may be either zero
