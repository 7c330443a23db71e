"""GPU: the 3x3 convolution k_conv_sw<512,128,4,true> (csrc/conv_sw.hip) with room beside its tiles -- at most 224 registers and an LDS
request that leaves a rasteriser strip's worth (tests/test_conv_sw_resources_host.py), so that light kernels of the other sub-batch
stream become resident on a CU that runs a conv tile.

1. Running beside them changes nothing: a conv with one tile for every CU on one stream, fp_render_crops + fp_warp_crops of 126
   hypotheses on another, launched together; every output equals, bit for bit, the output of the same call run alone.
2. It is still the same convolution: bit-equal to the 32x32x16 instantiation of the same kernel (engine.overrides(CONV_MFMA_16X16X32=0),
   eager launches), whose accumulators stay on the compiler's own register assignment, with and without a residual, at 128 and 256
   channels, on launches whose last tile is partial.  tests/test_gpu_conv_sw16.py and tests/test_gpu_amp.py hold both loops to the
   policy's gates."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _conv_case(dev, B, H, W, C, res, seed):
    """operands of one C -> C 3x3 convolution on B images of H x W in padded NHWC buffers, and a function that runs it into a new buffer"""
    from foundationpose_amd import ops
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.zeros((B, H + 2, W + 2, C), dtype=torch.float16)
    x[:, 1:-1, 1:-1] = torch.relu(torch.randn((B, H, W, C), generator=g) * 0.5).half()
    w = (torch.randn((C, 9 * C), generator=g) * (1.0 / (3 * C ** 0.5))).half()
    bias = torch.randn(C, generator=g) * 0.1
    r = torch.zeros_like(x)
    r[:, 1:-1, 1:-1] = (torch.randn((B, H, W, C), generator=g) * 0.5).half()
    x, w, bias, r = x.to(dev), w.to(dev), bias.to(dev), r.to(dev)
    gin, gout = ops.IgemmGeom.image(H, W, 1, C, stride=1, offset=0), ops.IgemmGeom.image(H, W, 1, C)

    def run(mfma16=None):
        y = torch.zeros_like(x)
        ops.igemm_f16(x, gin, w, bias, y, gout, B * H * W, C, C, 9, relu=True, residual=r if res else None, r_geom=gout if res else None,
                      conv_rounding=True, mfma16=mfma16)
        return y
    return run


# (B, H, W): M = B H W = 512 k + 37, a last tile of 37 rows.
#   k = 1 and 2 as the smallest such launches: 549 = 1 x 9 x 61 and 1061 = 1 x 1 x 1061 (a prime) pixels.  The 512 x 128 tile takes
#   launches of at least two full tiles whose patch fits its buffer, so of these two only 549 pixels at 256 channels reach the
#   shifted-window kernel at all (on its 256 x 256 tile); the others stay on the generic kernel, where the switch must change nothing.
#   k = 3 and 19 are the smallest launches with such a last tile that DO run k_conv_sw<512,128>: 1573 = 11 x 11 x 13 pixels (tiles
#   crossing image rows and images, the patch 752 of 768 rows long) and 9765 = 15 x 21 x 31.
PARTIAL = [(1, 9, 61), (1, 1, 1061), (11, 11, 13), (15, 21, 31)]


@pytest.mark.parametrize("B,H,W", PARTIAL)
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("res", [False, True])
def test_same_convolution_as_the_32x32x16_instantiation(dev, B, H, W, C, res):
    from foundationpose_amd import engine
    assert (B * H * W) % 512 == 37
    run = _conv_case(dev, B, H, W, C, res, seed=B * H * W + C)
    y16 = run()                                                   # the product's default: the 16x16x32 loop
    assert engine.CONV_MFMA_16X16X32
    with engine.overrides(CONV_MFMA_16X16X32=0):
        y32 = run()
    torch.cuda.synchronize()
    assert float(y16.abs().max()) > 0
    assert torch.equal(y16, y32), f"{int((y16 != y32).sum())} of {y16.numel()} elements differ"
    assert float(y16[:, 0].abs().max()) == 0 and float(y16[:, -1].abs().max()) == 0          # the zero border stays zero
    assert float(y16[:, :, 0].abs().max()) == 0 and float(y16[:, :, -1].abs().max()) == 0


def test_concurrent_results_equal_solo_results(dev, scene):
    from foundationpose_amd import ops
    from foundationpose_amd.Utils import make_mesh_tensors
    # stream A: 128 -> 128 on 2 x 82 images of 40 x 40: M = 262400 pixels, 513 tiles of 512 rows, so every one of the 256 CUs holds one
    conv = _conv_case(dev, 2 * 82, 40, 40, 128, True, seed=7)
    # stream B: render + warp of 126 hypotheses on the synthetic can
    N = 126
    gm = make_mesh_tensors(scene["mesh"], device=dev)
    K, diam = scene["K"], scene["diameter"]
    P = torch.as_tensor(scene["poses"][:N], device=dev)
    rgb = torch.as_tensor(scene["rgb"], device=dev).float().contiguous()
    depth = ops.bilateral_filter_depth(ops.erode_depth(torch.as_tensor(scene["depth"], device=dev)))
    xyz = ops.depth_to_xyz(depth, K, f64_internal=True)
    tf, bb = ops.crop_windows(P, K, diam, 1.2, (160, 160))
    ws = torch.empty(ops.workspace_bytes(N, int(gm["pos"].shape[0]), int(gm["faces"].shape[0])), dtype=torch.uint8, device=dev)

    def light():
        A = torch.zeros((N, 6, 160, 160), dtype=torch.float16, device=dev)
        Bc = torch.zeros((N, 6, 160, 160), dtype=torch.float16, device=dev)
        ops.render_crops(gm["_handle"], P, bb, K, scene["H"], scene["W"], (160, 160), diam, 0.001, True, want=("A",), A_out=A, workspace=ws)
        ops.warp_crops(rgb, xyz, None, tf, K, P, diam, ops.MODE_REFINE, normalize_xyz=True, out_hw=(160, 160), B_out=Bc)
        return A, Bc

    y_solo = conv()
    torch.cuda.synchronize()
    A_solo, B_solo = light()
    torch.cuda.synchronize()
    assert float(y_solo.abs().max()) > 0 and float(A_solo.abs().max()) > 0 and float(B_solo.abs().max()) > 0
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for rep in range(3):
        with torch.cuda.stream(sa):
            y = conv()
        with torch.cuda.stream(sb):
            A, Bc = light()
        torch.cuda.synchronize()
        assert torch.equal(y, y_solo), (rep, int((y != y_solo).sum()))
        assert torch.equal(A, A_solo), (rep, int((A != A_solo).sum()))
        assert torch.equal(Bc, B_solo), (rep, int((Bc != B_solo).sum()))
