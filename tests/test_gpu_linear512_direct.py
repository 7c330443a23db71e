"""GPU: k_linear512_direct (csrc/linear_ln.hip), the in_proj kernel that stores its 32 x 32 accumulator tiles straight from the registers,
against the kernel it takes the launches of (k_linear512: the same call with direct_store=False and the plain pack).

The two kernels form the same dot products, accumulated in the same k order, and round f16(acc + bias) with the same statement; what differs
is which MFMA source holds the rows, and with it who owns which output element.  The ISA does not promise that an MFMA sums alike with its
sources exchanged, so the arms are held to EQUAL BITS here, over a guarded arena: poison in front of and behind the output, which must
still be there afterwards.

M in {1, 31, 128, 129, 261}: a single row, a partial row tile, one full tile (the unpredicated instantiation alone), a full tile and a
ragged one of one row, two full tiles and a ragged one.  N in {512, 1536, 3072}: one column block, block chaining, and the 12 bias pieces
fetched by 8 waves.  With and without bias and ReLU.  The entry point takes a dense (M, N) output only, so there is no strided case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = (1, 31, 128, 129, 256 + 5)
NS = (512, 1536, 3072)
GUARD = 4096
POISON = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


_OPERANDS = {}


def _operands(dev, N):
    """weight, bias, both packs and the largest input of one N, shared by the cases of that N and left unchanged"""
    if N not in _OPERANDS:
        from foundationpose_amd import ops
        g = torch.Generator(device="cpu").manual_seed(12 + N)
        w = (torch.randn((N, 512), generator=g) * 0.05).half().to(dev)
        b = (torch.randn((N,), generator=g) * 0.1).to(dev)
        x = torch.randn((max(MS), 512), generator=g).half().to(dev)
        _OPERANDS[N] = (w, b, x, ops.PackedLinear512(w), ops.PackedLinear512(w, direct=True))
    return _OPERANDS[N]


def _run(dev, x, pack, bias, relu, direct):
    from foundationpose_amd import ops
    M, N = int(x.shape[0]), pack.out_features
    arena = torch.full((M * N + 2 * GUARD,), POISON, dtype=torch.float16, device=dev)
    ops.linear512(x, pack, bias, relu=relu, out=arena[GUARD:GUARD + M * N].view(M, N), direct_store=direct)
    return arena.cpu().view(torch.int16).numpy()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_direct_store_returns_the_bits_of_the_lds_store(dev, M, N):
    w, b, x, plain, direct = _operands(dev, N)
    poison = np.full(GUARD, POISON, dtype=np.float16).view(np.int16)
    for bias in (b, None):
        for relu in (False, True):
            want = _run(dev, x[:M], plain, bias, relu, False)
            got = _run(dev, x[:M], direct, bias, relu, True)
            for name, a in (("lds", want), ("direct", got)):
                assert np.array_equal(a[:GUARD], poison) and np.array_equal(a[GUARD + M * N:], poison), (name, M, N, "guards")
            diff = np.flatnonzero(got != want)
            assert diff.size == 0, (M, N, bias is not None, relu, diff.size, divmod(int(diff[0]) - GUARD, N))
            out = want[GUARD:GUARD + M * N].view(np.float16)
            assert np.isfinite(out).all() and np.abs(out).max() > 0.5            # a product, not poison or zeros
            if relu:
                assert (out >= 0).all() and (out == 0).mean() > 0.2


def test_default_switch_runs_the_direct_kernel_from_either_pack(dev):
    """ops.linear512 without direct_store follows engine.LINEAR512_DIRECT_STORE and brings the pack into the order its kernel reads"""
    from foundationpose_amd import engine, ops
    w, b, x, plain, direct = _operands(dev, 1536)
    assert engine.LINEAR512_DIRECT_STORE is True and not plain.direct and direct.direct
    want = ops.linear512(x, plain, b, direct_store=False)
    for pack in (plain, direct):
        assert torch.equal(ops.linear512(x, pack, b), want)
        with engine.overrides(LINEAR512_DIRECT_STORE=False):
            assert torch.equal(ops.linear512(x, pack, b), want)
    assert plain.in_order(True).direct and plain.in_order(True) is plain.in_order(True) and plain.in_order(False) is plain


def test_a_launch_refuses_the_pack_of_the_other_kernel(dev):
    from foundationpose_amd import ops
    from foundationpose_amd._lib import FpAmdError
    w, b, x, plain, direct = _operands(dev, 512)
    with pytest.raises(FpAmdError, match="w_packed is in the row order of fp_pack_linear512_f16"):
        ops.linear512(x, plain, b, direct_store=True)
    with pytest.raises(FpAmdError, match="w_packed is in the row order of fp_pack_linear512_direct_f16"):
        ops.linear512(x, direct, b, direct_store=False)
    # the row-owning fused kernels read the plain order only
    gm, bt = torch.ones(512, device=dev), torch.zeros(512, device=dev)
    with pytest.raises(FpAmdError, match="row order of linear512's direct-store kernel"):
        ops.linear_layernorm_res(x, direct, b, gm, bt, x32=x.float())
    with pytest.raises(FpAmdError, match="row order of linear512's direct-store kernel"):
        ops.ffn_layernorm_mean(x[:256].reshape(1, 256, 512), plain, b, direct, b, x[:256].float().reshape(1, 256, 512), gm, bt)


def test_direct_pack_is_the_plain_pack_of_the_row_permuted_matrix(dev):
    """include/fp_amd.h: within every group of 64 output channels, packed row 32 i + c holds weight row 2 c + i"""
    from foundationpose_amd import ops
    w = _operands(dev, 1536)[0]
    r = np.arange(64)
    src = 2 * (r % 32) + r // 32                                                  # the weight row that stands in place r of a group
    rows = np.arange(1536)
    perm = torch.as_tensor(rows // 64 * 64 + src[rows % 64], device=dev)
    want = ops.PackedLinear512(w[perm].contiguous()).data
    got = ops.PackedLinear512(w, direct=True).data
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not torch.equal(got.view(torch.int16), ops.PackedLinear512(w).data.view(torch.int16))
