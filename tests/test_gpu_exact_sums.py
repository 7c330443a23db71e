"""GPU: the convolution and Linear kernels against the float64 reference of their rounding policy on exactly summable operands
(tests/exact_cases.py), element for element and without any allowance.

On these operands every fp32 partial sum is exact in any order -- inside an MFMA, across k-steps, across split-K pieces -- so the
accumulator is a known number and every rounding point of the policy is one round-to-nearest-even.  A mismatch is a kernel or wrapper
bug, never summation noise: the number of mismatching elements has to be 0, on every kernel path, in the ragged last tile, in every
split-K piece, in every band of the 7x7 kernel.  (tests/test_exact_cases_host.py shows on the CPU that the cases reject a wrong rounding,
a moved rounding point, a dropped tap, swapped taps or image sides, a padding or a k range off by one: each changes >= 1 % of a case.)

The WHOLE allocation of every output is compared with the expected one as values (-0 == +0; a NaN equals nothing) and must be finite:
outputs, second outputs and residuals live between canary guards, column blocks between canary columns, and guards, zero borders,
inputs and residuals must come back as they were.  A failure names case, kernel path and the first mismatching index.

Entry points: (a) fp_igemm_f16_fwd taps = 9 on every kernel path, (b) taps = 1, (c) fp_igemm_f16_splitk_fwd with uneven pieces,
(d) fp_conv7x7s2_bn_relu_fwd, (e) fp_linear512_f16_fwd, (f) fp_rows_linear_fwd, (g) fp_colmean_f16_fwd without LayerNorm.
LayerNorm, attention and the fused row kernels go through rsqrt / exp and cannot be exact: they stay with their statistical gates.

A record of the run is merged into $FP_EXACT_SUMS_REPORT_DIR/exact_sums.json when that variable names a directory (nothing is written
otherwise; committed as profiles/exact_sums.json): per case the entry point, shape, path, elements compared, mismatches, and the largest
sum of |products| in units of 2^-11."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import exact_cases as ec

pytestmark = pytest.mark.gpu

GUARD = 4096                       # elements in front of and behind a buffer (the buffer stays 16-byte aligned)
CANARY = -1234.0                   # fp16-exact, nothing a case produces
REPORT = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("FP_EXACT_SUMS_REPORT_DIR")
    if REPORT and out:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "exact_sums.json")
        merged = {}
        if os.path.exists(path):          # several pytest invocations (-k subsets) contribute to one report
            try:
                with open(path) as f:
                    merged = json.load(f)
            except Exception:
                merged = {}
        merged.update(REPORT)
        with open(path, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)


def _record(entry, case, shape, sum_abs):
    rec = dict(entry_point=entry, shape=shape, paths=[], launches=0, elements_compared=0, mismatches=0, largest_sum_abs_products_units=sum_abs)
    REPORT[f"{entry}: {case}"] = rec
    return rec


def _guarded(shape, dev, fill=0.0, dtype=torch.float16):
    """-> (whole allocation, view of `shape` between two guards)"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), CANARY, dtype=dtype, device=dev)
    view = flat[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.fill_(fill)
    return flat, view


def _t(a, dev, dtype=torch.float16):
    """float64 values that `dtype` holds exactly -> device tensor"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    assert np.array_equal(t.double().numpy(), a)
    return t.to(dev)


def _compare(rec, what, path, got, exp, shape=None):
    """got, exp: whole allocations.  Counts into the record first, then asserts: finite, and not one element off"""
    got, exp = got.flatten(), exp.flatten()
    bad = got != exp
    n = int(bad.sum())
    finite = bool(torch.isfinite(got).all())
    rec["launches"] += 1
    rec["elements_compared"] += got.numel()
    rec["mismatches"] += n
    if path not in rec["paths"]:
        rec["paths"].append(path)
    where = ""
    if n:
        first = int(bad.nonzero()[0]) - GUARD
        where = f", first at element {first} of the buffer"
        if shape is not None and 0 <= first < int(np.prod(shape)):
            where += f" = index {tuple(int(v) for v in np.unravel_index(first, shape))} of {tuple(shape)}"
        where += f": got {float(got[first + GUARD])}, expected {float(exp[first + GUARD])}"
        rec.setdefault("first_failure", f"{what} [{path}]{where}")
    assert finite, f"{what} [{path}]: non-finite values in the output"
    assert n == 0, f"{what} [{path}]: {n} of {got.numel()} elements differ from the reference{where}"


def _unchanged(flat, before, what):
    assert torch.equal(flat.view(torch.int16), before.view(torch.int16)), f"{what}: the launch changed a buffer it only reads, or its guards"


# ------------------------------------------------------------------ (a), (c): 3x3 convolutions
def _conv_path(c):
    """the kernel igemm.hip's dispatch picks for the case (a label for the report; the shapes are chosen for these paths)"""
    bm = 256 if c.Cout % 256 == 0 and c.M < 1024 else 512
    if c.stride == 1 and c.Wo >= 2 and c.M >= 2 * bm:
        return "k_conv_sw 256x256" if bm == 256 else "k_conv_sw 512x128"
    if c.stride == 2 and c.Cin <= 64:
        return "k_igemm_f16 256x128"
    if c.Cout % 256 == 0 and (c.Cout >= 1024 or c.Cin >= 256):
        return "k_igemm_pp 256x256"
    return "k_igemm_f16 128x128"


class _ConvRun:
    """device operands of one conv case in guarded buffers; layout "plain" | "cols" (input, output and residual as column blocks of
    wider buffers whose other columns are canaries) | "concat" (bsplit: image b -> image b % (B/2), channel group b // (B/2)) |
    "tokens" (output without border + the positional second output)"""

    def __init__(self, dev, c, case, layout="plain"):
        from foundationpose_amd import ops
        self.dev, self.c, self.case, self.layout, self.op = dev, c, case, layout, case["op"]
        op = self.op
        G = ops.IgemmGeom.image
        B, Ho, Wo, Cin, N = c.B, c.Ho, c.Wo, c.Cin, c.Cout
        Hin, Win = c.hw_in
        wide = layout == "cols"
        cs_in, co_in = (Cin + 72, 40) if wide else (Cin, 0)
        cs_res, co_res = (N + 24, 8) if wide else (N, 0)
        self.xf, xb = _guarded((B, Hin + 2, Win + 2, cs_in), dev, fill=CANARY)
        xb[..., co_in:co_in + Cin] = 0
        xb[:, 1:-1, 1:-1, co_in:co_in + Cin] = _t(op["ix"] * 2.0 ** -ec.X_EXP, dev)
        self.xb, self.gin = xb, G(Ho, Wo, 1, cs_in, stride=c.stride, offset=0, coff=co_in)
        assert (self.gin.padded_h, self.gin.padded_w) == (Hin + 2, Win + 2)
        self.rf, rb = _guarded((B, Ho + 2, Wo + 2, cs_res), dev, fill=CANARY)
        rb[..., co_res:co_res + N] = 0
        rb[:, 1:-1, 1:-1, co_res:co_res + N] = _t(op["res"], dev)
        self.rb, self.gres = rb, G(Ho, Wo, 1, cs_res, coff=co_res)
        self.x_before, self.r_before = self.xf.clone(), self.rf.clone()
        self.wk = _t((op["iw"] * 2.0 ** -ec.W_EXP).reshape(N, 9 * Cin), dev)
        self.packs = {}
        self.bias, self.scale, self.shift = (_t(op[k], dev, torch.float32) for k in ("bias", "scale", "shift"))
        self.pe = _t(op["pe"], dev, torch.float32) if layout == "tokens" else None
        if layout == "concat":
            self.yshape, self.gout = (B // 2, Ho + 2, Wo + 2, 2 * N), G(Ho, Wo, 1, 2 * N, bsplit=B // 2, cgroup=N)
        elif layout == "tokens":
            self.yshape, self.gout = (B, Ho * Wo, N), G(Ho, Wo, 0, N)
        elif wide:
            self.yshape, self.gout = (B, Ho + 2, Wo + 2, N + 136), G(Ho, Wo, 1, N + 136, coff=64)
        else:
            self.yshape, self.gout = (B, Ho + 2, Wo + 2, N), G(Ho, Wo, 1, N)
        self.refs = {}

    def pack(self, kind):
        from foundationpose_amd import ops
        if kind is not None and kind not in self.packs:
            fn = ops.pack_conv3x3_tiles_direct if kind == "direct" else ops.pack_conv3x3_tiles
            self.packs[kind] = fn(self.wk, self.c.Cout, self.c.Cin)
        return self.packs.get(kind)

    def fresh_output(self):
        """-> (allocation, view, expected allocation before the reference goes in): zero where the product keeps a zero border,
        canaries in the columns of a wide buffer that are not the launch's"""
        c = self.c
        yf, y = _guarded(self.yshape, self.dev, fill=CANARY if self.layout == "cols" else 0.0)
        if self.layout == "cols":
            y[..., 64:64 + c.Cout] = 0
        return yf, y

    def expected(self, yf, y, flags):
        """the allocation as it has to come back: as it is now, the reference in the interior"""
        c = self.c
        if flags not in self.refs:
            ref = ec.conv_epilogue(self.case["A"], self.op, *flags)
            self.refs[flags] = (_t(ref, self.dev), _t(ec.pe_output(ref.reshape(c.M, c.Cout), self.op["pe"]), self.dev) if self.pe is not None else None)
        ref, ref_pe = self.refs[flags]
        ef = yf.clone()
        e = ef[GUARD:GUARD + y.numel()].view(self.yshape)
        if self.layout == "concat":
            half = c.B // 2
            for b in range(c.B):
                e[b % half, 1:-1, 1:-1, (b // half) * c.Cout:(b // half + 1) * c.Cout] = ref[b]
        elif self.layout == "tokens":
            e[:] = ref.reshape(self.yshape)
        elif self.layout == "cols":
            e[:, 1:-1, 1:-1, 64:64 + c.Cout] = ref
        else:
            e[:, 1:-1, 1:-1, :] = ref
        return ef, ref_pe

    def launch(self, rec, flags, path, s16=True, wt=None, direct=False, splits=None, fill=0x7f):
        """one launch on fresh guarded outputs, compared whole; -> the output allocation"""
        from foundationpose_amd import ops
        c = self.c
        bias, bn, res, relu = flags
        yf, y = self.fresh_output()
        ef, ref_pe = self.expected(yf, y, flags)
        pf = y_pe = None
        if self.pe is not None:
            pf, y_pe = _guarded((c.M, c.Cout), self.dev, fill=-7.0)
        kw = dict(relu=relu, residual=self.rb if res else None, r_geom=self.gres if res else None, bn_scale=self.scale if bn else None,
                  bn_shift=self.shift if bn else None, conv_rounding=True, pe=self.pe, y_pe=y_pe)
        b = self.bias if bias else None
        if splits is None:
            ops.igemm_f16(self.xb, self.gin, self.wk, b, y, self.gout, c.M, c.Cout, c.Cin, 9, w_tiles=self.pack(wt), mfma16=s16,
                          direct_store=direct, w_tiles_direct=wt == "direct", **kw)
        else:
            need = ops.igemm_splitk_workspace_bytes(c.M, c.Cout, splits)
            ws = torch.full((need + 64,), fill, dtype=torch.uint8, device=self.dev)       # NaN patterns: every word that is read has been written
            ops.igemm_f16_splitk(self.xb, self.gin, self.wk, b, y, self.gout, c.M, c.Cout, c.Cin, 9, splits, ws[:need], **kw)
            assert bool((ws[need:] == fill).all()), f"{c.name} x{splits}: wrote past the workspace"
        torch.cuda.synchronize()
        what = f"{c.name} (bias, BatchNorm, residual, ReLU) = {flags}"
        _compare(rec, what, path, yf, ef, self.yshape)
        if pf is not None:
            epf = pf.clone()
            epf[GUARD:GUARD + y_pe.numel()] = ref_pe.flatten()
            _compare(rec, what + " second output", path, pf, epf, (c.M, c.Cout))
        _unchanged(self.xf, self.x_before, what + " input")
        _unchanged(self.rf, self.r_before, what + " residual")
        return yf


def _conv_record(c, case, entry="fp_igemm_f16_fwd taps=9"):
    return _record(entry, c.name, dict(B=c.B, Ho=c.Ho, Wo=c.Wo, Cin=c.Cin, Cout=c.Cout, stride=c.stride, M=c.M, K=9 * c.Cin), case["sum_abs"])


def _mfma_and_store(c, both=True):
    """(MFMA shape 16x16x32?, direct store?) worth launching: the flags reach the shifted-window kernel only, the direct store its 512 x 128 tile"""
    path = _conv_path(c)
    if not path.startswith("k_conv_sw") or not both:
        return [(True, False)]
    return [(False, False), (True, False)] + ([(True, True)] if path.endswith("512x128") else [])


def _label(path, s16, wt, direct):
    if not path.startswith("k_conv_sw"):
        return path
    return f"{path} {'16x16x32' if s16 else '32x32x16'}{' tile-packed' if wt else ''}{' direct store' if direct else ''}"


@pytest.mark.parametrize("name", list(ec.SHAPE_CASES))
def test_conv3x3_on_every_kernel_path(dev, name):
    """the eight shapes of tests/test_gpu_igemm_epilogue_modes.py (the smallest that reach each kernel): both MFMA shapes, plain and
    tile-packed weights, the direct store on and off, the four layer kinds + a bias-less and a ReLU-less layer on the generic body"""
    c = ec.SHAPE_CASES[name]
    _, _, _, _, _, both, kind = ec.EPILOGUE_SHAPES[name]
    case = ec.conv_case(c)
    run = _ConvRun(dev, c, case, layout=kind if kind in ("concat", "tokens") else "plain")
    rec = _conv_record(c, case)
    path = _conv_path(c)
    for s16, direct in _mfma_and_store(c, both):
        for wt in [None] + (["direct" if direct else "packed"] if kind == "packed" else []):
            for flags in ec.LAYER_KINDS:
                # the direct-store kernel exists for the four layer kinds without the second output; a pack in ITS row order is refused by any other
                is_direct = direct and flags[0] and flags[3] and kind != "tokens"
                if direct and not is_direct:
                    continue
                run.launch(rec, flags, _label(path, s16, wt, is_direct), s16=s16, wt=wt, direct=direct)
    print(f"{name}: {rec['launches']} buffers, {rec['elements_compared']} elements, {rec['mismatches']} mismatches; paths {rec['paths']}")


OTHER_CONV = {**ec.NONSQUARE_CASES, **ec.REFUSED_CASES, **ec.SINGLE_TILE_CASES}


@pytest.mark.parametrize("name", list(OTHER_CONV))
def test_conv3x3_nonsquare_one_pixel_wide_and_single_tile(dev, name):
    """non-square images on the shifted-window kernel (and the transpose) and on the generic one, stride 2 at 6 x 10; the images one pixel
    wide that the shifted-window kernel refuses, for values on the kernel that takes them; launches of one tile down to M = 1"""
    c = OTHER_CONV[name]
    case = ec.conv_case(c)
    run = _ConvRun(dev, c, case)
    rec = _conv_record(c, case)
    path = _conv_path(c)
    assert path.startswith("k_conv_sw") == name.startswith("sw "), (name, path)
    for s16, direct in _mfma_and_store(c):
        for flags in ec.LAYER_KINDS:
            is_direct = direct and flags[0] and flags[3]
            if direct and not is_direct:
                continue
            run.launch(rec, flags, _label(path, s16, None, is_direct), s16=s16, direct=direct)
    print(f"{name}: {rec['launches']} buffers, {rec['elements_compared']} elements, {rec['mismatches']} mismatches; paths {rec['paths']}")


@pytest.mark.parametrize("name", ["sw 4x16x32 128->128", "generic 3x12x20 64->128", "stride2 2x6x10 64->128"])
def test_conv3x3_operands_as_column_blocks_of_wider_buffers(dev, name):
    """cstride > C, coff > 0 for input, output and residual: the neighbouring columns are canaries, read by nobody and left alone"""
    c = ec.NONSQUARE_CASES[name]
    case = ec.conv_case(c)
    run = _ConvRun(dev, c, case, layout="cols")
    rec = _conv_record(c, case, entry="fp_igemm_f16_fwd taps=9, column blocks")
    path = _conv_path(c)
    for s16, direct in _mfma_and_store(c):
        for flags in (ec.LAYER_KINDS[0], ec.LAYER_KINDS[3], ec.LAYER_KINDS[5]):
            is_direct = direct and flags[3]
            if direct and not is_direct:
                continue
            run.launch(rec, flags, _label(path, s16, None, is_direct), s16=s16, direct=direct)


@pytest.mark.parametrize("name", list(ec.SPLITK_CASES))
def test_splitk_conv_with_uneven_pieces(dev, name):
    """piece counts that do not divide the k-steps (ranges [s nk / n, (s + 1) nk / n) of unequal length), 1 and nk themselves; the
    workspace poisoned with both NaN patterns; the result is the reference and -- nothing depends on the order here -- the bits of
    the unsplit call"""
    c, res, bn, counts = ec.SPLITK_CASES[name]
    case = ec.conv_case(c)
    run = _ConvRun(dev, c, case)
    rec = _conv_record(c, case, entry="fp_igemm_f16_splitk_fwd taps=9")
    flags = (True, bn, res, True)
    unsplit = run.launch(_conv_record(c, case, entry="fp_igemm_f16_fwd taps=9, the unsplit call of"), flags, _conv_path(c))
    nk = 9 * c.Cin // 64
    for splits in counts:
        assert 1 <= splits <= nk
        for fill in (0x7f, 0xff):
            yf = run.launch(rec, flags, f"split-K 128x128, {splits} of {nk} k-steps", splits=splits, fill=fill)
            assert torch.equal(yf.view(torch.int16), unsplit.view(torch.int16)), f"{name} x{splits}: not the bits of the unsplit call"


@pytest.mark.parametrize("flags", ec.LAYER_KINDS, ids=lambda f: "bias%d-bn%d-res%d-relu%d" % f)
def test_splitk_token_layer_of_every_layer_kind(dev, flags):
    """k_splitk_epilogue with conv rounding: the 64-pixel token layer (output without border + the positional second output), split as
    the engine splits it for small calls, with each layer kind -- BatchNorm and residual on and off, a bias-less and a ReLU-less layer.
    Both outputs are the reference; the first is the bits of the unsplit call"""
    c, counts = ec.SPLITK_KINDS_CASE
    case = ec.conv_case(c)
    run = _ConvRun(dev, c, case, layout="tokens")
    kind = f"(bias, BatchNorm, residual, ReLU) = {flags}"
    rec = _conv_record(c, case, entry=f"fp_igemm_f16_splitk_fwd taps=9, {kind}")
    unsplit = run.launch(_conv_record(c, case, entry=f"fp_igemm_f16_fwd taps=9, {kind}, the unsplit call of"), flags, _conv_path(c))
    nk = 9 * c.Cin // 64
    for splits in counts:
        assert 1 <= splits <= nk
        for fill in (0x7f, 0xff):
            yf = run.launch(rec, flags, f"split-K 128x128, {splits} of {nk} k-steps", splits=splits, fill=fill)
            assert torch.equal(yf.view(torch.int16), unsplit.view(torch.int16)), f"{c.name} {flags} x{splits}: not the bits of the unsplit call"


# ------------------------------------------------------------------ (b), (c), (e): Linear
def _matrix(ld, coff=0):
    from foundationpose_amd import ops
    return ops.IgemmGeom(1, 1, 1, 1, 1, 0, int(ld), int(coff), 0, 0)


class _LinearRun:
    def __init__(self, dev, c, case):
        self.dev, self.c, self.case, self.op = dev, c, case, case["op"]
        op = self.op
        self.x = _t(op["ix"] * 2.0 ** -ec.X_EXP, dev)
        self.w = _t(op["iw"] * 2.0 ** -ec.W_EXP, dev)
        self.bias, self.pe = _t(op["bias"], dev, torch.float32), _t(op["pe"], dev, torch.float32)
        # the same operand as a column block of a wider matrix between canary columns
        self.xwf, self.xw = _guarded((c.M, c.K + 72), dev, fill=CANARY)
        self.xw[:, 40:40 + c.K] = self.x
        self.xw_before = self.xwf.clone()
        self.refs = {}

    def ref(self, bias, relu):
        if (bias, relu) not in self.refs:
            r = ec.linear_epilogue(self.case["A"], self.op, bias=bias, relu=relu)
            self.refs[bias, relu] = (_t(r, self.dev), _t(ec.pe_output(r, self.op["pe"]), self.dev))
        return self.refs[bias, relu]

    def launch(self, rec, path, bias, relu, wide, with_pe, splits=None, fill=0x7f):
        from foundationpose_amd import ops
        c = self.c
        ref, ref_pe = self.ref(bias, relu)
        ldy, coy = (c.N + 136, 64) if wide else (c.N, 0)
        yf, y = _guarded((c.M, ldy), self.dev, fill=CANARY)
        ef = yf.clone()
        ef[GUARD:GUARD + y.numel()].view(c.M, ldy)[:, coy:coy + c.N] = ref
        pf = y_pe = None
        if with_pe:
            pf, y_pe = _guarded((c.M, c.N), self.dev, fill=-7.0)
        x, gx = (self.xw, _matrix(c.K + 72, 40)) if wide else (self.x, _matrix(c.K))
        kw = dict(relu=relu, pe=self.pe if with_pe else None, y_pe=y_pe)
        b = self.bias if bias else None
        if splits is None:
            ops.igemm_f16(x, gx, self.w, b, y, _matrix(ldy, coy), c.M, c.N, c.K, 1, **kw)
        else:
            need = ops.igemm_splitk_workspace_bytes(c.M, c.N, splits)
            ws = torch.full((need + 64,), fill, dtype=torch.uint8, device=self.dev)
            ops.igemm_f16_splitk(x, gx, self.w, b, y, _matrix(ldy, coy), c.M, c.N, c.K, 1, splits, ws[:need], **kw)
            assert bool((ws[need:] == fill).all()), f"{c.name} x{splits}: wrote past the workspace"
        torch.cuda.synchronize()
        what = f"{c.name} bias={bias} relu={relu} wide={wide}"
        _compare(rec, what, path, yf, ef, (c.M, ldy))
        if pf is not None:
            epf = pf.clone()
            epf[GUARD:GUARD + y_pe.numel()] = ref_pe.flatten()
            _compare(rec, what + " second output", path, pf, epf, (c.M, c.N))
        _unchanged(self.xwf, self.xw_before, what + " input")
        return yf


def _linear_path(c):
    if c.N >= 1024:
        return "k_igemm_f16 256x128"
    if c.N % 256 == 0 and 4096 <= c.M < 75000:
        return "k_igemm_pp 256x256"
    return "k_igemm_f16 128x128"


# (bias, ReLU, leading dimensions larger than K and N, positional second output)
LINEAR_LAUNCHES = [(True, False, False, True), (True, True, True, False), (False, False, True, True), (False, True, False, False)]


@pytest.mark.parametrize("c", ec.LINEAR_CASES, ids=lambda c: c.name)
def test_linear_rounding_on_taps_1(dev, c):
    """nn.Linear: one rounding of accumulator + bias.  M around one and two 128-row tiles on the 128 x 128 kernel, 4097 rows on the
    256 x 256 ping-pong kernel (a ragged tile of one row), N = 1536 on the 256 x 128 kernel"""
    case = ec.linear_case(c)
    run = _LinearRun(dev, c, case)
    rec = _record("fp_igemm_f16_fwd taps=1", c.name, dict(M=c.M, K=c.K, N=c.N), case["sum_abs"])
    for bias, relu, wide, with_pe in LINEAR_LAUNCHES:
        run.launch(rec, _linear_path(c), bias, relu, wide, with_pe)


@pytest.mark.parametrize("name", list(ec.SPLITK_LINEAR_CASES))
def test_splitk_linear_with_positional_output(dev, name):
    c, counts = ec.SPLITK_LINEAR_CASES[name]
    case = ec.linear_case(c)
    run = _LinearRun(dev, c, case)
    rec = _record("fp_igemm_f16_splitk_fwd taps=1", c.name, dict(M=c.M, K=c.K, N=c.N), case["sum_abs"])
    unsplit = run.launch(_record("fp_igemm_f16_fwd taps=1, the unsplit call of", c.name, dict(M=c.M, K=c.K, N=c.N), case["sum_abs"]),
                         _linear_path(c), True, True, False, True)
    for splits in counts:
        for fill in (0x7f, 0xff):
            yf = run.launch(rec, f"split-K 128x128, {splits} of {c.K // 64} k-steps", True, True, False, True, splits=splits, fill=fill)
            assert torch.equal(yf.view(torch.int16), unsplit.view(torch.int16)), f"{name} x{splits}: not the bits of the unsplit call"
        run.launch(rec, f"split-K 128x128, {splits} of {c.K // 64} k-steps", False, False, True, True, splits=splits)


@pytest.mark.parametrize("c", ec.LINEAR512_CASES, ids=lambda c: c.name)
def test_linear512_against_the_reference(dev, c):
    """fp_linear512_f16_fwd against the float64 reference, not against another kernel"""
    from foundationpose_amd import ops
    case = ec.linear_case(c)
    op = case["op"]
    rec = _record("fp_linear512_f16_fwd", c.name, dict(M=c.M, K=c.K, N=c.N), case["sum_abs"])
    x = _t(op["ix"] * 2.0 ** -ec.X_EXP, dev)
    wp = ops.PackedLinear512(_t(op["iw"] * 2.0 ** -ec.W_EXP, dev))
    b = _t(op["bias"], dev, torch.float32)
    for bias, relu in itertools.product((True, False), (False, True)):
        yf, y = _guarded((c.M, c.N), dev, fill=CANARY)
        ef = yf.clone()
        ef[GUARD:GUARD + y.numel()] = _t(ec.linear_epilogue(case["A"], op, bias=bias, relu=relu), dev).flatten()
        ops.linear512(x, wp, b if bias else None, relu=relu, out=y)
        torch.cuda.synchronize()
        _compare(rec, f"{c.name} bias={bias} relu={relu}", "k_linear512", yf, ef, (c.M, c.N))


# ------------------------------------------------------------------ (d): the 7x7 stride-2 convolution
@pytest.mark.parametrize("c", ec.CONV7_CASES, ids=lambda c: c.name)
def test_conv7x7_bands_and_widths(dev, c):
    """one output row; below, on and above one 8-row band; bands crossing images; Wout no multiple of 8 or 32; the width limit.
    Every combination of BatchNorm and bias; pad 0, and pad 1 with a canary border the kernel must leave alone"""
    from foundationpose_amd import ops
    case = ec.conv7_case(c)
    op = case["op"]
    Ho, Wo = c.Hin // 2, c.Win // 2
    rec = _record("fp_conv7x7s2_bn_relu_fwd", c.name, dict(B=c.B, Hin=c.Hin, Win=c.Win, K=294), case["sum_abs"])
    xf, x = _guarded((c.B, 6, c.Hin, c.Win), dev)
    x[:] = _t(op["ix"] * 2.0 ** -ec.X_EXP, dev)
    x_before = xf.clone()
    w = _t((op["iw"] * 2.0 ** -ec.W_EXP).reshape(64, 294), dev)
    bias, scale, shift = (_t(op[k], dev, torch.float32) for k in ("bias", "scale", "shift"))
    for bn, has_bias in itertools.product((True, False), (True, False)):
        ref = _t(ec.conv_epilogue(case["A"], op, has_bias, bn, False, True), dev)
        for pad in (0, 1):
            shape = (c.B, Ho + 2 * pad, Wo + 2 * pad, 64)
            yf, y = _guarded(shape, dev, fill=CANARY)
            ef = yf.clone()
            ef[GUARD:GUARD + y.numel()].view(shape)[:, pad:pad + Ho, pad:pad + Wo, :] = ref
            ops.conv7x7s2_bn_relu(x, w, bias if has_bias else None, scale if bn else None, shift if bn else None, y, pad)
            torch.cuda.synchronize()
            _compare(rec, f"{c.name} BatchNorm={bn} bias={has_bias} pad={pad}", "k_conv7x7s2_nhwc", yf, ef, shape)
            _unchanged(xf, x_before, c.name + " input")


# ------------------------------------------------------------------ (f): fp_rows_linear_fwd
@pytest.mark.parametrize("c", ec.ROWS_LINEAR_CASES, ids=lambda c: c.name)
def test_rows_linear_all_modes(dev, c):
    """sum and bias add are exact: the fp32 output is the reference itself, the rounded modes one rounding of it; x as fp32 and as fp16"""
    from foundationpose_amd import ops
    case = ec.rows_linear_case(c)
    rec = _record("fp_rows_linear_fwd", c.name, dict(M=c.M, K=c.K, N=c.N), case["sum_abs"])
    w = _t(case["iw"] * 2.0 ** -ec.W_EXP, dev)
    b = _t(case["bias"], dev, torch.float32)
    out32, out16 = case["out32"], ec.f16(case["out32"])
    nob32 = case["A"] * ec.UNIT
    for xdt in (torch.float32, torch.float16):
        x = _t(case["ix"] * 2.0 ** -ec.X_EXP, dev, xdt)
        for mode, ydt, want, bias in (("f32", torch.float32, out32, b), ("f32 rounded", torch.float32, out16, b), ("f16", torch.float16, out16, b),
                                      ("f32 no bias", torch.float32, nob32, None)):
            yf, y = _guarded((c.M, c.N), dev, fill=CANARY, dtype=ydt)
            ef = yf.clone()
            ef[GUARD:GUARD + y.numel()] = _t(want, dev, ydt).flatten()
            ops.rows_linear(x, w, bias, round_f16=mode == "f32 rounded", out_f16=mode == "f16", out=y)
            torch.cuda.synchronize()
            _compare(rec, f"{c.name} x {xdt} out {mode}", "k_rows_linear", yf, ef, (c.M, c.N))


# ------------------------------------------------------------------ (g): fp_colmean_f16_fwd without LayerNorm
@pytest.mark.parametrize("groups,rows", ec.COLMEAN_CASES)
def test_colmean_plain(dev, groups, rows):
    """the column sums are exact.  A power-of-two row count: the output is the mean itself.  Otherwise the kernel multiplies the sum by
    fl(1 / rows): two roundings of relative 2^-24 each, so |out - s / rows| <= 2^-23 |s / rows| (1 + 2^-24) -- derived, not measured"""
    from foundationpose_amd import ops
    case = ec.colmean_case(groups, rows)
    rec = _record("fp_colmean_f16_fwd", f"{groups} groups of {rows} rows", dict(groups=groups, rows=rows, D=512), case["sum_abs"])
    out = ops.colmean_f16(_t(case["x"], dev))
    torch.cuda.synchronize()
    got, mean = out.double().cpu().numpy(), case["mean"]
    assert got.shape == mean.shape and np.isfinite(got).all()
    if rows & (rows - 1) == 0:
        bad = got != mean
    else:
        bad = np.abs(got - mean) > 2.0 ** -23 * np.abs(mean) * (1 + 2.0 ** -24)
    rec.update(launches=1, elements_compared=int(got.size), mismatches=int(bad.sum()), paths=["k_colmean512"])
    assert not bad.any(), f"colmean {groups} x {rows}: {int(bad.sum())} of {got.size} outputs off, first at {tuple(int(v) for v in np.argwhere(bad)[0])}"
