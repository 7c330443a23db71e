"""Exactly summable operands for the convolution and Linear kernels, and the float64 reference of their rounding policy (numpy only).

Every operand is an integer times a power of two: x = ix * 2^-4, w = iw * 2^-7, so every product is an integer number of UNIT = 2^-11.
As long as the sum over k of |x||w| stays below 2^24 units at every output element, every partial sum -- in any order, inside an MFMA,
across split-K pieces -- is an integer below 2^24 units and therefore exactly representable in fp32: the accumulator is a known number,
whatever the kernel's summation order, and every rounding point of the policy is ONE well-defined round-to-nearest-even.  A kernel then
has to return the reference at every element; there is nothing left for a tolerance to absorb.

The ranges of ix and iw are chosen per reduction length (`ranges_for`): wide enough that the accumulators outgrow the 11 significant
bits of fp16 (at least 10 % of them need rounding: asserted), narrow enough for the 2^24 rule (asserted), and no wider -- accumulators of
a few thousand units are where exact fp16 ties are common, and ties are what tells round-to-nearest-even from its neighbours.

The epilogue operands are exact too: bias and BatchNorm shift k * 2^-11 (|k| <= 2047), BatchNorm scale from a few short binary
fractions, residual k * 2^-10, positional table k * 2^-12.  With them the float32 evaluation of every elementwise statement equals the
float64 one (asserted on every use), so the reference does not depend on whether the kernel fuses `y * scale + shift` into an fmaf.

The case lists at the end are what tests/test_gpu_exact_sums.py launches and tests/test_exact_cases_host.py checks on the CPU."""
import functools
from dataclasses import dataclass

import numpy as np

LIMIT = 1 << 24
X_EXP, W_EXP = 4, 7
UNIT = 2.0 ** -(X_EXP + W_EXP)
BN_SCALES = np.array([0.5, 0.75, 1.0, 1.25, 1.5, 2.0, -1.0, -0.75])
F16_MAX = 65504.0
NEED_ROUNDING = 0.10                # share of the accumulators with more than 11 significant bits, at least
# (largest |ix|, largest |iw|), narrowest first
RANGES = ((15, 15), (31, 15), (31, 31), (63, 31), (63, 63), (127, 63), (255, 63))


# ------------------------------------------------------------------ roundings
def f16(v):
    """round to nearest even to fp16 (numpy converts float64 -> float16 in one rounding), as float64"""
    return np.asarray(v, dtype=np.float64).astype(np.float16).astype(np.float64)


def _toward_zero16(v):
    v = np.asarray(v, dtype=np.float64)
    r = v.astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(v)
    return np.where(over, np.nextafter(r, np.float16(0)), r)


def f16_toward_zero(v):
    return _toward_zero16(v).astype(np.float64)


def f16_half_away(v):
    """round to nearest, ties away from zero"""
    v = np.asarray(v, dtype=np.float64)
    lo = _toward_zero16(v)
    hi = np.nextafter(lo, np.where(v < 0, -np.inf, np.inf).astype(np.float16))
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    tie = (v != lo64) & (v - lo64 == hi64 - v)              # both differences are exact in float64
    return np.where(tie, hi64, f16(v))


def _same_in_f32(a, b, op, what):
    """the float32 evaluation of one elementwise statement equals the float64 one (`op`: '+' or '*+' with b = (scale, shift))"""
    a32 = np.asarray(a, dtype=np.float32)
    if op == "+":
        r32, r64 = a32 + np.asarray(b, dtype=np.float32), np.asarray(a, dtype=np.float64) + b
    else:
        sc, sh = b
        p32 = a32 * np.asarray(sc, dtype=np.float32)          # multiply, then add: two float32 roundings, both of which have to be exact
        assert np.array_equal(p32.astype(np.float64), np.asarray(a, dtype=np.float64) * sc), what
        r32, r64 = p32 + np.asarray(sh, dtype=np.float32), np.asarray(a, dtype=np.float64) * sc + sh
    assert np.array_equal(r32.astype(np.float64), r64), f"{what}: float32 and float64 disagree"


# ------------------------------------------------------------------ operands
def ranges_for(k_eff):
    """the narrowest (|ix|, |iw|) ranges whose accumulators are expected to exceed 2048 units (x: 40 % zeros): sqrt(k Ex^2 Ew^2) >= 2048"""
    for xmax, wmax in RANGES:
        ex2 = 0.6 * (xmax + 1) * (2 * xmax + 1) / 6.0
        ew2 = wmax * (wmax + 1) / 3.0
        if k_eff * ex2 * ew2 >= 2048.0 ** 2:
            return xmax, wmax
    return RANGES[-1]


def _ints(rng, shape, lo, hi, zeros=0.0):
    v = rng.integers(lo, hi + 1, size=shape).astype(np.float64)
    if zeros:
        v[rng.random(shape) < zeros] = 0.0
    return v


def _epilogue_operands(rng, N, res_shape, pe_period):
    return dict(bias=_ints(rng, N, -2047, 2047) * 2.0 ** -11, scale=BN_SCALES[rng.integers(0, len(BN_SCALES), size=N)],
                shift=_ints(rng, N, -2047, 2047) * 2.0 ** -11, res=_ints(rng, res_shape, -2047, 2047) * 2.0 ** -10,
                pe=_ints(rng, (pe_period, N), -4095, 4095) * 2.0 ** -12 if pe_period else None)


def _check_operands(*arrays):
    for a in arrays:
        if a is None:
            continue
        a = np.asarray(a, dtype=np.float64)
        assert np.isfinite(a).all()
        nz = np.abs(a[a != 0])
        assert nz.size == 0 or nz.min() >= 2.0 ** -14, "a subnormal operand"       # fp16's smallest normal number


def _check_sums(A, S, what, extra=0.0):
    """the generator's two conditions.  A: accumulators, S: sums of |products| (+ `extra`: |bias| where it joins the fp32 sum), in units"""
    smax = float(S.max() + extra)
    assert smax < LIMIT, f"{what}: sum of |products| reaches {smax} units"
    val = A * UNIT
    frac = float(np.mean(f16(val) != val))
    assert frac >= NEED_ROUNDING, f"{what}: only {frac:.3f} of the accumulators need rounding"
    return smax, frac


# ------------------------------------------------------------------ 3x3 convolution (fp_igemm_f16_fwd, taps = 9, and its split-K form)
@dataclass(frozen=True)
class Conv:
    name: str
    B: int
    Ho: int
    Wo: int
    Cin: int
    Cout: int
    stride: int = 1
    seed: int = 0
    pe_period: int = 0               # > 0: a positional table of that many rows (the token layer)
    xw: tuple = None                 # (|ix|, |iw|) instead of ranges_for

    @property
    def M(self):
        return self.B * self.Ho * self.Wo

    @property
    def hw_in(self):
        return self.Ho * self.stride, self.Wo * self.stride

    @property
    def k_eff(self):                 # products that are not padding at a typical output pixel
        Hin, Win = self.hw_in
        return self.Cin * min(3, Hin) * min(3, Win)


@functools.lru_cache(maxsize=6)
def conv_operands(c):
    """ix (B, Hin, Win, Cin) NHWC and iw (Cout, ky, kx, Cin) -- the kernel's k order -- as integers (float64), the epilogue operands as values"""
    rng = np.random.default_rng([c.seed, c.B, c.Ho, c.Wo, c.Cin, c.Cout, c.stride])
    xmax, wmax = c.xw or ranges_for(c.k_eff)
    Hin, Win = c.hw_in
    op = dict(ix=_ints(rng, (c.B, Hin, Win, c.Cin), 0, xmax, zeros=0.4), iw=_ints(rng, (c.Cout, 3, 3, c.Cin), -wmax, wmax), xmax=xmax, wmax=wmax)
    op.update(_epilogue_operands(rng, c.Cout, (c.B, c.Ho, c.Wo, c.Cout), c.pe_period))
    _check_operands(op["ix"] * 2.0 ** -X_EXP, op["iw"] * 2.0 ** -W_EXP, op["bias"], op["scale"], op["shift"], op["res"], op["pe"])
    return op


def conv_acc(c, ix, iw, keep=None, swap_kyx=False):
    """acc[b, oy, ox, n] = sum_{ky, kx, ci} x[b, oy*stride + ky - 1, ox*stride + kx - 1, ci] * w[n, ky, kx, ci] in units, zero padding;
    keep: (9, Cin) bool, the k = tap * Cin + ci that take part (None: all); swap_kyx: the weight's taps read as (kx, ky)"""
    xp = np.pad(ix, ((0, 0), (1, 1), (1, 1), (0, 0)))
    s = c.stride
    A = np.zeros((c.M, c.Cout))
    for ky in range(3):
        for kx in range(3):
            sel = slice(None) if keep is None else keep[ky * 3 + kx]
            if keep is not None and not sel.any():
                continue
            patch = xp[:, ky:ky + s * c.Ho:s, kx:kx + s * c.Wo:s, :].reshape(c.M, c.Cin)
            wk = iw[:, kx, ky] if swap_kyx else iw[:, ky, kx]
            A += patch[:, sel] @ wk[:, sel].T
    return A.reshape(c.B, c.Ho, c.Wo, c.Cout)


@functools.lru_cache(maxsize=6)
def conv_case(c):
    """-> dict(op, A: accumulators in units, sum_abs: largest sum of |products| in units, need_rounding).  Asserts the two conditions."""
    op = conv_operands(c)
    A = conv_acc(c, op["ix"], op["iw"])
    S = conv_acc(c, op["ix"], np.abs(op["iw"]))
    smax, frac = _check_sums(A, S, c.name)
    return dict(op=op, A=A, sum_abs=smax, need_rounding=frac)


def conv_epilogue(A, op, bias=True, bn=True, res=True, relu=True, rnd=f16, variant=None):
    """the policy on accumulators A (units): f16(f16(f16(f16(acc) + bias) * scale + shift) + residual), then ReLU.  rnd: the rounding at
    every point.  variant: a WRONG neighbour -- 'single_bias' (one rounding of acc + bias), 'bn_unrounded' (BatchNorm without its own
    rounding), 'res_before_bn', 'relu_before_res'.  The float32-equals-float64 checks run on the policy itself (variant None)."""
    check = variant is None and rnd is f16
    acc = A * UNIT
    if bias and variant == "single_bias":
        y = rnd(acc + op["bias"])
    else:
        y = rnd(acc)
        if bias:
            if check:
                _same_in_f32(y, op["bias"], "+", "conv + bias")
            y = rnd(y + op["bias"])
    r = op["res"] if res else None
    if res and variant == "res_before_bn":
        y, r = rnd(y + r), None
    if bn:
        if check:
            _same_in_f32(y, (op["scale"], op["shift"]), "*+", "BatchNorm")
        y = y * op["scale"] + op["shift"]
        if not (variant == "bn_unrounded" and r is not None):
            y = rnd(y)
    if variant == "relu_before_res" and relu:
        y = np.maximum(y, 0.0)
    if r is not None:
        if check:
            _same_in_f32(y, r, "+", "+ residual")
        y = rnd(y + r)
    if relu and variant != "relu_before_res":
        y = np.maximum(y, 0.0)
    assert np.isfinite(y).all() and np.abs(y).max() < F16_MAX
    return y


def pe_output(y, pe):
    """second output: y_pe[m] = f16(y[m] + pe[m % period]) for y (M, N)"""
    t = pe[np.arange(y.shape[0]) % pe.shape[0]]
    _same_in_f32(y, t, "+", "+ positional table")
    return f16(y + t)


def splitk_ranges(nk, splits):
    """k-step ranges of fp_igemm_f16_splitk_fwd: piece s takes [s * nk / splits, (s + 1) * nk / splits)"""
    return [(s * nk // splits, (s + 1) * nk // splits) for s in range(splits)]


def conv_keep_steps(c, steps):
    """(9, Cin) mask of the k-steps (64 k each, k = tap * Cin + ci) in `steps`"""
    keep = np.zeros(9 * c.Cin, dtype=bool)
    for t in steps:
        keep[64 * t:64 * t + 64] = True
    return keep.reshape(9, c.Cin)


# ------------------------------------------------------------------ Linear (fp_igemm_f16_fwd taps = 1, its split-K form, fp_linear512_f16_fwd)
@dataclass(frozen=True)
class Linear:
    M: int
    K: int
    N: int
    seed: int = 0
    pe_period: int = 100

    @property
    def name(self):
        return f"linear {self.M}x{self.K}x{self.N}"


@functools.lru_cache(maxsize=6)
def linear_case(c):
    """x (M, K) signed with 20 % zeros, w (N, K), bias, pe as values; A = x @ w^T in units.  The bias joins the fp32 sum (nn.Linear: one
    rounding of accumulator + bias), so it counts towards the 2^24 units, and `need_rounding` is taken on accumulator + bias."""
    rng = np.random.default_rng([c.seed, c.M, c.K, c.N])
    xmax, wmax = ranges_for(c.K * 0.8 / 0.6)         # 20 % zeros where ranges_for reckons with 40 %
    ix, iw = _ints(rng, (c.M, c.K), -xmax, xmax, zeros=0.2), _ints(rng, (c.N, c.K), -wmax, wmax)
    op = dict(ix=ix, iw=iw, xmax=xmax, wmax=wmax)
    op.update(_epilogue_operands(rng, c.N, (1,), c.pe_period))
    _check_operands(ix * 2.0 ** -X_EXP, iw * 2.0 ** -W_EXP, op["bias"], op["pe"])
    A = ix @ iw.T
    S = np.abs(ix) @ np.abs(iw).T
    smax, frac = _check_sums(A + op["bias"] / UNIT, S, c.name, extra=2047)
    return dict(op=op, A=A, sum_abs=smax, need_rounding=frac)


def linear_epilogue(A, op, bias=True, relu=False, rnd=f16, variant=None):
    """f16(acc + bias), then ReLU.  variant 'double': f16(f16(acc) + bias)"""
    acc = A * UNIT
    if bias:
        if variant is None and rnd is f16:
            _same_in_f32(acc, op["bias"], "+", "Linear acc + bias")
        y = rnd(rnd(acc) + op["bias"]) if variant == "double" else rnd(acc + op["bias"])
    else:
        y = rnd(acc)
    if relu:
        y = np.maximum(y, 0.0)
    assert np.isfinite(y).all() and np.abs(y).max() < F16_MAX
    return y


def linear_keep_steps(c, steps):
    keep = np.zeros(c.K, dtype=bool)
    for t in steps:
        keep[64 * t:64 * t + 64] = True
    return keep


# ------------------------------------------------------------------ 7x7 stride-2 convolution (fp_conv7x7s2_bn_relu_fwd), K = 6 * 49 = 294
@dataclass(frozen=True)
class Conv7:
    B: int
    Hin: int
    Win: int
    seed: int = 0

    @property
    def name(self):
        return f"conv7x7 {self.B}x{self.Hin}x{self.Win}"


def conv7_acc(c, ix, iw, pad=3):
    """acc[b, oy, ox, n] = sum_{ci, ky, kx} x[b, ci, 2 oy + ky - pad, 2 ox + kx - pad] * w[n, ci, ky, kx] in units (NCHW in, NHWC out)"""
    Ho, Wo = c.Hin // 2, c.Win // 2
    xp = np.pad(ix, ((0, 0), (0, 0), (pad, 7), (pad, 7)))
    A = np.zeros((c.B * Ho * Wo, 64))
    for ky in range(7):
        for kx in range(7):
            patch = xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2].transpose(0, 2, 3, 1).reshape(-1, 6)
            A += patch @ iw[:, :, ky, kx].T
    return A.reshape(c.B, Ho, Wo, 64)


@functools.lru_cache(maxsize=None)
def conv7_case(c):
    rng = np.random.default_rng([c.seed, c.B, c.Hin, c.Win, 7])
    xmax, wmax = ranges_for(6 * min(7, c.Hin) * min(7, c.Win))     # the taps of a small image that are not padding
    ix, iw = _ints(rng, (c.B, 6, c.Hin, c.Win), 0, xmax, zeros=0.4), _ints(rng, (64, 6, 7, 7), -wmax, wmax)
    op = dict(ix=ix, iw=iw, xmax=xmax, wmax=wmax)
    op.update(_epilogue_operands(rng, 64, (1,), 0))
    _check_operands(ix * 2.0 ** -X_EXP, iw * 2.0 ** -W_EXP, op["bias"], op["scale"], op["shift"])
    A = conv7_acc(c, ix, iw)
    smax, frac = _check_sums(A, conv7_acc(c, ix, np.abs(iw)), c.name)
    return dict(op=op, A=A, sum_abs=smax, need_rounding=frac)


# ------------------------------------------------------------------ fp_rows_linear_fwd
@dataclass(frozen=True)
class RowsLinear:
    M: int
    K: int
    N: int
    seed: int = 0

    @property
    def name(self):
        return f"rows_linear {self.M}x{self.K}x{self.N}"


@functools.lru_cache(maxsize=None)
def rows_linear_case(c):
    """x: integers up to +-255 times 2^-4 (exact in fp32 AND in fp16, so one case serves both input types); the widest w that keeps
    K * 255 * |iw| + |bias| below 2^24 units.  -> out32 = x @ w^T + bias, exact; the rounded output modes are f16(out32)."""
    rng = np.random.default_rng([c.seed, c.M, c.K, c.N, 11])
    xmax = 255
    wmax = max(w for w in (15, 31, 63) if c.K * xmax * w + 2047 < LIMIT)
    ix, iw = _ints(rng, (c.M, c.K), -xmax, xmax, zeros=0.2), _ints(rng, (c.N, c.K), -wmax, wmax)
    bias = _ints(rng, c.N, -2047, 2047) * 2.0 ** -11
    _check_operands(ix * 2.0 ** -X_EXP, iw * 2.0 ** -W_EXP, bias)
    A = ix @ iw.T
    smax, frac = _check_sums(A + bias / UNIT, np.abs(ix) @ np.abs(iw).T, c.name, extra=2047)
    _same_in_f32(A * UNIT, bias, "+", "rows_linear acc + bias")
    out32 = A * UNIT + bias
    assert np.array_equal(out32.astype(np.float32).astype(np.float64), out32)
    return dict(ix=ix, iw=iw, bias=bias, A=A, out32=out32, sum_abs=smax, need_rounding=frac, xmax=xmax, wmax=wmax)


# ------------------------------------------------------------------ fp_colmean_f16_fwd without LayerNorm
@functools.lru_cache(maxsize=None)
def colmean_case(groups, rows):
    """x (groups, rows, 512) = k * 2^-4, |k| <= 1023: the column sums are integers below 2^20 units of 2^-4, exact in any order.
    -> x, sums (values), mean = sums / rows in float64"""
    rng = np.random.default_rng([groups, rows, 13])
    ix = _ints(rng, (groups, rows, 512), -1023, 1023)
    assert np.abs(ix).sum(axis=1).max() < LIMIT
    x = ix * 2.0 ** -4
    _check_operands(x)
    s = x.sum(axis=1)
    return dict(x=x, sums=s, mean=s / rows, sum_abs=float(np.abs(ix).sum(axis=1).max()))


# ------------------------------------------------------------------ the cases of tests/test_gpu_exact_sums.py
# (bias, BatchNorm, residual, ReLU): the four layer kinds the library compiles an epilogue body for, then a bias-less and a ReLU-less
# layer, which run the generic body
LAYER_KINDS = [(True, True, True, True), (True, True, False, True), (True, False, True, True), (True, False, False, True),
               (False, True, True, True), (True, True, True, False)]
# (a) the eight shapes of tests/test_gpu_igemm_epilogue_modes.py SHAPES, field for field (test_exact_cases_host.py holds the two equal)
EPILOGUE_SHAPES = {
    "sw128": (3, 40, 128, 128, 1, True, "plain"),
    "sw512": (5, 20, 512, 512, 1, True, "plain"),
    "sw256": (2, 40, 256, 256, 1, True, "packed"),
    "sw256x256": (2, 20, 256, 256, 1, True, "plain"),
    "s2_64": (2, 40, 64, 128, 2, False, "plain"),
    "s2_256": (2, 20, 256, 512, 2, False, "plain"),
    "concat": (4, 40, 128, 128, 1, True, "concat"),
    "tokens": (3, 20, 512, 512, 1, True, "tokens"),
}
SHAPE_CASES = {n: Conv(n, B, H, H, Cin, Cout, stride, seed=i, pe_period=H * H if kind == "tokens" else 0)
               for i, (n, (B, H, Cin, Cout, stride, _, kind)) in enumerate(EPILOGUE_SHAPES.items())}
# non-square images: the shifted-window kernel (two whole 512-row tiles) and its transpose, the generic kernel, stride 2
NONSQUARE_CASES = {c.name: c for c in (
    Conv("sw 4x16x32 128->128", 4, 16, 32, 128, 128, seed=20), Conv("sw 4x32x16 128->128", 4, 32, 16, 128, 128, seed=21),
    Conv("generic 3x12x20 64->128", 3, 12, 20, 64, 128, seed=22), Conv("generic 3x5x9 128->128", 3, 5, 9, 128, 128, seed=23),
    Conv("stride2 2x6x10 64->128", 2, 6, 10, 64, 128, stride=2, seed=24))}
# images one pixel wide, which the shifted-window kernel refuses (tests/test_conv_sw_applicable_host.py REFUSED), on the generic kernel
REFUSED = [(2048, 1, 1, 128), (64, 40, 1, 128), (4096, 2, 1, 256)]
REFUSED_CASES = {f"refused {B}x{H}x{W} {C}->{C}": Conv(f"refused {B}x{H}x{W} {C}->{C}", B, H, W, C, C, seed=30 + i)
                 for i, (B, H, W, C) in enumerate(REFUSED)}
# launches of a single tile
SINGLE_TILE_CASES = {c.name: c for c in (Conv("single 1x1x1 64->128", 1, 1, 1, 64, 128, seed=40), Conv("single 1x2x2 64->128", 1, 2, 2, 64, 128, seed=41),
                                         Conv("single 1x8x8 64->128", 1, 8, 8, 64, 128, seed=42))}
CONV_CASES = {**SHAPE_CASES, **NONSQUARE_CASES, **REFUSED_CASES, **SINGLE_TILE_CASES}

# (c) split-K: the shapes of test_gpu_amp.py test_igemm_splitk_policy with one image: name -> (case, residual, BatchNorm, piece counts);
# nk = 9 Cin / 64 k-steps; counts that do not divide nk (uneven pieces), 1 and nk itself
SPLITK_CASES = {
    "splitk 40x40 128->128": (Conv("splitk 40x40 128->128", 1, 40, 40, 128, 128, seed=50), True, True, (5, 17, 1, 18)),
    "splitk 40x40 256->256": (Conv("splitk 40x40 256->256", 1, 40, 40, 256, 256, seed=51), True, True, (35, 1, 36)),
    "splitk 20x20 512->512": (Conv("splitk 20x20 512->512", 1, 20, 20, 512, 512, seed=52), True, True, (71, 1, 72)),
    "splitk 20x20 512->512 plain": (Conv("splitk 20x20 512->512 plain", 1, 20, 20, 512, 512, seed=53), False, False, (71, 1, 72)),
    "splitk s2 40x40 64->128": (Conv("splitk s2 40x40 64->128", 1, 40, 40, 64, 128, stride=2, seed=54), False, True, (2, 7, 1, 9)),
    "splitk s2 20x20 256->512": (Conv("splitk s2 20x20 256->512", 1, 20, 20, 256, 512, stride=2, seed=55), False, True, (35, 1, 36)),
    "splitk 8x8 128->128": (Conv("splitk 8x8 128->128", 1, 8, 8, 128, 128, seed=56), True, True, (5, 17, 1, 18)),
}
# ... and the smallest of them (its seed: the same operands) as the token layer -- output without border + the positional second output --
# which the engine runs split for small calls: launched with every one of LAYER_KINDS, so k_splitk_epilogue's arithmetic is pinned for
# conv rounding with and without BatchNorm, residual, bias and ReLU, each with the positional add behind it.  (case, piece counts)
SPLITK_KINDS_CASE = (Conv("splitk 8x8 128->128 tokens", 1, 8, 8, 128, 128, seed=56, pe_period=64), (5, 17, 1, 18))
SPLITK_LINEAR_CASES = {"splitk linear 400x512x512": (Linear(400, 512, 512, seed=57), (3, 7, 1, 8)),
                       "splitk linear 37x64x128": (Linear(37, 64, 128, seed=58), (1,))}

# (b) taps = 1: the 128 x 128 kernel, the 256 x 256 ping-pong kernel with a ragged tile, the 256 x 128 kernel (N >= 1024)
LINEAR_CASES = [Linear(M, K, N) for M in (1, 127, 128, 129, 255, 257) for K in (64, 512) for N in (128, 512)] + \
               [Linear(4097, 512, 512), Linear(1, 512, 1536), Linear(257, 512, 1536)]
# (e) fp_linear512_f16_fwd
LINEAR512_CASES = [Linear(M, 512, N, seed=5) for M in (1, 127, 128, 129, 400) for N in (512, 1536, 3072)]

# (d) (B, Hin, Win): one output row; below, on and above one 8-row band; bands crossing images; Wout no multiple of 8 or 32; the width limit
CONV7_CASES = [Conv7(*s) for s in ((1, 2, 8), (1, 14, 8), (1, 16, 8), (1, 18, 8), (3, 34, 24), (2, 16, 40), (1, 6, 72), (1, 4, 256), (5, 30, 56))]

# (f) a covering subset of M {1, 3, 4, 5, 252} x K {8, 64, 512, 520, 1024, 2048} x N {1, 3, 31, 32, 33, 130}: every value of each
# at least twice; K = 520, 1024, 2048 run the second to fourth k0 iteration, 520 with lanes past K in it.  (1, 8, 1) has ONE
# accumulator, which has to be one that needs rounding: the fourth field is the seed at which the generator's condition holds
ROWS_LINEAR_CASES = [RowsLinear(*s) for s in ((1, 8, 1, 1), (3, 64, 3), (4, 512, 31), (5, 520, 32), (252, 1024, 33), (1, 2048, 130), (3, 2048, 1), (4, 1024, 3),
                                              (5, 8, 31), (252, 64, 32), (252, 520, 33), (5, 512, 130), (4, 2048, 33), (3, 520, 130), (1, 1024, 32))]

# (g) rows per group x groups
COLMEAN_CASES = [(g, r) for r in (1, 15, 16, 17, 63, 64, 65, 400, 1024) for g in (1, 3)]
