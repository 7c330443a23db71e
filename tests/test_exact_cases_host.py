"""CPU: the exactly summable cases of tests/exact_cases.py -- what tests/test_gpu_exact_sums.py holds the convolution and Linear kernels to
with no tolerance -- are what they claim to be, and a subtly wrong kernel could not meet them.

 1. On every conv and Linear case the float64 reference with explicit roundings equals amp_util.conv_amp_ref (pinned to the reference's
    modules under autocast by tests/test_oracle_amp_golden.py) bit for bit; for taps = 1, the r16((x @ w.T + b).float()) form of
    tests/test_gpu_amp.py test_igemm_channel_concat_and_linear_policy.  On exact operands the two cannot differ.
 2. The generator's two conditions (sum of |products| below 2^24 units; at least 10 % of the accumulators need rounding) hold for every
    case of the GPU file.  exact_cases asserts them on every use; here every case is used.
 3. Wrong variants -- another rounding, a rounding point moved or dropped, a tap dropped, taps or image sides swapped, a padding or a
    split-K range off by one -- each change at least 1 % of the elements of every case they are named on, so the GPU file's "0
    mismatches" rejects them whatever the case.  The 1 % is a condition on the cases (exact_cases.ranges_for), not a measurement."""
import dataclasses

import numpy as np
import pytest
import torch

import exact_cases as ec
from amp_util import conv_amp_ref, r16

MIN_CHANGED = 0.01
# (bias, BatchNorm, residual, ReLU) as the GPU file launches them: the four layer kinds, then a bias-less and a ReLU-less one
KINDS = ec.LAYER_KINDS
ALL_CONV = {**ec.CONV_CASES, **{n: v[0] for n, v in ec.SPLITK_CASES.items()}, ec.SPLITK_KINDS_CASE[0].name: ec.SPLITK_KINDS_CASE[0]}
ALL_LINEAR = {c.name + f" seed {c.seed}": c for c in ec.LINEAR_CASES + ec.LINEAR512_CASES + [v[0] for v in ec.SPLITK_LINEAR_CASES.values()]}


def _changed(a, b):
    return float(np.mean(a != b))


def test_the_epilogue_shapes_are_those_of_the_epilogue_modes_file():
    import test_gpu_igemm_epilogue_modes as modes
    assert ec.EPILOGUE_SHAPES == modes.SHAPES
    import test_conv_sw_applicable_host as app
    assert ec.REFUSED == app.REFUSED


# ------------------------------------------------------------------ 1. the reference is the pinned one
@pytest.mark.parametrize("name", list(ALL_CONV))
def test_conv_reference_equals_conv_amp_ref(name):
    c = ALL_CONV[name]
    case = ec.conv_case(c)
    op = case["op"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    x = t((op["ix"] * 2.0 ** -ec.X_EXP).transpose(0, 3, 1, 2))
    w = t((op["iw"] * 2.0 ** -ec.W_EXP).transpose(0, 3, 1, 2))
    assert torch.equal(r16(x), x) and torch.equal(r16(w), w)                      # fp16 values
    res = t(op["res"].transpose(0, 3, 1, 2))
    kinds = KINDS if c.M * 9 * c.Cin * c.Cout < 1e9 else KINDS[:1]                  # conv_amp_ref convolves anew on every call
    for bias, bn, rs, relu in kinds:
        want, _, _ = conv_amp_ref(x, w, t(op["bias"]) if bias else None, (t(op["scale"]), t(op["shift"])) if bn else None, c.stride,
                                  residual=res if rs else None, relu=relu)
        got = ec.conv_epilogue(case["A"], op, bias, bn, rs, relu)
        assert np.array_equal(got.transpose(0, 3, 1, 2), want.double().numpy()), (name, bias, bn, rs, relu)


@pytest.mark.parametrize("name", list(ALL_LINEAR))
def test_linear_reference_equals_the_rounded_matmul(name):
    c = ALL_LINEAR[name]
    case = ec.linear_case(c)
    op = case["op"]
    x = torch.from_numpy(op["ix"] * 2.0 ** -ec.X_EXP).float()
    w = torch.from_numpy(op["iw"] * 2.0 ** -ec.W_EXP).float()
    b = torch.from_numpy(op["bias"]).float()
    assert torch.equal(r16(x), x) and torch.equal(r16(w), w)
    want = r16((x.double() @ w.double().t() + b.double()).float())
    assert np.array_equal(ec.linear_epilogue(case["A"], op), want.double().numpy())
    assert np.array_equal(ec.linear_epilogue(case["A"], op, relu=True), torch.relu(want).double().numpy())
    want0 = r16((x.double() @ w.double().t()).float())
    assert np.array_equal(ec.linear_epilogue(case["A"], op, bias=False), want0.double().numpy())


# ------------------------------------------------------------------ 2. the generator's conditions, on every case of the GPU file
def test_every_case_meets_the_generators_conditions():
    rep = {}
    for name, c in ALL_CONV.items():
        rep[name] = ec.conv_case(c)
    for name, c in ALL_LINEAR.items():
        rep[name] = ec.linear_case(c)
    for c in ec.CONV7_CASES:
        rep[c.name] = ec.conv7_case(c)
    for c in ec.ROWS_LINEAR_CASES:
        rep[c.name] = ec.rows_linear_case(c)
    for name, r in rep.items():
        assert r["sum_abs"] < ec.LIMIT and r["need_rounding"] >= ec.NEED_ROUNDING, (name, r["sum_abs"], r["need_rounding"])
    for g, rows in ec.COLMEAN_CASES:
        assert ec.colmean_case(g, rows)["sum_abs"] < ec.LIMIT
    worst = max(rep, key=lambda n: rep[n]["sum_abs"])
    least = min(rep, key=lambda n: rep[n]["need_rounding"])
    print(f"largest sum of |products|: {rep[worst]['sum_abs']:.0f} units ({worst}); least rounding: {rep[least]['need_rounding']:.3f} ({least})")


def test_the_rounding_helpers():
    v = np.array([2049.0, 2051.0, -2049.0, -2051.0, 2050.0, 0.5 + 2.0 ** -12, 1.0 + 2.0 ** -11 + 2.0 ** -20])   # ties at 2048 .. 4096: odd integers
    assert ec.f16(v).tolist() == [2048.0, 2052.0, -2048.0, -2052.0, 2050.0, 0.5, 1.0 + 2.0 ** -10]
    assert ec.f16_half_away(v).tolist() == [2050.0, 2052.0, -2050.0, -2052.0, 2050.0, 0.5 + 2.0 ** -11, 1.0 + 2.0 ** -10]
    assert ec.f16_toward_zero(v).tolist() == [2048.0, 2050.0, -2048.0, -2050.0, 2050.0, 0.5, 1.0]


# ------------------------------------------------------------------ 3. wrong variants
def _conv_variants(c, case):
    """name -> wrong output, for the layer with everything in it (bias, BatchNorm, residual, ReLU) unless the variant says otherwise"""
    op, A = case["op"], case["A"]
    Hin, Win = c.hw_in
    out = {
        "single rounding of acc + bias": ec.conv_epilogue(A, op, variant="single_bias"),
        "round toward zero": ec.conv_epilogue(A, op, rnd=ec.f16_toward_zero),
        "round half away from zero": ec.conv_epilogue(A, op, rnd=ec.f16_half_away),
        "BatchNorm without its rounding": ec.conv_epilogue(A, op, variant="bn_unrounded"),
        "residual in front of BatchNorm": ec.conv_epilogue(A, op, variant="res_before_bn"),
        "ReLU in front of the residual": ec.conv_epilogue(A, op, variant="relu_before_res"),
    }
    if Hin > 1 and Win > 1:             # a corner tap of a one-pixel-wide image meets padding only
        keep = np.ones((9, c.Cin), dtype=bool)
        keep[8] = False
        out["corner tap (2, 2) dropped"] = ec.conv_epilogue(ec.conv_acc(c, op["ix"], op["iw"], keep=keep), op)
    if Hin * Win > 1:                   # a 1 x 1 image meets the centre tap only
        out["ky / kx swapped in the weight"] = ec.conv_epilogue(ec.conv_acc(c, op["ix"], op["iw"], swap_kyx=True), op)
    if c.Ho != c.Wo:
        ct = dataclasses.replace(c, Ho=c.Wo, Wo=c.Ho)
        At = ec.conv_acc(ct, op["ix"].reshape(c.B, Win, Hin, c.Cin), op["iw"]).reshape(A.shape)      # the same memory, the sides mixed up
        out["H and W swapped"] = ec.conv_epilogue(At, op)
    return out


@pytest.mark.parametrize("name", list(ALL_CONV))
def test_conv_wrong_variants_change_at_least_one_per_cent(name):
    c = ALL_CONV[name]
    case = ec.conv_case(c)
    ref = ec.conv_epilogue(case["A"], case["op"])
    rep = {v: _changed(out, ref) for v, out in _conv_variants(c, case).items()}
    print(name, {v: round(f, 4) for v, f in rep.items()})
    for v, f in rep.items():
        assert f >= MIN_CHANGED, (name, v, f)


@pytest.mark.parametrize("name", list(ec.SPLITK_CASES))
def test_a_splitk_piece_one_step_short_changes_at_least_one_per_cent(name):
    c, res, bn, counts = ec.SPLITK_CASES[name]
    case = ec.conv_case(c)
    op = case["op"]
    ref = ec.conv_epilogue(case["A"], op, True, bn, res, True)
    nk = 9 * c.Cin // 64
    for splits in counts:
        ranges = ec.splitk_ranges(nk, splits)
        assert ranges[0][0] == 0 and ranges[-1][1] == nk and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(ranges, ranges[1:] + [(nk, nk + 1)]))
        s = splits // 2
        steps = [t for i, (k0, k1) in enumerate(ranges) for t in range(k0, k1 - (1 if i == s else 0))]
        assert len(steps) == nk - 1
        wrong = ec.conv_epilogue(ec.conv_acc(c, op["ix"], op["iw"], keep=ec.conv_keep_steps(c, steps)), op, True, bn, res, True)
        f = _changed(wrong, ref)
        assert f >= MIN_CHANGED, (name, splits, f)
        whole = ec.conv_acc(c, op["ix"], op["iw"], keep=ec.conv_keep_steps(c, range(nk)))
        assert np.array_equal(whole, case["A"])


def test_the_splitk_token_case_has_an_exact_positional_output_for_every_layer_kind():
    """pe_output asserts that the float32 add equals the float64 one; the second output differs from the first, so it is checked at all"""
    c, counts = ec.SPLITK_KINDS_CASE
    case = ec.conv_case(c)
    assert c.M == 64 and c.pe_period == c.M and all(1 <= s <= 9 * c.Cin // 64 for s in counts)
    for flags in KINDS:
        ref = ec.conv_epilogue(case["A"], case["op"], *flags).reshape(c.M, c.Cout)
        assert _changed(ec.pe_output(ref, case["op"]["pe"]), ref) >= 0.5, flags


@pytest.mark.parametrize("name", list(ALL_LINEAR))
def test_linear_wrong_variants_change_at_least_one_per_cent(name):
    c = ALL_LINEAR[name]
    case = ec.linear_case(c)
    op, A = case["op"], case["A"]
    ref = ec.linear_epilogue(A, op)
    rep = {"double rounding": ec.linear_epilogue(A, op, variant="double"), "round toward zero": ec.linear_epilogue(A, op, rnd=ec.f16_toward_zero),
           "round half away from zero": ec.linear_epilogue(A, op, rnd=ec.f16_half_away)}
    if c.K > 64:
        keep = ec.linear_keep_steps(c, range(c.K // 64 - 1))
        rep["last k-step dropped"] = ec.linear_epilogue(op["ix"][:, keep] @ op["iw"][:, keep].T, op)
    rep = {v: _changed(out, ref) for v, out in rep.items()}
    print(name, {v: round(f, 4) for v, f in rep.items()})
    for v, f in rep.items():
        assert f >= MIN_CHANGED, (name, v, f)


@pytest.mark.parametrize("c", ec.CONV7_CASES, ids=lambda c: c.name)
def test_conv7x7_wrong_variants_change_at_least_one_per_cent(c):
    case = ec.conv7_case(c)
    op, A = case["op"], case["A"]
    ref = ec.conv_epilogue(A, op, res=False)
    rep = {"single rounding of acc + bias": ec.conv_epilogue(A, op, res=False, variant="single_bias"),
           "round toward zero": ec.conv_epilogue(A, op, res=False, rnd=ec.f16_toward_zero),
           "round half away from zero": ec.conv_epilogue(A, op, res=False, rnd=ec.f16_half_away),
           "pad 2 instead of 3": ec.conv_epilogue(ec.conv7_acc(c, op["ix"], op["iw"], pad=2), op, res=False)}
    rep = {v: _changed(out, ref) for v, out in rep.items()}
    print(c.name, {v: round(f, 4) for v, f in rep.items()})
    for v, f in rep.items():
        assert f >= MIN_CHANGED, (c.name, v, f)
    # ... and against amp_util.conv_amp_ref (stride 2, its padding is (7 - 1) / 2 = 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    want, _, _ = conv_amp_ref(t(op["ix"] * 2.0 ** -ec.X_EXP), t(op["iw"] * 2.0 ** -ec.W_EXP), t(op["bias"]), (t(op["scale"]), t(op["shift"])), 2)
    assert np.array_equal(ref.transpose(0, 3, 1, 2), want.double().numpy())
