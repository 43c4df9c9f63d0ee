"""CPU only: the data conditions of tests/linear_util.py hold for every case tests/test_gpu_linear.py launches, the kernels'
arithmetic restated in torch fp32 fits linear_bound (tests/transformer_check.py), and wrong arithmetic does not.

The mutants are value-only: a tanh-approximation GELU, the activation before the residual add, the pre-activation rounded to the
storage type before the activation, the neighbouring column's bias, erf(z) without the 1 / sqrt 2.  Each must exceed the bound in
the dtypes named below; torch's fp32 erf / tanh stand in for the device's (their own error is inside E: the correct restatement
fits)."""
import functools

import pytest
import torch

import linear_util as U
import transformer_check as T

ROWS = 400                                                  # the host-sized subset: every generic case whole, the others' first rows
IDS = [U.DT_NAMES[d] for d in U.DTYPES]


def cases_of(dt):
    return [c for c in U.all_cases() if c.dt == dt]


@functools.lru_cache(maxsize=None)
def prepared(c):
    """(inputs, reference, bound) of a case's host subset, computed once and shared by the tests below."""
    x, w, bias, res = U.make_inputs(c, rows=ROWS)
    r = T.linear_reference(x, w, bias, res, c.act, c.data != "random")
    return (x, w, bias, res), r, T.linear_bound(r, U.TORCH_DT[c.odt])


def test_the_table_is_what_it_says():
    """Every value of M, N and K with every activation; every activation with and without the residual; an fp32 output with act 2
    and 3 in both 16-bit types; the two-per-CU table's GELU launches in bf16 only."""
    for dt in U.DTYPES:
        for act in range(4):
            cs = U.generic_cases(dt, act)
            assert {c.M for c in cs} == {1, 127, 128, 129, 300} and {c.N for c in cs} == set(U.GENERIC_N)
            assert {c.K for c in cs} == {U.ktile(dt), 768} and {c.res for c in cs} == {False, True}
            assert {c.odt for c in cs} == ({dt} if dt == U.F32 else {dt, U.F32})
        if dt != U.F32:
            cs = U.duo_cases(dt)
            assert {c.M for c in cs} == {1024, 1025, 1151, 2600} and {c.N for c in cs} == {256, 768} and {c.K for c in cs} == {64, 128, 768, 3072}
            assert {(c.act, c.res) for c in cs} == {(a, r) for a in range(3 if dt == U.BF16 else 2) for r in (False, True)}
    names = [c.name for c in U.all_cases()]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("dt", U.DTYPES, ids=IDS)
def test_conditions_hold_for_every_dyadic_case(dt):
    n = 0
    for c in cases_of(dt):
        if c.data != "random":
            (x, w, bias, res), r, _ = prepared(c)
            U.check_conditions(c, x, w, bias, res, r["z"])
            n += 1
    assert n >= 36


def test_conditions_can_fail():
    c = next(c for c in U.generic_cases(U.F16, 3) if c.res and c.N >= 64)
    x, w, bias, res = U.make_inputs(c)
    U.check_conditions(c, x, w, bias, res)
    with pytest.raises(AssertionError):
        U.check_conditions(c, x + 0.0625, w, bias, res)                       # x off the 2^-3 grid
    wide = res.clone()
    wide[5, 5] = 257 * 2.0 ** -(3 + U.scale_exp(c.K))                          # nine significant bits: fp16 holds it, bf16 does not
    with pytest.raises(AssertionError, match="significant bits"):
        U.check_conditions(c, x, w, bias, wide)
    with pytest.raises(AssertionError, match="2\\^24"):
        U.check_conditions(c, x, w, bias + float(1 << 24), res)


@pytest.mark.parametrize("dt", U.DTYPES, ids=IDS)
def test_restatement_fits_the_bound(dt):
    """Correct arithmetic: worst |out - ref| / bound <= 1 over every case, printed per data kind and activation; on dyadic data with
    act 0 / 1 the restatement has the bits of the float64 value rounded once."""
    worst = {}
    for c in cases_of(dt):
        (x, w, bias, res), r, bound = prepared(c)
        out = U.restate(c, x, w, bias, res)
        wr, at = T.worst_ratio(out, r["ref"], bound)
        key = (c.data, U.ACT_NAMES[c.act], U.DT_NAMES[c.odt])
        worst[key] = max(worst.get(key, 0.0), wr)
        assert wr <= 1.0, (c.name, wr, at)
        if c.data != "random" and c.act <= 1:
            assert torch.equal(out, r["ref"].to(U.TORCH_DT[c.odt])), c.name
    for key, wr in sorted(worst.items()):
        print(f"\n[restated {U.DT_NAMES[dt]} {' '.join(key)}] worst |out - ref| / bound {wr:.3f}", end="")


# (mutant, the dtypes it must fail in, the cases it applies to)
DYADIC = lambda c: c.data != "random"                       # noqa: E731
MUTANTS = [("gelu_tanh", U.DTYPES, lambda c: DYADIC(c) and c.act == 2),
           ("act_before_res", U.DTYPES, lambda c: DYADIC(c) and c.act != 0 and c.res),
           # on the fine data: a dyadic z (a multiple of 2^-6 ... 2^-9 of a few units) IS an fp16 number wherever the activations bend,
           # and rounding it changes nothing (bf16's 8 bits do not hold it, but a narrow case has few elements to show it)
           ("round_z", (U.F16, U.BF16), lambda c: c.act >= 2 and c.data == "fine"),
           ("neighbour_bias", U.DTYPES, DYADIC),
           ("erf_no_sqrt2", U.DTYPES, lambda c: DYADIC(c) and c.act == 2)]


@pytest.mark.parametrize("mutant,dts,applies", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutants_exceed_the_bound(mutant, dts, applies):
    """Every case the mutation applies to fails, in every dtype named; the smallest worst ratio and the smallest share of
    elements off the bound are printed.  (The value mutants are asked of the dyadic cases: on random data
    the bound carries the pre-activation's error, (K + 2) 2^-24 of the sum of magnitudes, and at K = 768 in fp32 that alone is wider
    than what the tanh approximation is off by.  The exact data is there for this.)"""
    for dt in dts:
        ratios, shares = [], []
        for c in cases_of(dt):
            if not applies(c):
                continue
            (x, w, bias, res), r, bound = prepared(c)
            out = U.restate(c, x, w, bias, res, mutant)
            wr, _ = T.worst_ratio(out, r["ref"], bound)
            assert wr > 1.0, (mutant, c.name, wr)
            off = (out.double() - r["ref"]).abs() > bound
            ratios.append(wr)
            shares.append(float(off.double().mean()))
        assert len(ratios) >= 3, (mutant, dt)
        print(f"\n[{mutant} {U.DT_NAMES[dt]}] {len(ratios)} cases, worst ratio >= {min(ratios):.1f}, elements off the bound >= {min(shares):.1%}", end="")
