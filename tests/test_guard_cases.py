"""No GPU: the guard's numpy reference, the affine trigger and the planted defects of tests/guard_cases.py.

Shown here, on the float64 oracle's output of the fixed batch: the recipe's fields are bad in part, with every coverage
condition met for all three output types; the unplanted restatement of the guard epilogue equals `guard_ref`; and each of the
eight planted defects changes y or the counter on this data, i.e. would fail an assertion of test_gpu_nonfinite_guard.py.
"""
import numpy as np
import pytest

import guard_cases as gc
from conftest import STATS_TXT


@pytest.fixture(scope="module")
def ref(srcfd, enc_weights, dec_weights, coarse_cases):
    return gc.recipe_reference(enc_weights, dec_weights, coarse_cases, srcfd.load_stats(STATS_TXT, 10, 400)[0])


def _precision_for(out_dtype):
    # the arithmetic of the affine is the precision's, not the output type's: both forms are walked
    return {"float32": "fp32", "bfloat16": "bf16", "float16": "f16"}[out_dtype]


def test_casts_round_to_nearest_even_and_overflow_at_the_stated_thresholds():
    for dt, top in (("float16", np.float32(65504.0)), ("bfloat16", np.array(0x7F7F0000, np.uint32).view(np.float32)[()])):
        T = gc.OVERFLOW[dt]
        below = np.nextafter(T, np.float32(0))
        v = np.array([top, below, T, -below, -T, np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0], np.float32)
        y = gc.cast(v, dt)
        f = gc.to_f32(y, dt)
        assert f[0] == top and f[1] == top and f[2] == np.inf and f[3] == -top and f[4] == -np.inf
        assert f[5] == np.inf and f[6] == -np.inf and np.isnan(f[7]) and f[10] == 1.0
        assert gc.bits(y)[8] == 0 and gc.bits(y)[9] == 0x8000
        yg, cnt = gc.guard_ref(v, dt)
        assert cnt == 5 and gc.finite(yg, dt).all() and not gc.bits(yg)[[2, 4, 5, 6, 7]].any()
        np.testing.assert_array_equal(gc.bits(yg)[[0, 1, 3, 8, 9, 10]], gc.bits(y)[[0, 1, 3, 8, 9, 10]])
    # bfloat16 against an independent statement of the rounding: the nearer of the two neighbours, the even one on a tie
    rng = np.random.default_rng(0)
    v = rng.standard_normal(4096).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, 4096).astype(np.float32)
    v[:64] = ((np.arange(64, dtype=np.uint32) + 0x3F80) << 16 | 0x8000).view(np.float32)   # exact ties
    a = np.abs(v)                                            # sign and magnitude: the neighbours of |v|, the sign put back
    lo = (a.view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.float64)
    hi = ((a.view(np.uint32) & 0xFFFF0000) + 0x10000).view(np.float32).astype(np.float64)
    d = (a - lo) - (hi - a)
    lo_even = ((a.view(np.uint32) >> 16) & 1) == 0
    want = np.copysign(np.where((d < 0) | ((d == 0) & lo_even), lo, hi), v).astype(np.float32)
    np.testing.assert_array_equal(gc.to_f32(gc.cast(v, "bfloat16"), "bfloat16"), want)
    y32, cnt = gc.guard_ref(np.array([gc.FLT_MAX, np.inf, -np.inf, np.nan, 65520.0], np.float32), "float32")
    assert cnt == 3 and list(y32) == [gc.FLT_MAX, 0, 0, 0, 65520.0]


def test_fma32_rounds_once():
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a = rng.standard_normal(2000).astype(np.float32)
    b = rng.standard_normal(2000).astype(np.float32)
    c = (rng.standard_normal(2000) * 2.0 ** rng.integers(-30, 5, 2000)).astype(np.float32)
    # ties of the float32 result that only the sticky error decides: a * b lands on a midpoint, c is far below an ulp
    a[:500] = np.float32(1 + 2.0 ** -12)
    b[:500] = np.float32(1 + 2.0 ** -12)                       # 1 + 2^-11 + 2^-24: a midpoint of float32 at 2^-23 spacing
    c[:500] = (rng.choice([-1.0, 1.0], 500) * 2.0 ** rng.integers(-90, -60, 500)).astype(np.float32)
    got = gc.fma32(a, b, c)
    for i in range(2000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                          # float(Fraction) rounds once to 53 bits; walk to the bracketing pair
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda f: (abs(Fraction(float(f)) - exact), int(np.float32(f).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)
    assert gc.fma32(np.float32(3e38), np.float32(2.0), np.float32(0)) == np.inf
    assert gc.fma32(np.float32(-3e38), np.float32(2.0), np.float32(1e38)) == -np.inf


@pytest.mark.parametrize("out_dtype", gc.OUT_DTYPES)
def test_the_recipe_delivers_every_coverage_condition(ref, out_dtype):
    """Measured here (float64 oracle, fixed_batch(3), rows (0.90, 0), (0.80, +T/8), (0.97, -T/8)): the shares are printed; they
    are 1 - Q up to the shift by the mean, except float32's third sample, whose std is held at FLT_MAX."""
    acc = ref["acc"]
    prec = _precision_for(out_dtype)
    aout = gc.trigger_rows(acc, out_dtype)
    assert np.isfinite(aout).all() and (aout[:, 1] > 0).all() and aout[1, 0] > 0 > aout[2, 0] and aout[0, 0] == 0
    v = gc.affine_ref(acc, aout, prec)
    f = gc.to_f32(gc.cast(v, out_dtype), out_dtype)
    assert not np.isnan(f).any()
    cov, share = gc.coverage(~np.isfinite(f), f == np.inf, f == -np.inf)
    print(f"{out_dtype} ({prec}): bad share per sample {np.array2string(share, precision=4)}; +Inf {(f == np.inf).sum()}, -Inf {(f == -np.inf).sum()}")
    assert all(cov.values()), cov
    if out_dtype != "float32":     # the case the float32 test of the value cannot see: finite in float32, Inf in y's type
        assert (np.isfinite(v) & ~np.isfinite(f)).any()


@pytest.mark.parametrize("out_dtype", gc.OUT_DTYPES)
def test_every_planted_defect_changes_y_or_the_count(ref, out_dtype):
    acc = ref["acc"]
    prec = _precision_for(out_dtype)
    v = gc.affine_ref(acc, gc.trigger_rows(acc, out_dtype), prec)
    # the second batch of the GPU module: a triggered sample, one with std = 1, one that a NaN input made NaN throughout
    aout_b = gc.trigger_rows(acc, out_dtype)
    aout_b[1] = (0.0, 1.0)
    v_b = gc.affine_ref(acc, aout_b, prec)
    v_b[2] = np.nan
    for seg in (1, 5, 25):
        for name, vv in (("three triggered", v), ("triggered | std = 1 | NaN", v_b)):
            y_ref, cnt = gc.guard_ref(vv, out_dtype)
            y, counter = gc.guard_epilogue(vv, out_dtype, seg=seg)
            assert counter == gc.START + cnt and np.array_equal(gc.bits(y), gc.bits(y_ref)), (name, seg)
            assert gc.finite(y, out_dtype).all()
    np.testing.assert_array_equal(gc.bits(gc.guard_ref(v_b, out_dtype)[0][1]), gc.bits(gc.cast(acc[1], out_dtype)))
    assert gc.guard_ref(v_b[2:], out_dtype)[1] == gc.H * gc.W
    tripped = {}
    for d in gc.DEFECTS:
        hits = []
        for name, vv in (("triggered", v), ("with_nan", v_b)):
            y_ref, cnt = gc.guard_ref(vv, out_dtype)
            y, counter = gc.guard_epilogue(vv, out_dtype, defect=d)
            if not np.array_equal(gc.bits(y), gc.bits(y_ref)):
                hits.append(f"{name}: y")
            if not gc.finite(y, out_dtype).all():
                hits.append(f"{name}: non-finite y")
            if counter != gc.START + cnt:
                hits.append(f"{name}: counter")
        tripped[d] = hits
    print(out_dtype, tripped)
    for d, hits in tripped.items():
        if d == "a_test_before_cast" and out_dtype == "float32":
            assert not hits        # float32: the cast is the identity, the two orders are the same code
            continue
        assert hits, f"{out_dtype}: planted defect {d} ({gc.DEFECTS[d]}) changes nothing on this data"


def test_nan_footprint_follows_the_layer_geometry():
    m = gc.nan_footprint(5, 7)
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    assert (rows[0], rows[-1], cols[0], cols[-1]) == (32 * 5 - 1, 32 * 5 + 48, 32 * 7 - 1, 32 * 7 + 48) and m.sum() == 50 * 50
    m0, m11 = gc.nan_footprint(0, 0), gc.nan_footprint(11, 11)
    assert m0[0, 0] and m0[48, 48] and not m0[49].any() and m11[399, 399] and m11[351, 351] and not m11[350].any()
    # the same set from the float64 oracle: a NaN in that bias unit, everything else finite
    from oracle import sr_oracle as o
    dec = o.synthetic_decoder(1)
    dec = dict(dec, **{"dense_1/bias": dec["dense_1/bias"].copy()})
    dec["dense_1/bias"][gc.nan_unit(5, 7, 3)] = np.nan
    y = o.decoder_forward(np.zeros((1, 50)), dec, np.float64)[0, ..., 0]
    np.testing.assert_array_equal(np.isnan(y), m)
