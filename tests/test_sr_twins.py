"""The integer twins of tests/sr_twins.py on the CPU: the conditions their exactness rests on, their reach, what they mean to the
project's own references, and that every planted index-level defect changes the output.  Each test takes a few seconds; the
twins and their activations on the 8 samples are computed once per process and never modified."""
import numpy as np
import pytest

import sr_twins as tw

LOG2E = tw.LOG2E
SEEDS = [pytest.param(s, id=f"seed{s}") for s in tw.TWIN_SEEDS]
_STATE = {}
N_REF = 3       # samples of the comparisons with the oracles (every layer shape is there at n = 1; 3 keeps a test to a few seconds)


def state(seed):
    """(K, J, x, y, acts, pre, S) on the 8 samples, condition-checked."""
    if seed not in _STATE:
        K, J = tw.integer_twin(seed)
        x = tw.inputs(8)
        y, acts, pre, S = tw.check_conditions(K, J, x)
        for a in [x, y] + acts + pre + S:
            a.setflags(write=False)
        _STATE[seed] = (K, J, x, y, acts, pre, S)
    return _STATE[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_conditions_hold(seed):
    """Conditions 1-3 (check_conditions: bands, 16-bit exactness of every stored activation, sums below 2^24) on every input, and
    5: the 16-bit outputs have a stated value."""
    K, J, x, y, acts, pre, S = state(seed)
    for name, u in zip(tw.LAYERS, pre):
        if tw.SWISH[name]:
            print(f"seed {seed} {name}: {float((u >= tw.HI).mean()):.2f} pass, {float((u <= tw.LO).mean()):.2f} killed, {float((u == 0).mean()):.2f} zero; max |sum| {S[tw.LAYERS.index(name)].max():.0f}")
    assert np.array_equal(y, np.rint(y)) and np.abs(y).max() < 65504
    for kind in ("float32", "bfloat16", "float16"):
        e = tw.expected_output(y, kind)
        assert e.dtype == np.float32 and np.isfinite(e).all()
    # the 8 samples are distinct, and larger batches never repeat a sample at a seam
    assert len({x[i].tobytes() for i in range(8)}) == 8
    o = tw.order(300)
    assert (o[1:] != o[:-1]).all() and not any(np.array_equal(o[8:8 + p], o[8 + p:8 + 2 * p]) for p in range(1, 60))


def test_affines_are_exact_in_float32():
    """Condition 4, on the largest batch the GPU tests use and with every seed's output."""
    aff, raw, out = tw.check_affines(300)
    for seed in tw.TWIN_SEEDS:
        y = state(seed)[3]
        exact = tw.check_out_affine_exact(y, out[:8])
        assert np.abs(exact).max() < 65504          # the f16 output with an affine stays finite
        # every row of the table on every sample
        for r in range(5):
            tw.check_out_affine_exact(y, np.tile(tw.out_affine(5)[r], (8, 1)))


@pytest.mark.parametrize("seed", SEEDS)
def test_richness(seed):
    K, J, x, y, acts, pre, S = state(seed)
    miss = tw.richness(K, J, x, y, acts, pre)
    assert not miss, "\n".join(miss)


def test_reach():
    """Over TWIN_SEEDS every MFMA k-step of every layer carries a non-zero weight, every (tap, channel) of the output convolution
    is read, and (richness) every output channel is non-zero somewhere."""
    miss = tw.unreached()
    assert not miss, f"no seed reaches {miss[0]} ({len(miss)} k-steps in all)"
    assert len(tw.k_steps(tw.integer_twin(0)[0])) == 36 + 100 + 4 + 4 + 144 + 8 + 4 + 2 + 1 + 72


def _to16(v32, kind):
    return tw.round_bf16(v32) if kind == "bf16" else np.asarray(v32, np.float32).astype(np.float16).astype(np.float32)


def test_scaled_encoding_packs_to_the_integers():
    """What operand_pack.cpp makes of the scaled encoding, restated: the 16-bit weight of every |k| <= 256 is k exactly, whether the
    pack multiplies by LOG2E, by 1.0 / LOG2E or divides by LOG2E (in double, then float32, then 16 bits); conv1's f32 weights and
    the f32 biases are k (1 + d), |d| <= 1e-7."""
    k = np.arange(-256, 257).astype(np.float64)
    div, mul = (k / LOG2E).astype(np.float32), (k * LOG2E).astype(np.float32)
    for kind in ("bf16", "f16"):
        for back in ((div.astype(np.float64) * LOG2E), (mul.astype(np.float64) * (1.0 / LOG2E)), (mul.astype(np.float64) / LOG2E)):
            assert np.array_equal(_to16(back.astype(np.float32), kind).astype(np.float64), k), kind
    f = (div.astype(np.float64) * LOG2E).astype(np.float32).astype(np.float64)
    d = np.abs(f[k != 0] / k[k != 0] - 1)
    print(f"scaled f32 weights and biases: max |d| {d.max():.2e}")
    assert d.max() <= 1e-7
    for seed in tw.TWIN_SEEDS:
        K, J = tw.integer_twin(seed)
        enc, dec = tw.encode(K, J, "scaled")
        w = {**enc, **dec}
        for name in tw.LAYERS:
            sk, sj = tw.SCALED[name]
            kk = w[f"{name}/kernel"].astype(np.float64)
            back = kk * LOG2E if sk == "/" else kk * (1.0 / LOG2E) if sk == "*" else kk
            if name != "conv2d":
                for kind in ("bf16", "f16"):
                    assert np.array_equal(_to16(back.astype(np.float32), kind).astype(np.float64), K[name]), (name, kind)
            assert w[f"{name}/kernel"].shape == tw.SHAPES[name] and w[f"{name}/kernel"].dtype == np.float32


def _report(got, want, label):
    msg = tw.describe_mismatch(got, want, label)
    assert msg is None, msg


@pytest.mark.parametrize("seed", SEEDS)
def test_float32_oracle_on_the_plain_encoding_is_the_integer_model(oracle, seed):
    """All eleven activations, assert_array_equal (-0 == +0)."""
    K, J, x, y, acts, pre, S = state(seed)
    enc, dec = tw.encode(K, J, "plain")
    z, ea = oracle.encoder_forward(x[:N_REF], enc, np.float32, return_all=True)
    yo, da = oracle.decoder_forward(z, dec, np.float32, return_all=True)
    assert yo.dtype == np.float32
    for name, got, want in zip(tw.LAYERS, ea + da, acts):
        _report(got.reshape(want[:N_REF].shape).astype(np.float64), want[:N_REF], f"seed {seed} {name}")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("seed", SEEDS)
def test_lowp_emulation_on_the_scaled_encoding_is_the_integer_model(seed, kind):
    """oracle.superres_forward_lowp: equal after rint, and within 1e-12 of max |y| before it (the float64 products
    (u / log2e) (log2e k)); the activations it returns (latent, the five transposed convolutions) the same, times log2e."""
    from oracle import sr_oracle_lowp as lp
    K, J, x, y, acts, pre, S = state(seed)
    enc, dec = tw.encode(K, J, "scaled")
    yo, ea = lp.superres_forward_lowp(x[:N_REF], enc, dec, kind, return_all=True)
    pairs = [("output_image_400", yo, y[:N_REF]), ("latent_vector", ea["latent"], acts[3][:N_REF])]
    pairs += [(tw.LAYERS[5 + i], ea[f"t{i}"] * LOG2E, acts[5 + i][:N_REF]) for i in range(5)]
    for name, got, want in pairs:
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"seed {seed} {kind} {name}: max error {err:.1e} of max |value|")
        _report(np.rint(got), want, f"seed {seed} {kind} {name} after rint")
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("encoding", ["scaled", "plain"])
@pytest.mark.parametrize("seed", SEEDS)
def test_float64_oracle_within_the_derived_bound(oracle, seed, encoding):
    """All eleven activations, element by element, within sr_twins.oracle_bound (saturation residue 2^-25 per swish layer, 2^-24 per
    float32-rounded scaled weight, carried through |K|)."""
    K, J, x, y, acts, pre, S = state(seed)
    enc, dec = tw.encode(K, J, encoding)
    z, ea = oracle.encoder_forward(x[:N_REF], enc, np.float64, return_all=True)
    yo, da = oracle.decoder_forward(z, dec, np.float64, return_all=True)
    bound = tw.oracle_bound(K, J, x[:N_REF], [a[:N_REF] for a in acts], [u[:N_REF] for u in pre], [s[:N_REF] for s in S], encoding)
    for name, got, want, b in zip(tw.LAYERS, ea + da, acts, bound):
        got = got.reshape(want[:N_REF].shape) * (LOG2E if encoding == "scaled" and tw.SWISH[name] else 1.0)
        err = np.abs(got - want[:N_REF])
        worst = float((err / np.maximum(b, 1e-300)).max())
        print(f"seed {seed} {encoding} {name}: max error {err.max():.2e}, max bound {b.max():.2e}, worst error / bound {worst:.3f}")
        assert (err <= b).all(), f"{name}: error {err.max():.3e} above the bound at {tuple(np.argwhere(err > b)[0])}"
    assert np.array_equal(np.rint(yo), y[:N_REF])


@pytest.mark.parametrize("defect", tw.PLANTED)
def test_planted_defect_changes_the_output(defect):
    """On every seed, at n = 2; the message the exact comparison would give names where."""
    for seed in tw.TWIN_SEEDS:
        K, J, x, y, acts, pre, S = state(seed)
        bad = tw.forward(K, J, x[:2], defect=defect)
        msg = tw.describe_mismatch(bad, y[:2], f"seed {seed} {defect}")
        assert msg is not None, f"seed {seed}: {defect} leaves the output unchanged"
        assert "first at" in msg and "bounding box" in msg and "mod 16" in msg
        print(msg)


# ------------------------------------------------------------------------------------------------------------------------
# the hardware-independent half of the saturation claim
# ------------------------------------------------------------------------------------------------------------------------
def _ulps(v32, k):
    """v32 moved by k float32 ulps (inf, 0 and denormals stay: the device's exp2 overflows and underflows exactly)."""
    v32 = np.asarray(v32, np.float32)
    out = (v32.view(np.int32) + np.int32(k)).view(np.float32)
    return np.where(np.isfinite(v32) & (np.abs(v32) >= np.float32(2.0 ** -125)), out, v32).astype(np.float32)


def _exp2_f32(t, k):
    with np.errstate(over="ignore"):
        return _ulps(np.exp2(np.asarray(t, np.float64)).astype(np.float32), k)


def _rcp_f32(d, k):
    with np.errstate(divide="ignore"):
        return _ulps((1.0 / np.asarray(d, np.float64)).astype(np.float32), k)


def swish_scaled(u, ke=0, kr=0):
    """dev16.h in float32 numpy: u * rcp(1 + exp2(-u)); the transcendentals in float64, rounded, moved by ke / kr ulps."""
    u = np.asarray(u, np.float32)
    return u * _rcp_f32(np.float32(1) + _exp2_f32(-u.astype(np.float64), ke), kr)


def swish_precise(v, ke=0, kr=0):
    """kernels_fp32.hip, act_apply_precise: max(v, -FLT_MAX) * rcp(1 + exp2(v * -log2e))."""
    v = np.asarray(v, np.float32)
    return np.maximum(v, np.float32(-3.402823466e38)) * _rcp_f32(np.float32(1) + _exp2_f32((v * np.float32(-1.4426950408889634)).astype(np.float64), ke), kr)


def swish_train(z, ke=0, kr=0):
    """act_device.h: z * sigmoid_fast(z), the reciprocal with its Newton step."""
    z = np.asarray(z, np.float32)
    den = np.float32(1) + _exp2_f32((z * np.float32(-1.4426950408889634)).astype(np.float64), ke)
    r = _rcp_f32(den, kr)
    with np.errstate(invalid="ignore"):
        res = (1.0 - den.astype(np.float64) * r.astype(np.float64)).astype(np.float32)     # fmaf(-den, r, 1): one rounding
        res = np.where(np.isfinite(den), np.minimum(res, np.float32(1)), np.float32(0))    # den = inf: fminf(NaN, 1) = 1, times r = 0
        s = (res.astype(np.float64) * r.astype(np.float64) + r.astype(np.float64)).astype(np.float32)
    return z * s


@pytest.mark.parametrize("fn", [swish_scaled, swish_precise, swish_train], ids=lambda f: f.__name__)
def test_saturated_swish_is_exact_in_float32(fn):
    """u on [25, 256], 0 at 0, -0 on [-2048, -130], with exp2 exact and 2 ulp off either way (the error the device's may have;
    rcp(1.0f) = 1.0f, exp2(x >= 128) = inf and rcp(inf) = 0 are the three hardware facts the GPU half rests on).  With the
    reciprocal 2 ulp off as well the pass band is no longer exact in float32, but still is after the 16-bit store of every layer."""
    up = np.arange(25, 257).astype(np.float32)
    down = -np.arange(130, 2049).astype(np.float32)
    for ke in (-2, 0, 2):
        got = fn(up, ke)
        assert np.array_equal(got, up), (ke, got[got != up][:4])
        assert fn(np.float32(0), ke) == 0
        got = fn(down, ke)
        assert np.array_equal(got, np.zeros_like(down)) and np.signbit(got).all(), ke
        for kr in (-2, 2):
            got = fn(up, ke, kr)
            if fn is not swish_train:        # (its Newton step repairs the reciprocal)
                assert not np.array_equal(got, up)
            assert np.array_equal(tw.round_bf16(got), up) and np.array_equal(got.astype(np.float16).astype(np.float32), up)
    # why the bands are where they are (the f32 kernels take x, not log2(e) x: their bands are wider by that factor)
    if fn is swish_scaled:
        assert fn(np.float32(17)) != 17
        leak = [u for u in (-129, -128, -127, -126) if fn(np.float32(u), -2) != 0 or fn(np.float32(u)) != 0]
        assert -126 in leak and -127 in leak, leak
    else:
        assert fn(np.float32(16)) != 16 and fn(np.float32(-87)) != 0
