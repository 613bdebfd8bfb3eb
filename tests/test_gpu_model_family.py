"""The notebook's model family and Conv2DTranspose(padding='same') on an MI355X: single layers and whole encoder_10 + decoder_X
models against the float64 reference of tests/family_ref.py (the project's f32 bar, relative L2 <= 1e-5), training gradients
against float64 autograd under the rule of tests/test_gpu_training_oracle.py, and the warm start of a 100x100 fine solve from a
10 -> 100 model without a resampler."""
import importlib
import os

import numpy as np
import pytest

import family_ref as fr
from conftest import STATS_TXT, require_gpu

pytestmark = pytest.mark.gpu
TOL_FP32 = 1e-5
HRS = (10, 20, 50, 80, 100)


def _family():
    return importlib.import_module("sr-for-cfd_amd.family")


# ---------------------------------------------------------------------------
# single layers
# ---------------------------------------------------------------------------
# (k, s, h, w, cin, cout): the widest layer of the family (decoder_50 / 100's first), one pixel, odd sizes and channel counts,
# the narrow-channel layer of decoder_80, stride 1, pb > 0 with an even and an odd kernel, and kernel == stride
SAME_CASES = [(3, 2, 3, 3, 512, 256), (3, 2, 1, 1, 8, 8), (3, 2, 5, 7, 3, 5), (3, 2, 12, 12, 32, 16), (3, 1, 4, 5, 8, 8), (4, 2, 3, 4, 8, 8),
              (5, 2, 3, 3, 4, 4), (2, 2, 4, 4, 16, 8)]


def _layer(case, same=True, act="swish"):
    k, s, h, w, cin, cout = case
    rng = np.random.default_rng(1000 * k + 100 * s + cin)
    wt = (rng.standard_normal((k, k, cout, cin)) / np.sqrt(cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    x = rng.standard_normal((3, h, w, cin)).astype(np.float32)
    return [dict(kind="conv2d_transpose", name="up", k=k, stride=s, same=same, act=act, w=wt, b=b)], x


@pytest.mark.parametrize("precision", ["fp32", "fp32_naive"])
@pytest.mark.parametrize("case", SAME_CASES, ids=["k%ds%d_%dx%d_%dto%d" % c for c in SAME_CASES])
def test_single_same_layers(srcfd, oracle, case, precision):
    require_gpu(srcfd)
    k, s, h, w, cin, cout = case
    specs, x = _layer(case)
    ref = fr.forward_specs64(specs, x)
    m = srcfd.SRModel.from_layers(specs, (h, w, cin), device=0)
    m.precision = precision
    for n in (1, 3):
        y = m.predict(x[:n])
        assert y.shape == (n, h * s, w * s, cout)
        err = oracle.rel_l2(y, ref[:n])
        print(f"same k{k}s{s} {h}x{w} {cin}->{cout} {precision} n={n}: rel L2 {err:.2e}")
        assert err <= TOL_FP32
    if k == s:   # 'same' and 'valid' are one layer: the same kernels, the same bits
        v = srcfd.SRModel.from_layers(_layer(case, same=False)[0], (h, w, cin), device=0)
        v.precision = precision
        np.testing.assert_array_equal(m.predict(x).view(np.uint32), v.predict(x).view(np.uint32))


def test_same_layer_on_the_split_bf16_gemm(srcfd, oracle):
    """SRCFD_PREC_FP32X3 takes the wide SAME layers from 64 samples on (their four cropped phases as one launch of
    kernels_x3.hip): 70 samples of the 512 -> 256 layer against float64 at the f32 bar; the kernel ran; rows do not depend on
    the batch."""
    require_gpu(srcfd)
    case = SAME_CASES[0]
    k, s, h, w, cin, cout = case
    specs, _ = _layer(case)
    x = np.random.default_rng(70).standard_normal((70, h, w, cin)).astype(np.float32)
    ref = fr.forward_specs64(specs, x)
    m = srcfd.SRModel.from_layers(specs, (h, w, cin), device=0)
    m.precision = "fp32x3"
    m.set_profiling(True)
    y = m.predict(x)
    names = [nm for nm, _ in m.get_profile()]
    m.set_profiling(False)
    assert any(nm.endswith("(x3)") for nm in names), names
    err = oracle.rel_l2(y, ref)
    print(f"same k3s2 512->256 fp32x3 n=70: rel L2 {err:.2e}")
    assert y.shape == ref.shape and err <= TOL_FP32
    np.testing.assert_array_equal(m.predict(x[3:68]), y[3:68])


@pytest.mark.parametrize("precision", ["fp32", "fp32_naive"])
def test_same_layer_known_answers(srcfd, precision):
    """k = 3, s = 2: a one-hot input at the last pixel with the one-hot tap (2, 2) lands outside the output (bias only);
    pixel (0, 0) with tap (0, 0) lands at out[0, 0]."""
    require_gpu(srcfd)
    h, w = 3, 4
    bias = np.array([0.25], np.float32)
    for pix, tap, where in (((h - 1, w - 1), (2, 2), None), ((0, 0), (0, 0), (0, 0)), ((h - 1, w - 1), (1, 1), (2 * h - 1, 2 * w - 1))):
        wt = np.zeros((3, 3, 1, 1), np.float32)
        wt[tap[0], tap[1], 0, 0] = 2.0
        x = np.zeros((1, h, w, 1), np.float32)
        x[0, pix[0], pix[1], 0] = 3.0
        m = srcfd.SRModel.from_layers([dict(kind="conv2d_transpose", k=3, stride=2, same=True, act="linear", w=wt, b=bias)], (h, w, 1), device=0)
        m.precision = precision
        want = np.full((1, 2 * h, 2 * w, 1), 0.25, np.float32)
        if where is not None:
            want[0, where[0], where[1], 0] = 6.25
        np.testing.assert_array_equal(m.predict(x), want)


# ---------------------------------------------------------------------------
# whole models
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields(srcfd, coarse_cases):
    """Six of the golden coarse fields: raw float32 (6, 10, 10, 1) and their (mean, std) pairs."""
    lr, _ = srcfd.load_stats(STATS_TXT, 10, 400)
    xs, aff = [], []
    for case in list(coarse_cases.values())[:2]:
        for c in ("u", "v", "p"):
            xs.append(case[c].astype(np.float32))
            aff.append(lr[c])
    return np.stack(xs)[..., None], np.asarray(aff, np.float32)


_MODELS = {}


def _model_case(srcfd, enc_weights, fields, hr):
    """(specs, standardised inputs, float64 reference) of encoder_10 + a seeded decoder_{hr}: computed once."""
    if hr not in _MODELS:
        dec = _family().synthetic_decoder_weights(hr, seed=20 + hr)
        specs = srcfd.layers_from_weights(enc_weights, dec)
        x, ain = fields
        xn = ((x - ain[:, 0].reshape(-1, 1, 1, 1)) / ain[:, 1].reshape(-1, 1, 1, 1)).astype(np.float32)
        _MODELS[hr] = (specs, dec, xn, fr.forward_specs64(specs, xn))
    return _MODELS[hr]


@pytest.mark.parametrize("hr", HRS)
def test_encoder10_decoder_x_fp32(srcfd, oracle, enc_weights, fields, hr):
    require_gpu(srcfd)
    specs, dec, xn, ref = _model_case(srcfd, enc_weights, fields, hr)
    x, ain = fields
    m = srcfd.SRModel.from_weights(enc_weights, dec, device=0)
    assert m.output_shape == (hr, hr, 1)
    y = m.predict(xn)
    err = oracle.rel_l2(y, ref)
    print(f"encoder_10 + decoder_{hr} fp32: rel L2 vs float64 {err:.2e}")
    assert y.shape == (6, hr, hr, 1) and err <= TOL_FP32
    m.precision = "fp32_naive"
    assert oracle.rel_l2(m.predict(xn), ref) <= TOL_FP32
    m.precision = "fp32"
    # in / out affines: float32 (x - mean) / std in front, float32 y * std + mean behind, two roundings each (srcfd.h)
    rng = np.random.default_rng(hr)
    aout = np.stack([rng.standard_normal(6) * 0.1, rng.uniform(0.05, 0.3, 6)], 1).astype(np.float32)
    ya = m.predict(x, in_affine=ain, out_affine=aout)
    want = y * aout[:, 1].reshape(-1, 1, 1, 1) + aout[:, 0].reshape(-1, 1, 1, 1)
    assert want.dtype == np.float32
    np.testing.assert_array_equal(ya.view(np.uint32), want.view(np.uint32))
    # a sample's bits do not depend on the batch it rides in, nor on its place: the six fields first, in the middle and last of 130
    np.testing.assert_array_equal(m.predict(xn[2:5]), y[2:5])
    xb = rng.standard_normal((130, 10, 10, 1)).astype(np.float32)
    for at in (0, 62, 124):
        xb[at:at + 6] = xn
    yb = m.predict(xb)
    for at in (0, 62, 124):
        np.testing.assert_array_equal(yb[at:at + 6].view(np.uint32), y.view(np.uint32))
    if hr == 50:
        # 1024 samples: conv2d_transpose_1 ('same', 256 -> 128 on 6x6) then has 4 x 288 tiles and takes the large-launch GEMM
        # (gemm32_big_qualifies: >= 1024), bit-identical to the grouped launch of the small batch
        big = m.predict(np.concatenate([xn] * 171)[:1024])
        np.testing.assert_array_equal(big[:6], y)
        np.testing.assert_array_equal(big[1020:1024], y[:4])
    # NaN guard: one poisoned input sample is zero-filled and counted, its neighbours keep their bits
    xb = xn.copy()
    xb[1, 4, 4, 0] = np.nan
    yb, bad = m.predict(xb, nan_guard=True, return_nonfinite=True)
    assert bad == hr * hr and np.isfinite(yb).all() and not yb[1].any()
    np.testing.assert_array_equal(yb[[0, 2, 3, 4, 5]], y[[0, 2, 3, 4, 5]])


def test_keras_surface_runs_a_family_decoder_file(srcfd, enc_weights, fields, tmp_path):
    """`load_model` of the encoder / decoder_100 files and `SuperResolutionAE(encoder, decoder).predict`, as the solver scripts
    do it: the bits of the handle built from the same weights."""
    require_gpu(srcfd)
    kc = importlib.import_module("sr-for-cfd_amd.keras_compat")
    specs, dec, xn, ref = _model_case(srcfd, enc_weights, fields, 100)
    e, d = str(tmp_path / "vanilla_encoder10_to_100_t.h5"), str(tmp_path / "vanilla_decoder100_from_10_t.h5")
    srcfd.SRModel.from_weights(enc_weights, dec, device=-1).save_h5(e, d)

    class SuperResolutionAE(kc.Model):
        def __init__(self, encoder_lr, decoder_hr, **kw):
            super().__init__(**kw)
            self.encoder_lr, self.decoder_hr = encoder_lr, decoder_hr

        def call(self, inputs, training=False):
            return self.decoder_hr(self.encoder_lr(inputs, training=training), training=training)

    want = srcfd.SRModel.from_weights(enc_weights, dec, device=0).predict(xn)
    try:
        y = SuperResolutionAE(kc.load_model(e, compile=False), kc.load_model(d, compile=False)).predict(xn, verbose=0)
        assert y.shape == (6, 100, 100, 1)
        np.testing.assert_array_equal(y, want)
        z = kc.load_model(e, compile=False).predict(xn)
        y2 = kc.load_model(d, compile=False).predict(z)        # the two files one after the other: the same f32 arithmetic
        assert np.linalg.norm(y2 - want) <= 1e-6 * np.linalg.norm(want)
        # precision="bf16": the handle runs what srcfd_model_supports_precision allows -- the 16-bit path for this graph
        y16 = SuperResolutionAE(kc.load_model(e, compile=False), kc.load_model(d, compile=False), precision="bf16").predict(xn, verbose=0)
        h16 = kc._device_handle((e, d), "bf16")
        assert h16.supports_precision("bf16") and h16.precision == "bf16" and h16.last_plan()["decoder"] == "any16"
        assert not np.array_equal(y16, want) and np.linalg.norm(y16 - want) <= 2e-2 * np.linalg.norm(want)
    finally:
        kc.clear_handle_cache()


# ---------------------------------------------------------------------------
# the same five models in bf16 and f16 (any16: enc16 -> gemm16 / gemm16n per layer -> outconv16)
# ---------------------------------------------------------------------------
_EMU = {}


def _emu(srcfd, enc_weights, fields, hr, kind):
    if (hr, kind) not in _EMU:
        specs, dec, xn, ref = _model_case(srcfd, enc_weights, fields, hr)
        _EMU[(hr, kind)] = fr.forward_specs_lowp(specs, xn, kind)
    return _EMU[(hr, kind)]


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("hr", HRS)
def test_encoder10_decoder_x_16bit(srcfd, oracle, enc_weights, fields, hr, kind):
    """Device against the CPU emulation of the same roundings (tests/family_ref.py, the rules of oracle/sr_oracle_lowp.py): within
    test_gpu_parity_bf16.py's TOL[kind][0], taken as a ceiling; against float64: at most the emulation's own distance from
    float64 + that ceiling; the median over the samples within MEDIAN_EMU[kind].  Batches of 6, 7 and 130 (1030 for decoder_10:
    past the 1024-sample capacity), and the six fields placed first, in the middle and last of 130 have the bits of the batch
    of six.  16-bit outputs are the rounding of the f32 output of the same call."""
    require_gpu(srcfd)
    import torch
    from test_gpu_parity_bf16 import MEDIAN_EMU, TOL, per_sample_rel_l2
    specs, dec, xn, ref = _model_case(srcfd, enc_weights, fields, hr)
    emu = _emu(srcfd, enc_weights, fields, hr, kind)
    m = srcfd.SRModel.from_weights(enc_weights, dec, device=0)
    assert m.supports_precision(kind)
    m.precision = kind
    y = m.predict(xn)
    plan = m.last_plan()
    assert plan["decoder"] == "any16" and plan["encoder"] == "enc16" and plan["precision"] == kind
    e_emu, e_64, emu_64 = per_sample_rel_l2(y, emu), per_sample_rel_l2(y, ref), per_sample_rel_l2(emu, ref)
    print(f"encoder_10 + decoder_{hr} {kind}: vs emulation max {e_emu.max():.2e} median {np.median(e_emu):.2e}; vs float64 max {e_64.max():.2e} "
          f"(emulation vs float64 {emu_64.max():.2e})")
    assert e_emu.max() <= TOL[kind][0]
    assert e_64.max() <= emu_64.max() + TOL[kind][0]
    assert np.median(e_emu) <= MEDIAN_EMU[kind]
    # a sample's bits depend neither on the batch size nor on its position
    rng = np.random.default_rng(hr)
    for n in (7, 130) + ((1030,) if hr == 10 else ()):
        xb = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
        places = (0,) if n == 7 else (0, (n - 6) // 2, n - 6)
        for at in places:
            xb[at:at + 6] = xn
        yb = m.predict(xb)
        assert np.isfinite(yb).all()
        for at in places:
            np.testing.assert_array_equal(yb[at:at + 6].view(np.uint32), y.view(np.uint32))
    # the layer-by-layer encoder (SRCFD_ENC=0, the functional A/B switch of the fused path) under the same bounds
    os.environ["SRCFD_ENC"] = "0"
    try:
        yl = m.predict(xn)
        assert m.last_plan()["encoder"] == "layers" and m.last_plan()["decoder"] == "any16"
    finally:
        del os.environ["SRCFD_ENC"]
    assert per_sample_rel_l2(yl, emu).max() <= TOL[kind][0]
    # affine + NaN guard: y std + mean as ONE fma of the f32 result (srcfd.h, the 16-bit precisions); a poisoned sample is zero-filled
    aout = np.stack([rng.standard_normal(6) * 0.1, rng.uniform(0.05, 0.3, 6)], 1).astype(np.float32)
    ya = m.predict(xn, out_affine=aout)
    want = (y.astype(np.float64) * aout[:, 1].reshape(-1, 1, 1, 1).astype(np.float64) + aout[:, 0].reshape(-1, 1, 1, 1).astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(ya.view(np.uint32), want.view(np.uint32))
    xp = xn.copy()
    xp[1, 4, 4, 0] = np.nan
    yp, bad = m.predict(xp, nan_guard=True, return_nonfinite=True)
    assert bad == hr * hr and not yp[1].any()
    np.testing.assert_array_equal(yp[[0, 2, 3, 4, 5]], y[[0, 2, 3, 4, 5]])
    # predict_device with 16-bit output: every element is the rounding of the f32 output of the same call
    xd = torch.from_numpy(xn).cuda()
    y32 = torch.empty((6, hr, hr, 1), dtype=torch.float32, device="cuda")
    m.predict_device(xd, y32)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y32.cpu().numpy(), y)
    for dt in (torch.bfloat16, torch.float16):
        y16 = torch.empty((6, hr, hr, 1), dtype=dt, device="cuda")
        m.predict_device(xd, y16)
        torch.cuda.synchronize()
        assert torch.equal(y16.view(torch.int16).cpu(), y32.to(dt).view(torch.int16).cpu())


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_16bit_graph_replay_and_side_stream(srcfd, enc_weights, fields, kind):
    """encoder_10 + decoder_80 (the narrow-channel GEMM runs): three identical calls at n = 3 give identical bits and the third is a
    hipGraph replay; one call on a non-default stream behind the delay of tests/stream_order.py equals the default-stream result."""
    require_gpu(srcfd)
    import torch
    import stream_order as so
    specs, dec, xn, ref = _model_case(srcfd, enc_weights, fields, 80)
    m = srcfd.SRModel.from_weights(enc_weights, dec, device=0)
    m.precision = kind
    xd = torch.from_numpy(xn[:3]).cuda()
    y = torch.empty((3, 80, 80, 1), dtype=torch.float32, device="cuda")
    outs, graphs = [], []
    for _ in range(3):
        y.fill_(7.0)
        m.predict_device(xd, y)
        torch.cuda.synchronize()
        outs.append(y.clone())
        graphs.append(m.last_plan()["graph"])
    assert graphs[2] == "replay", graphs
    so.assert_bit_equal(outs[1], outs[0], "second call")
    so.assert_bit_equal(outs[2], outs[0], "replayed call")
    np.testing.assert_array_equal(outs[0].cpu().numpy(), m.predict(xn[:3]))
    delay, side = so.Delay(torch), torch.cuda.Stream()
    slot, y2 = torch.empty_like(xd), torch.empty_like(y)
    out = so.delayed_call(torch, delay, side, [so.Arrival(slot, xd * 0.5 + 1.0, xd)], lambda: m.predict_device(slot, y2), [y2],
                          stale=[(y2, torch.full_like(y2, 3.0))], label=f"any16 {kind}")
    so.assert_pending(out, f"any16 {kind} predict_device")
    so.assert_bit_equal(out.clones[0], outs[0], f"any16 {kind} on a side stream")


def test_other_encoders_run_in_fp32(srcfd, oracle):
    """encoder_50 + decoder_100 (four strided convolutions in front): forward only, through the generic f32 plan."""
    require_gpu(srcfd)
    fam = _family()
    enc, dec = fam.synthetic_encoder_weights(50, seed=3), fam.synthetic_decoder_weights(100, seed=4)
    specs = fam.layers_from_weights(enc, dec, 50, 100)
    x = np.random.default_rng(5).standard_normal((3, 50, 50, 1)).astype(np.float32)
    m = srcfd.SRModel.from_weights(enc, dec, device=0, lr_dim=50)
    y = m.predict(x)
    assert y.shape == (3, 100, 100, 1) and oracle.rel_l2(y, fr.forward_specs64(specs, x)) <= TOL_FP32
    with pytest.raises(ValueError, match="strided Conv2D"):
        importlib.import_module("sr-for-cfd_amd.train").Trainer(m, max_batch=2)


# ---------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hr", [10, 50])
def test_training_gradients_match_float64_autograd(srcfd, oracle, enc_weights, hr):
    """Trainer on encoder_10 + decoder_10 / decoder_50 (padding='same' layers in the data-gradient chain and in the weight
    gradients), batches of 2 and 3: loss and every gradient tensor under `check` of tests/test_gpu_training_oracle.py; then two
    optimiser steps, and the exported model predicts with the updated weights."""
    require_gpu(srcfd)
    import torch
    from test_gpu_training_oracle import check, device_step
    tr = importlib.import_module("sr-for-cfd_amd.train")
    dec = _family().synthetic_decoder_weights(hr, seed=30 + hr)
    specs = srcfd.layers_from_weights(enc_weights, dec)
    t = tr.Trainer(srcfd.SRModel.from_layers(specs, (10, 10, 1), device=0), max_batch=3)
    assert t.plan["fused_tail"] == 0
    rng = np.random.default_rng(40 + hr)
    for n in (2, 3):
        x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
        y = rng.standard_normal((n, hr, hr, 1)).astype(np.float32)
        y[:, :1] += 2.0
        y[:, :, -1:] -= 2.0
        ref = fr.GradRef(specs, (10, 10, 1), x, y)
        assert t.n_params == ref.g64.size
        loss, g = device_step(t, x, y)
        check(f"encoder_10+decoder_{hr} n={n}", ref, loss, g)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    before = t.params.clone()
    l1 = t.step(xd, yd)
    l2 = t.step(xd, yd)
    assert np.isfinite([l1, l2]).all() and not torch.equal(before, t.params)
    w = t.weights()
    new_specs = [dict(s, w=w[f"{s['name']}/kernel"], b=w[f"{s['name']}/bias"]) if "w" in s else s for s in specs]
    m = t.export_model()
    assert oracle.rel_l2(m.predict(x), fr.forward_specs64(new_specs, x)) <= TOL_FP32
    t.close()


@pytest.mark.parametrize("k,s", [(4, 2), (5, 2), (3, 1)])
def test_training_gradients_of_same_layers_with_a_shifted_origin(srcfd, k, s):
    """pb = (k - s) // 2 > 0: the data gradient reads dZ at s i + a - pb (negative origins at the top / left border) and the forward
    phases start inside the VALID result.  A small front convolution, the 'same' transposed convolution under test, a 3x3 output
    convolution; batches of 1 and 3 under the rule of tests/test_gpu_training_oracle.py."""
    require_gpu(srcfd)
    from test_gpu_training_oracle import check, conv, device_step
    tr = importlib.import_module("sr-for-cfd_amd.train")
    rng = np.random.default_rng(100 * k + s)
    lim = np.sqrt(3.0 / (max(1.0, (k / s) ** 2) * 8))
    specs = [conv(rng, "front", 3, 2, 8),
             dict(kind="conv2d_transpose", name="lut", k=k, stride=s, same=True, act="swish", w=rng.uniform(-lim, lim, (k, k, 5, 8)).astype(np.float32),
                  b=(0.1 * rng.standard_normal(5)).astype(np.float32)),
             conv(rng, "out", 3, 5, 1, act="linear")]
    in_shape = (5, 4, 2)
    m = srcfd.SRModel.from_layers(specs, in_shape, device=0)
    assert m.output_shape == (5 * s, 4 * s, 1)
    t = tr.Trainer(m, max_batch=3)
    for n in (1, 3):
        x = rng.standard_normal((n,) + in_shape).astype(np.float32)
        y = rng.standard_normal((n, 5 * s, 4 * s, 1)).astype(np.float32)
        y[:, :1] += 2.0
        y[:, :, -1:] -= 2.0
        ref = fr.GradRef(specs, in_shape, x, y)
        loss, g = device_step(t, x, y)
        check(f"same k{k}s{s} n={n}", ref, loss, g)
    t.close()


# ---------------------------------------------------------------------------
# warm start without a resampler
# ---------------------------------------------------------------------------
def test_warm_start_100x100_from_a_10_to_100_model(srcfd, enc_weights):
    """A 100x100 lid-driven-cavity batch of two cases primed by FineSolverBatch.init_from_prediction from encoder_10 +
    decoder_100, no resampler: the bits of the host recipe (predict, float64, transposed, init(Var)), then two outer
    iterations that equal the host-primed batch's."""
    require_gpu(srcfd)
    from test_gpu_fine_batch_handoff import _check_against_reference_batch, _host_var, _tiny_inputs
    fine = importlib.import_module("sr-for-cfd_amd.fine")
    coarse = importlib.import_module("sr-for-cfd_amd.coarse")
    model = srcfd.SRModel.from_weights(enc_weights, _family().synthetic_decoder_weights(100, seed=7), device=0)
    assert model.output_shape == (100, 100, 1)
    x, ain, aout = _tiny_inputs((10, 10, 1), 2)
    aout[:, 1] *= 0.05   # O(0.1) initial fields
    pbs = [fine.problem(Re, 100, 100, 1.0, 1.0, 0.001, "QUICK", None, bc) for Re, bc in ((100.0, coarse.LDC_SINGLE_LID), (400.0, coarse.LDC_DOUBLE_LID))]
    b = fine.FineSolverBatch(pbs)
    assert b.init_from_prediction(model, x, ain, aout) == 0
    _check_against_reference_batch(fine, pbs, _host_var(model, x, ain, aout), b, iterations=2)
    b.close()
