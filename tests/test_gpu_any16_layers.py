"""The generic 16-bit layer path (any16: enc16 -> gemm16 / gemm16n per layer -> outconv16) on an MI355X, on the graphs of
tests/any16_cases.py: every branch of those kernels that the five family decoders of test_gpu_model_family.py never take.

  B  integer twins: the device in bf16 and in f16 equals the float64 forward bit for bit (test_any16_cases.py proves on the CPU
     that every intermediate is representable and that a wrong tap, crop, phase or channel quad changes the result);
  C  random weights: per-sample relative L2 against the emulation under the rule of test_encoder10_decoder_x_16bit, the class
     check of tests/error_maps.py on position classes of the case's own output size with the CPU-calibrated margin
     2 x any16_cases.SPREAD, and the path's invariants bit for bit.

The references (float64, one emulation per kind) are computed once per case; a test takes a few seconds.
"""
import os

import numpy as np
import pytest

import any16_cases as ac
import error_maps as em
import family_ref as fr
from conftest import STATS_TXT, require_gpu
from test_gpu_parity_bf16 import MEDIAN_EMU, TOL, per_sample_rel_l2

pytestmark = pytest.mark.gpu
PARAMS = [pytest.param(c, k, id=f"{c}-{k}") for c in ac.CASES for k in ac.KINDS]


@pytest.fixture(scope="module")
def lr_stats(srcfd):
    return srcfd.load_stats(STATS_TXT, 10, 400)[0]


def _model(srcfd, specs, kind):
    m = srcfd.SRModel.from_layers(specs, (10, 10, 1), device=0)
    assert m.supports_precision(kind) and not m.has_fused_path
    m.precision = kind
    return m


def _ran_any16(m, kind, encoder="enc16"):
    plan = m.last_plan()
    assert plan["decoder"] == "any16" and plan["encoder"] == encoder and plan["precision"] == kind, plan


# ------------------------------------------------------------------------------------------------------------------------
# B. exact geometry
# ------------------------------------------------------------------------------------------------------------------------
_TWIN = {}


def _twin(case, seed, enc_weights, x):
    if (case, seed) not in _TWIN:
        specs = ac.build_specs(case, enc_weights, ac.integer_twin(case, seed), all_linear=True)
        _TWIN[(case, seed)] = (specs, fr.forward_specs64(specs, x))
    return _TWIN[(case, seed)]


@pytest.mark.parametrize("case,kind", PARAMS)
def test_integer_twin_equals_float64_bit_for_bit(srcfd, enc_weights, coarse_cases, lr_stats, case, kind):
    """Sparse small-integer weights behind a zero dense_1 kernel: every product, sum and stored activation is an integer of
    magnitude <= 256, so no rounding happens anywhere and the result does not depend on the order of any sum.  n = 1 and n = 3,
    every seed of the twin (together they read every tap and channel of the output convolution).  No tolerance."""
    require_gpu(srcfd)
    x = em.fixed_batch(coarse_cases, lr_stats, 3)
    for seed in ac.TWIN_SEEDS:
        specs, y64 = _twin(case, seed, enc_weights, x)
        m = _model(srcfd, specs, kind)
        for n in (1, 3):
            y = m.predict(x[:n])
            _ran_any16(m, kind)
            assert y.shape == (n,) + ac.out_hw(case) + (1,) and y.dtype == np.float32
            np.testing.assert_array_equal(y.astype(np.float64), y64[:n], err_msg=f"{case} {kind} seed {seed} n = {n}")


# ------------------------------------------------------------------------------------------------------------------------
# C. random weights: error statistics per sample and per position class
# ------------------------------------------------------------------------------------------------------------------------
def _statistics(label, y, ref, kind):
    """Prints, then asserts: the per-sample rule of test_encoder10_decoder_x_16bit and the class check."""
    emu, T = ref[kind], ref["T"]
    e_emu, e_64, emu_64 = per_sample_rel_l2(y, emu), per_sample_rel_l2(y, T), per_sample_rel_l2(emu, T)
    ok, report, _, worst = em.class_check((y - T)[None], (emu - T)[None], ref["classes"][kind], 2 * ac.SPREAD[kind], label)
    print(f"{label}: vs emulation max {e_emu.max():.2e} median {np.median(e_emu):.2e}; vs float64 max {e_64.max():.2e} (emulation vs float64 "
          f"{emu_64.max():.2e}); worst class ratio {worst:.3f} (margin {2 * ac.SPREAD[kind]:.2f})")
    assert e_emu.max() <= TOL[kind][0]
    assert e_64.max() <= emu_64.max() + TOL[kind][0]
    assert np.median(e_emu) <= MEDIAN_EMU[kind]
    assert ok, report


@pytest.mark.parametrize("case,kind", PARAMS)
def test_random_graph_error_statistics(srcfd, enc_weights, coarse_cases, lr_stats, case, kind):
    """The bounds: TOL / MEDIAN_EMU of test_gpu_parity_bf16.py and 2 x any16_cases.SPREAD (CPU-calibrated).  For the record, not the
    source of any bound, an MI355X on 2026-10-19: worst class ratio 1.002 ... 1.040 in bf16, 1.005 ... 1.068 in f16 (per case in
    DESIGN.md section 7); per-sample relative L2 against the emulation at most 6.6e-3 in bf16 and 9.4e-4 in f16, both on wide_1px."""
    require_gpu(srcfd)
    ref = ac.references(case, enc_weights, coarse_cases, lr_stats)
    m = _model(srcfd, ref["specs"], kind)
    y = m.predict(ref["x"])
    _ran_any16(m, kind)
    _statistics(f"{case} {kind} n = {len(y)}", y[..., 0], ref, kind)
    # the layer-by-layer encoder (SRCFD_ENC=0): conv2d_1, dense and latent_vector on gemm16 too, under the same bounds
    os.environ["SRCFD_ENC"] = "0"
    try:
        yl = m.predict(ref["x"])
        _ran_any16(m, kind, encoder="layers")
    finally:
        del os.environ["SRCFD_ENC"]
    _statistics(f"{case} {kind} SRCFD_ENC=0", yl[..., 0], ref, kind)


@pytest.mark.parametrize("case,kind", PARAMS)
def test_random_graph_invariants(srcfd, enc_weights, coarse_cases, lr_stats, case, kind):
    """Bit for bit: a sample's output does not depend on the batch it rides in or on its place in it (first, middle, last of
    130); 16-bit outputs of predict_device are the round-to-nearest-even of the f32 output; out_affine is one fma of the f32
    result; a NaN-poisoned sample is zero-filled and counted as H W values, its neighbours keep their bits."""
    require_gpu(srcfd)
    import torch
    ref = ac.references(case, enc_weights, coarse_cases, lr_stats)
    H, W = ac.out_hw(case)
    m = _model(srcfd, ref["specs"], kind)
    x6 = ref["x"][:6]
    y6 = m.predict(x6)
    _ran_any16(m, kind)
    y1 = m.predict(x6[4:5])
    np.testing.assert_array_equal(y1.view(np.uint32), y6[4:5].view(np.uint32))
    rng = np.random.default_rng(list(ac.CASES).index(case))
    xb = rng.standard_normal((130, 10, 10, 1)).astype(np.float32)
    for at in (0, 64, 129):
        xb[at] = x6[4]
    yb = m.predict(xb)
    assert np.isfinite(yb).all()
    for at in (0, 64, 129):
        np.testing.assert_array_equal(yb[at].view(np.uint32), y1[0].view(np.uint32), err_msg=f"place {at} of 130")
    aout = np.stack([rng.standard_normal(6) * 0.1, rng.uniform(0.05, 0.3, 6)], 1).astype(np.float32)
    ya = m.predict(x6, out_affine=aout)
    want = (y6.astype(np.float64) * aout[:, 1].reshape(-1, 1, 1, 1).astype(np.float64) + aout[:, 0].reshape(-1, 1, 1, 1).astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(ya.view(np.uint32), want.view(np.uint32))
    xp = x6.copy()
    xp[1, 4, 4, 0] = np.nan
    yp, bad = m.predict(xp, nan_guard=True, return_nonfinite=True)
    assert bad == H * W and not yp[1].any()
    np.testing.assert_array_equal(yp[[0, 2, 3, 4, 5]].view(np.uint32), y6[[0, 2, 3, 4, 5]].view(np.uint32))
    xd = torch.from_numpy(x6).cuda()
    y32 = torch.empty((6, H, W, 1), dtype=torch.float32, device="cuda")
    m.predict_device(xd, y32)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y32.cpu().numpy().view(np.uint32), y6.view(np.uint32))
    for dt in (torch.bfloat16, torch.float16):
        y16 = torch.empty((6, H, W, 1), dtype=dt, device="cuda")
        m.predict_device(xd, y16)
        torch.cuda.synchronize()
        assert torch.equal(y16.view(torch.int16).cpu(), y32.to(dt).view(torch.int16).cpu()), dt
    _ran_any16(m, kind)
