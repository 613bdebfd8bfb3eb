"""Per-position error maps of the inference kernels against the float64 oracle (tests/error_maps.py holds the statistic).

Every forward-path parity test reduces a 400x400 field to one relative L2; a defect of one row, one column, one lattice phase,
one corner or one channel is diluted by sqrt(its share of the field) and passes.  Here the device's error field dG = G - T is
reduced per POSITION CLASS (border rows / columns, corners, row / column lattices of 2, 4, 8, strip and segment seams, column
bands, every single row and column; for ConvT#0 / ConvT#1: every channel, channel groups, the four phases) and each class is held
to margin_P times what the CPU emulation of the same arithmetic shows IN THAT CLASS, plus the worst single element likewise.
margin_P = 2 x spread_P comes from two CPU emulations, not from the device (tests/test_error_maps.py, error_maps.SPREAD):
bf16 2.14, f16 2.10, the f32 family 4.0 (single rows / columns pooled in pairs).

A flipped bf16 rounding moves a whole sample, not a class, so it raises every class of that sample alike; classes are pooled over
the N samples, and the per-sample MEDIAN_EMU check stays where it is (test_gpu_parity_bf16.py).

Cost: the references (float64 oracle + emulations of 8 samples on two weight sets) are computed once per module (5 s on the GPU
box's 16 cores).  Wall time on the MI355X box, 2026-10-16: 33 tests in 22 s, next to 18 s for test_gpu_parity_bf16.py.
"""
import importlib
import importlib.util
import math

import numpy as np
import pytest

import error_maps as em
from conftest import STATS_TXT, require_gpu

# The module's own time limit needs the pytest-timeout plugin (named in README.md next to the gpu run); without it the mark would be a silent no-op.
assert importlib.util.find_spec("pytest_timeout"), "tests/test_gpu_error_maps.py needs the pytest-timeout plugin for its time limit"
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]      # per test, references included: a hung kernel ends the test, not the box's day
LOG2E = math.log2(math.e)
BATCHES = (8, 13, 256, 300)


def auto_seg(n, cus):
    """The automatic segmentation of the 16-bit tail: the cost rule of the fused forward (lowp16_plan.cpp, tail_segments) restated.  Cost =
    strips walked by the busiest workgroup; a finer cut has to be 15 % cheaper than the best so far."""
    seg, best = 1, -(-n // cus) * 50 + 2
    for cand in (2, 5, 10, 25):
        cost = -(-n * cand // cus) * (50 // cand + 1) + 2
        if cost * 115 < best * 100:
            best, seg = cost, cand
    return seg


assert [auto_seg(n, 256) for n in BATCHES] == [25, 10, 1, 5]      # a full MI355X: four different segmentations


@pytest.fixture(scope="module")
def batch(srcfd, coarse_cases):
    lr, _ = srcfd.load_stats(STATS_TXT, 10, 400)
    return em.fixed_batch(coarse_cases, lr)


@pytest.fixture(scope="module")
def weight_sets(enc_weights, dec_weights):
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    return {"trained": (enc_weights, dec_weights), "keras-init": synth.keras_default_init(em.KERAS_SEED)}


@pytest.fixture(scope="module")
def refs(batch, weight_sets):
    """{weight set: {"T": (y, acts), "bf16" / "f16" / "f32": (y, acts)}}: shared by every arm; f16 on the trained set only
    (default-initialised weights put this network into f16's denormal range, test_gpu_parity_fp32.py:175)."""
    out = {}
    for name, (enc, dec) in weight_sets.items():
        out[name] = {"T": em.oracle_f64(batch, enc, dec)}
        for kind in (("bf16", "f16", "f32") if name == "trained" else ("bf16", "f32")):
            out[name][kind] = em.emulation(batch, enc, dec, kind)
    return out


def _padded(batch, n):
    """-> (x, rows): the reference samples spread evenly through a batch of n (first and last row included), standard-normal
    samples between them.  The large runs compare only the rows that have a reference; spread out, those rows are first, middle
    and last virtual samples of their workgroups (ids blockIdx + k gridDim, kernels_bf16.hip:404-414), so the entry side of a
    sample seam and the pipeline that does not drain between samples lie under the class table too."""
    if n == len(batch):
        return batch, np.arange(n)
    rows = np.round(np.linspace(0, n - 1, len(batch))).astype(int)
    x = np.random.default_rng(n).standard_normal((n, 10, 10, 1)).astype(np.float32)
    x[rows] = batch
    return x, rows


def _check_output(y, ref, precision, seg, label):
    kind = em.emu_kind(precision)
    T, E = ref["T"][0], ref[kind][0]
    g = np.asarray(y, np.float64)[..., 0]
    assert g.shape == T.shape
    ok, report, _, worst = em.class_check(g - T, E - T, em.output_classes(seg, em.POOL_ROWS[kind]), em.MARGIN[kind], label)
    print(report)
    assert ok, report
    return worst


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("tail", ["tail16", "tail16s"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_output_error_map_16bit(srcfd, enc_weights, dec_weights, batch, refs, kind, tail, n, monkeypatch):
    """Both tail kernels at four batch sizes whose automatic segmentation differs (25 / 10 / 1 / 5 segments per sample on 256
    CUs): the seam classes are built from the segmentation that RAN, and that value is asserted against the cost rule evaluated
    for the CU count the device reports (a partitioned or masked device has fewer; at least three different values must remain)."""
    require_gpu(srcfd)
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert len({auto_seg(b, cus) for b in BATCHES}) >= 3, (cus, [auto_seg(b, cus) for b in BATCHES])
    if tail == "tail16s":
        monkeypatch.setenv("SRCFD_TAIL", "s")
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = kind
    # through the device entry point: the host one stages a large batch in chunks of 128, each with a segmentation of its own
    x, rows = _padded(batch, n)
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty((n, 400, 400, 1), dtype=torch.float32, device="cuda")
    m.predict_device(xd, yd)
    torch.cuda.synchronize()
    y = yd[torch.from_numpy(rows).cuda()].cpu().numpy()
    plan = m.last_plan()
    assert plan["tail"] == tail and plan["tail_seg"] == str(auto_seg(n, cus)), (plan, cus)
    assert plan["encoder"] == "enc16" and plan["middle"] == "mid16_4x64"
    _check_output(y, refs["trained"], kind, int(plan["tail_seg"]), f"{kind} {tail} n={n} seg={plan['tail_seg']}")


@pytest.mark.parametrize("precision", ["fp32", "fp32_naive", "fp32x3"])
def test_output_error_map_f32_family(srcfd, enc_weights, dec_weights, batch, refs, precision):
    """fp32x3 takes a batch of 64 so that its (x3) launches run (asserted from the profile); its reference rows are spread through it."""
    require_gpu(srcfd)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = precision
    if precision == "fp32x3":
        m.set_profiling(True)
        x, rows = _padded(batch, 64)
        y = m.predict(x)[rows]
        names = [nm for nm, _ in m.get_profile()]
        m.set_profiling(False)
        assert sum(nm.endswith("(x3)") for nm in names) == 3, names
    else:
        y = m.predict(batch)
    _check_output(y, refs["trained"], precision, 1, precision)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_output_error_map_on_default_initialised_weights(srcfd, weight_sets, batch, refs, precision):
    """A weight set that is not the trained one (fragment packing errors that happen to be small on the trained encoder)."""
    require_gpu(srcfd)
    m = srcfd.SRModel.from_weights(*weight_sets["keras-init"], device=0)
    m.precision = precision
    y = m.predict(batch)
    seg = int(m.last_plan()["tail_seg"]) if precision == "bf16" else 1
    _check_output(y, refs["keras-init"], precision, seg, f"keras-init {precision}")


@pytest.mark.parametrize("mid", ["3", "2", "1", "0"], ids=["fused_mid_4x64", "fused_mid_8x64", "fused_mid_8x32", "generic_gemm"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_activation_error_maps(srcfd, enc_weights, dec_weights, batch, refs, kind, mid, monkeypatch):
    """ConvT#1's output (50x50x64) from every implementation of the middle, and ConvT#0's (25x25x128) from the generic GEMMs: per
    channel, channel group, border, phase, row and column against decoder_forward(float64), the emulation's activations as the
    yardstick.  The device stores log2(e) x activation."""
    require_gpu(srcfd)
    from oracle import sr_oracle_lowp as lp
    monkeypatch.setenv("SRCFD_MID", mid)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = kind
    m.predict(batch)
    assert m.last_plan()["middle"] == {"3": "mid16_4x64", "2": "mid16_8x64", "1": "mid16_8x32", "0": "gemm16"}[mid]
    conv = lp.bf16_bits_to_f32 if kind == "bf16" else (lambda b: b.view(np.float16).astype(np.float32))
    n = len(batch)
    Ta, Ea = refs["trained"]["T"][1], refs["trained"][kind][1]
    for index, name, shape in ((0, "t1", (50, 50, 64)), (1, "t0", (25, 25, 128))):
        if name == "t0" and mid != "0":
            continue
        g = conv(m.debug_activation(index, (n,) + shape)).astype(np.float64) / LOG2E
        ok, report, _, _ = em.class_check(g - Ta[name], Ea[name] - Ta[name], em.activation_classes(*shape), em.MARGIN[kind], f"{kind} mid={mid} {name}")
        print(report)
        assert ok, report


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "out_affine"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_16bit_outputs_are_the_f32_outputs_rounded_to_nearest_even(srcfd, enc_weights, dec_weights, batch, kind, affine):
    """bf16 / f16 `y` tensors through predict_device: every element equals the float32 output of the same call on the same handle
    rounded to nearest-even, bit for bit (the kernel packs the float32 value it would have stored), with and without out_affine,
    and with the NaN guard on a poisoned sample (zeros, count 160000).  Until now the 16-bit formats were compared only between
    the two tail kernels."""
    require_gpu(srcfd)
    import torch
    from oracle import sr_oracle_lowp as lp
    x = batch.copy()
    x[5, 2, 2, 0] = np.nan
    n = len(x)
    xd = torch.from_numpy(x).cuda()
    rng = np.random.default_rng(31)
    aout = torch.from_numpy(np.stack([rng.standard_normal(n) * 0.1, rng.uniform(0.05, 0.3, n)], 1).astype(np.float32)).cuda() if affine else None
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = kind
    outs = {}
    for odt in (torch.float32, torch.bfloat16, torch.float16):
        y = torch.empty((n, 400, 400, 1), dtype=odt, device="cuda")
        bad = torch.zeros(1, dtype=torch.int64, device="cuda")
        m.predict_device(xd, y, out_affine=aout, nan_guard=True, nonfinite=bad)
        torch.cuda.synchronize()
        assert int(bad.item()) == 160000
        outs[odt] = y.cpu()
    y32 = outs[torch.float32].numpy()
    assert np.all(y32[5] == 0) and np.isfinite(y32).all() and np.abs(y32[0]).max() > 0
    want_bf16 = (lp.round_bf16(y32).view(np.uint32) >> 16).astype(np.uint16)
    got_bf16 = outs[torch.bfloat16].view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got_bf16, want_bf16), f"bf16 output: {np.mean(got_bf16 != want_bf16):.3e} of the elements differ"
    want_f16 = y32.astype(np.float16).view(np.uint16)
    got_f16 = outs[torch.float16].view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got_f16, want_f16), f"f16 output: {np.mean(got_f16 != want_f16):.3e} of the elements differ"
