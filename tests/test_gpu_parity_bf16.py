"""GPU parity of the 16-bit throughput path (bf16 / f16 operands, f32 accumulate).

Stated tolerances (relative L2 per sample, max over the set, on the
standardised output):
  * against the 16-bit CPU emulation (oracle/sr_oracle_lowp.py): the kernels
    must be *right* -- only accumulation order and hardware exp/rcp differ;
  * against the float64 oracle: the accuracy price of 16-bit operands.  The
    north-star figure of 1e-5 applies to the f32 path (test_gpu_parity_fp32.py);
    bf16 carries 8 mantissa bits and cannot meet it (SURVEY.md 7 'hard parts').
"""
import math

import numpy as np
import pytest

from conftest import STATS_TXT, require_gpu

pytestmark = pytest.mark.gpu
LOG2E = math.log2(math.e)

# (vs emulation, vs float64 oracle): bounds on the MAXIMUM over the samples.  Measured on MI355X: f16 6.1e-4 / 9.0e-4,
# bf16 5.5e-3 / 7.5e-3.  bf16-vs-emulation is not tighter than bf16-vs-f64 because a last-bit difference in an f32 sum
# flips bf16 roundings (2^-8 relative each) that then propagate.
# The f16-vs-emulation row is the logic check, and it is stated per sample: the TYPICAL sample sits at 0.8-1.9e-4 from the
# emulation (MEDIAN_EMU: the median over the samples must stay below 3e-4), and the maximum is set by ONE flipped f16
# rounding of one of the 50 latent components, which moves that sample to ~6e-4 (profiles/r03/a_enc_ab_f16_flipped_rounding.txt,
# written by tools/enc_ab.py: the one-launch encoder and the layer-by-layer chain each have one such sample -- a different
# one -- and agree with the emulation everywhere else).  A wrong kernel moves every sample, i.e. the median.
TOL = {
    "bf16": (1e-2, 2e-2),
    "f16": (1.2e-3, 3e-3),
}
MEDIAN_EMU = {"bf16": 8e-3, "f16": 3e-4}


def per_sample_rel_l2(y, ref):
    y = np.asarray(y, np.float64).reshape(y.shape[0], -1)
    ref = np.asarray(ref, np.float64).reshape(ref.shape[0], -1)
    return np.linalg.norm(y - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)


def _coarse_batch(coarse_cases, srcfd):
    lr, _ = srcfd.load_stats(STATS_TXT, 10, 400)
    xs = []
    for case in coarse_cases.values():
        for c in ("u", "v", "p"):
            x = case[c].astype(np.float32)
            xs.append(((x - lr[c][0]) / lr[c][1]).astype(np.float32))
    return np.stack(xs)[..., None]


@pytest.fixture(scope="module")
def refs(srcfd, oracle, enc_weights, dec_weights, coarse_cases):
    from oracle import sr_oracle_lowp as lp
    x = _coarse_batch(coarse_cases, srcfd)[:6]
    out = {"x": x, "f64": oracle.superres_forward(x, enc_weights, dec_weights, np.float64)}
    for kind in ("bf16", "f16"):
        out[kind] = lp.superres_forward_lowp(x, enc_weights, dec_weights, kind, return_all=True)
    return out


@pytest.mark.parametrize("mid", ["3", "2", "1", "0"], ids=["fused_mid_4x64", "fused_mid_8x64", "fused_mid_8x32", "generic_gemm"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_intermediate_activations(srcfd, oracle, enc_weights, dec_weights, refs, kind, mid, monkeypatch):
    """ConvT#1 output (50x50x64) before the fused tail, from both implementations of the middle
    of the network: the fused ConvT#0->ConvT#1 kernel in its three workgroup shapes (SRCFD_MID=3, the default: 4 waves x 64 pixels;
    2: 8 x 64; 1: 8 x 32) and the generic 16-bit implicit GEMMs (SRCFD_MID=0), which also expose ConvT#0's output (25x25x128)."""
    require_gpu(srcfd)
    from oracle import sr_oracle_lowp as lp
    monkeypatch.setenv("SRCFD_MID", mid)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = kind
    x = refs["x"]
    y = m.predict(x)
    assert m.last_plan()["middle"] == {"3": "mid16_4x64", "2": "mid16_8x64", "1": "mid16_8x32", "0": "gemm16"}[mid]
    _, acts = refs[kind]
    n = x.shape[0]
    conv = lp.bf16_bits_to_f32 if kind == "bf16" else (lambda b: b.view(np.float16).astype(np.float32))
    e1 = oracle.rel_l2(conv(m.debug_activation(0, (n, 50, 50, 64))) / LOG2E, acts["t1"])
    print(f"{kind} mid={mid}: ConvT#1 rel L2 {e1:.2e}")
    assert e1 <= TOL[kind][0]
    if mid == "0":
        e0 = oracle.rel_l2(conv(m.debug_activation(1, (n, 25, 25, 128))) / LOG2E, acts["t0"])
        print(f"{kind}: ConvT#0 rel L2 {e0:.2e}")
        assert e0 <= TOL[kind][0]
    assert oracle.rel_l2(y, refs["f64"]) <= TOL[kind][1]


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_full_model(srcfd, oracle, enc_weights, dec_weights, refs, kind):
    require_gpu(srcfd)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = kind
    y = m.predict(refs["x"])
    e_emu = oracle.rel_l2(y, refs[kind][0])
    e_f64 = oracle.rel_l2(y, refs["f64"])
    print(f"{kind}: rel L2 vs 16-bit emulation {e_emu:.2e}, vs f64 oracle {e_f64:.2e}")
    assert y.shape == (6, 400, 400, 1) and np.isfinite(y).all()
    assert e_emu <= TOL[kind][0]
    assert e_f64 <= TOL[kind][1]
    per = per_sample_rel_l2(y, refs[kind][0])
    print(f"{kind}: per-sample rel L2 vs emulation {np.array2string(per, precision=2)}; median {np.median(per):.2e}")
    assert np.median(per) <= MEDIAN_EMU[kind]
    assert m.last_plan()["encoder"] == "enc16" and m.last_plan()["middle"] == "mid16_4x64"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_the_workgroup_shapes_of_the_fused_middle_agree_bit_for_bit(srcfd, enc_weights, dec_weights, kind, monkeypatch):
    """mid16 with 4 waves x 64 pixels (default), 8 x 64 (three weight tiles in flight) and 8 x 32 per workgroup run the same
    products in the same order per output: identical bits, for batches whose last workgroup of a phase is full, partial or alone."""
    require_gpu(srcfd)
    rng = np.random.default_rng(11)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = kind
    for n in (1, 3, 7, 50, 303):
        x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
        outs = {}
        monkeypatch.delenv("SRCFD_MID_ORDER", raising=False)
        monkeypatch.delenv("SRCFD_MID_WAVES", raising=False)
        for mid in ("1", "2", "3"):
            monkeypatch.setenv("SRCFD_MID", mid)
            outs[mid] = m.predict(x).copy()
            assert m.last_plan()["middle"] == {"1": "mid16_8x32", "2": "mid16_8x64", "3": "mid16_4x64"}[mid]
            if n <= 50:   # (the hook sees the workspace of the last chunk of a large batch only)
                outs[mid + "a"] = m.debug_activation(0, (n, 50, 50, 64)).copy()
        if n <= 50:
            assert np.array_equal(outs["1a"], outs["2a"]) and np.array_equal(outs["1a"], outs["3a"]), f"n={n}: ConvT#1 activations differ"
        assert np.array_equal(outs["1"], outs["2"]) and np.array_equal(outs["1"], outs["3"]), f"n={n}"
        # the remaining diagnostic shapes / orders of the same kernel: 4 and 16 waves at 32 pixels per wave, phases dispatched alternately
        monkeypatch.setenv("SRCFD_MID_ORDER", "1")
        assert np.array_equal(m.predict(x), outs["1"]), f"n={n}: SRCFD_MID_ORDER=1"
        monkeypatch.delenv("SRCFD_MID_ORDER")
        for w, name in (("4", "mid16_4x32"), ("16", "mid16_16x32")):
            monkeypatch.setenv("SRCFD_MID_WAVES", w)
            assert np.array_equal(m.predict(x), outs["1"]), f"n={n}: SRCFD_MID_WAVES={w}"
            assert m.last_plan()["middle"] == name
        monkeypatch.delenv("SRCFD_MID_WAVES")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_one_launch_encoder_against_the_layer_by_layer_chain(srcfd, oracle, enc_weights, dec_weights, refs, kind, monkeypatch):
    """enc16 (conv2d -> conv2d_1 -> dense -> latent_vector in one kernel, 5 samples per workgroup) and the four-launch chain
    it replaces (SRCFD_ENC=0) are two complete implementations of rows a7-a10: both within the 16-bit tolerance of the
    emulation, close to each other, and enc16's rows do not depend on the batch they sit in (partial last workgroups:
    n = 1, 6, 7, 11) or, with standardisation fused in, on where the affine is applied."""
    require_gpu(srcfd)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = kind
    x = refs["x"]
    # the switches are part of the hipGraph key (three identical calls on one handle would otherwise replay the capture of
    # the second): every arm asserts the implementation that RAN (srcfd_model_last_plan)
    y_enc = m.predict(x)
    assert m.last_plan()["encoder"] == "enc16" and m.last_plan()["dense_1"] == "dense1_16"
    monkeypatch.setenv("SRCFD_ENC", "0")
    y_chain = m.predict(x)
    assert m.last_plan()["encoder"] == "layers" and m.last_plan()["dense_1"] == "dense1_16"
    y_chain2 = m.predict(x)                        # second identical call: captured
    y_chain3 = m.predict(x)                        # third: replayed -- still the layer-by-layer chain
    assert m.last_plan()["encoder"] == "layers" and m.last_plan()["graph"] == "replay"
    np.testing.assert_array_equal(y_chain2, y_chain)
    np.testing.assert_array_equal(y_chain3, y_chain)
    monkeypatch.delenv("SRCFD_ENC")
    monkeypatch.setenv("SRCFD_DENSE1", "0")        # dense_1 (64 -> 36 864) on the generic implicit GEMM instead of dense1_16
    y_gemm_d1 = m.predict(x)
    assert m.last_plan()["encoder"] == "enc16" and m.last_plan()["dense_1"] == "gemm16" and m.last_plan()["graph"] == "eager"
    monkeypatch.delenv("SRCFD_DENSE1")
    np.testing.assert_array_equal(m.predict(x), y_enc)   # back on the defaults: not the replay of an A/B arm
    assert m.last_plan()["encoder"] == "enc16" and m.last_plan()["dense_1"] == "dense1_16"
    for y in (y_enc, y_chain, y_gemm_d1):
        assert oracle.rel_l2(y, refs[kind][0]) <= TOL[kind][0]
        assert oracle.rel_l2(y, refs["f64"]) <= TOL[kind][1]
        assert np.median(per_sample_rel_l2(y, refs[kind][0])) <= MEDIAN_EMU[kind]
    assert oracle.rel_l2(y_enc, y_chain) <= TOL[kind][0]
    assert oracle.rel_l2(y_enc, y_gemm_d1) <= TOL[kind][0]
    rng = np.random.default_rng(5)
    xs = rng.standard_normal((11, 10, 10, 1)).astype(np.float32)
    y11 = m.predict(xs)
    for lo, hi in ((0, 1), (4, 10), (3, 10), (10, 11)):
        np.testing.assert_array_equal(m.predict(xs[lo:hi]), y11[lo:hi])
    ain = np.stack([rng.standard_normal(11) * 0.1, rng.uniform(0.5, 2.0, 11)], 1).astype(np.float32)
    xn = ((xs - ain[:, 0].reshape(11, 1, 1, 1)) / ain[:, 1].reshape(11, 1, 1, 1)).astype(np.float32)
    np.testing.assert_array_equal(m.predict(xs, in_affine=ain), m.predict(xn))


def test_bf16_batch_larger_than_cu_count_and_affine(srcfd, oracle, enc_weights, dec_weights):
    """300 samples > 256 workgroups: a workgroup walks more than one sample; results
    must not depend on the batch a sample sits in, and the fused de-standardise /
    NaN guard epilogue must match the f32 formula applied to the raw output."""
    require_gpu(srcfd)
    rng = np.random.default_rng(21)
    n = 300
    x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = "bf16"
    y = m.predict(x)
    y_small = m.predict(x[257:260])
    np.testing.assert_array_equal(y[257:260], y_small)
    aout = np.stack([rng.standard_normal(n) * 0.1, rng.uniform(0.05, 0.3, n)], 1).astype(np.float32)
    ya, bad = m.predict(x, out_affine=aout, nan_guard=True, return_nonfinite=True)
    assert bad == 0
    # the 16-bit path de-standardises with ONE fma per value (round 3; the f32 parity path keeps numpy's two roundings bit for bit,
    # test_gpu_parity_fp32.py): within 1 ulp of y * std + mean evaluated in float32, and exactly the float64 expression rounded once
    prod = y * aout[:, 1].reshape(n, 1, 1, 1)
    ref = (prod + aout[:, 0].reshape(n, 1, 1, 1)).astype(np.float32)
    assert np.all(np.abs(ya - ref) <= 2.0 ** -23 * (np.abs(prod) + np.abs(ref)))   # the product's rounding, which the fma does not make
    ref_fma = (y.astype(np.float64) * aout[:, 1].astype(np.float64).reshape(n, 1, 1, 1) + aout[:, 0].astype(np.float64).reshape(n, 1, 1, 1)).astype(np.float32)
    np.testing.assert_array_equal(ya, ref_fma)
    # spot-check a few samples against the float64 oracle
    idx = [0, 255, 256, 299]
    assert oracle.rel_l2(y[idx], oracle.superres_forward(x[idx], enc_weights, dec_weights, np.float64)) <= TOL["bf16"][1]


def test_bf16_in_affine_and_nan_guard(srcfd, enc_weights, dec_weights):
    require_gpu(srcfd)
    rng = np.random.default_rng(22)
    x = rng.standard_normal((4, 10, 10, 1)).astype(np.float32) * 0.2
    ain = np.array([[0.1, 0.2], [0.0, 0.0], [-0.1, 0.3], [0.05, 0.25]], np.float32)  # sample 1: std==0 -> 1e-8
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = "bf16"
    sd = np.where(ain[:, 1] == 0, np.float32(1e-8), ain[:, 1]).reshape(4, 1, 1, 1)
    xn = ((x - ain[:, 0].reshape(4, 1, 1, 1)) / sd).astype(np.float32)
    keep = [0, 2, 3]
    y_fused = m.predict(x, in_affine=ain)
    y_pre = m.predict(xn)
    np.testing.assert_array_equal(y_fused[keep], y_pre[keep])
    xb = x.copy()
    xb[2, 3, 3, 0] = np.nan  # NaN input poisons the whole field through the dense layers
    yb, bad = m.predict(xb, nan_guard=True, return_nonfinite=True)
    assert bad == 160000 and np.all(yb[2] == 0) and np.isfinite(yb).all()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_full_size_batch256_properties(srcfd, oracle, enc_weights, dec_weights, precision):
    """BASELINE config 2 at its full size (256 fields = 768 samples) through the device entry point the bench uses.
    The oracle needs ~1 s per sample, so the whole batch is checked through size-independent properties: samples are
    independent (any permutation of the batch permutes the outputs bit for bit; a sub-batch reproduces its rows),
    a duplicated input gives a duplicated output, and a handful of rows are compared with the float64 oracle."""
    require_gpu(srcfd)
    import torch
    rng = np.random.default_rng(256)
    n = 768
    x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
    x[700] = x[3]  # duplicate
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = precision
    xd = torch.from_numpy(x).cuda()
    y = torch.empty((n, 400, 400, 1), dtype=torch.float32, device="cuda")
    m.predict_device(xd, y)
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    yp = torch.empty_like(y)
    m.predict_device(xd[perm].contiguous(), yp)
    torch.cuda.synchronize()
    assert torch.equal(yp, y[perm])
    assert torch.equal(y[700], y[3])
    ys = torch.empty((5, 400, 400, 1), dtype=torch.float32, device="cuda")
    m.predict_device(xd[381:386].contiguous(), ys)
    torch.cuda.synchronize()
    assert torch.equal(ys, y[381:386])
    idx = [0, 255, 511, 767]
    tol = TOL["bf16"][1] if precision == "bf16" else 1e-5
    assert oracle.rel_l2(y[idx].cpu().numpy(), oracle.superres_forward(x[idx], enc_weights, dec_weights, np.float64)) <= tol
    assert bool(torch.isfinite(y).all())


def test_handles_release_their_device_memory(srcfd, enc_weights, dec_weights):
    """Create / use / destroy models, trainers, resamplers and fine-mesh batches repeatedly, reaching every owner of device
    memory, streams, events and graph executables in them: free device memory must come back (every hipMalloc of a handle is
    released by its destroy call).  The trainer is closed with its captured two-stream step graph just replayed and no device-wide
    wait in between: destroyed like that, a trainer that only waited for its own streams lost 56 MiB per cycle."""
    require_gpu(srcfd)
    import gc
    import importlib
    import torch
    from test_dropin import page_locked
    tr = importlib.import_module("sr-for-cfd_amd.train")
    rs = importlib.import_module("sr-for-cfd_amd.resample")
    fine = importlib.import_module("sr-for-cfd_amd.fine")
    x = np.random.default_rng(1).standard_normal((4, 10, 10, 1)).astype(np.float32)

    def cycle():
        m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
        for prec in ("fp32", "fp32x3", "bf16", "f16"):
            m.precision = prec
            m.predict(x)
        y_locked, free_locked = page_locked((4, 400, 400, 1))   # the copy stream, its four events, the second result buffer
        m.predict(x, out=y_locked)
        del y_locked
        free_locked()
        xd, yd = torch.from_numpy(x[:3]).cuda(), torch.empty((3, 400, 400, 1), device="cuda")
        for _ in range(3):                                      # the second call captures a graph, the third replays it
            m.predict_device(xd, yd)
        assert m.last_plan()["graph"] == "replay"
        m.predict_into_solver_state(x[:3], np.zeros((3, 4), np.int32), np.zeros((3, 4)))
        t = tr.Trainer(m, max_batch=2)
        xt, yt = torch.from_numpy(x[:2]).cuda(), torch.zeros((2, 400, 400, 1), device="cuda")
        for _ in range(2):                                      # the second identical step is captured
            t.step(xt, yt)
        r = rs.Resampler(np.eye(400), np.eye(400), 0)
        m.predict_resampled(x[:3], r)
        b = fine.FineSolverBatch([fine.problem(100.0, 12, 10), fine.problem(200.0, 12, 10)])
        b.run(2)
        t.close(); r.close(); b.close(); m.close()
        del t, r, b, m
        gc.collect()

    cycle()  # first cycle: one-time allocations of the runtime itself
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(5):
        cycle()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 << 20, f"leaked {(free0 - free1) / 2**20:.1f} MiB over 5 create/destroy cycles"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_tail_segmentation_is_bit_identical(srcfd, enc_weights, dec_weights, kind, monkeypatch):
    """Small batches cut every sample into 2 / 5 / 10 / 25 segments of strips handled by different workgroups (each with
    one warm-up strip); the arithmetic per pixel is unchanged, so every segmentation must reproduce the unsegmented
    result bit for bit -- including the de-standardise epilogue, sample seams and more virtual samples than CUs."""
    require_gpu(srcfd)
    rng = np.random.default_rng(77)
    n = 13
    x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
    aout = np.stack([rng.standard_normal(n) * 0.1, rng.uniform(0.05, 0.3, n)], 1).astype(np.float32)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = kind
    monkeypatch.setenv("SRCFD_TAIL_SEG", "1")
    ref = m.predict(x, out_affine=aout, nan_guard=True)
    assert m.last_plan()["tail_seg"] == "1"
    for seg in ("2", "5", "10", "25"):   # 13 x 25 = 325 virtual samples > 256 workgroups
        monkeypatch.setenv("SRCFD_TAIL_SEG", seg)   # read on every call (round 2 read it once per process: the loop compared one segmentation with itself)
        y = m.predict(x, out_affine=aout, nan_guard=True)
        assert m.last_plan()["tail_seg"] == seg, m.last_plan()   # the segmentation that RAN
        np.testing.assert_array_equal(y, ref, err_msg=f"segments={seg}")
    monkeypatch.delenv("SRCFD_TAIL_SEG")
    np.testing.assert_array_equal(m.predict(x, out_affine=aout, nan_guard=True), ref)
    assert m.last_plan()["tail_seg"] == "10"    # the automatic choice for 13 samples on 256 CUs


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_the_two_tail_kernels_agree_bit_for_bit(srcfd, enc_weights, dec_weights, kind, monkeypatch):
    """tail16 (16 waves, stage by stage: the shipped kernel) and tail16s (SRCFD_TAIL=s: 8 waves of 256 registers, every MFMA inside
    the swish stream of its wave, D epilogues deferred across the barrier, a different static schedule and work split) are two
    complete implementations of rows a15-a20 with the same arithmetic per output: every batch size / segmentation / seam case must
    agree bit for bit, outputs in all three formats."""
    require_gpu(srcfd)
    import torch
    rng = np.random.default_rng(303)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = kind
    for n in (1, 3, 13, 130, 300):
        x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
        aout = np.stack([rng.standard_normal(n) * 0.1, rng.uniform(0.05, 0.3, n)], 1).astype(np.float32)
        segs = ("1", "2", "5", "10", "25") if n == 13 else (None,)
        for seg in segs:
            if seg is None:
                monkeypatch.delenv("SRCFD_TAIL_SEG", raising=False)
            else:
                monkeypatch.setenv("SRCFD_TAIL_SEG", seg)
            monkeypatch.setenv("SRCFD_TAIL", "s")
            y_new, bad_new = m.predict(x, out_affine=aout, nan_guard=True, return_nonfinite=True)
            assert m.last_plan()["tail"] == "tail16s"
            monkeypatch.delenv("SRCFD_TAIL", raising=False)
            y_old, bad_old = m.predict(x, out_affine=aout, nan_guard=True, return_nonfinite=True)
            assert m.last_plan()["tail"] == "tail16"
            np.testing.assert_array_equal(y_new, y_old, err_msg=f"n={n} seg={seg}")
            assert bad_new == bad_old == 0
    monkeypatch.delenv("SRCFD_TAIL_SEG", raising=False)
    # 16-bit outputs and the NaN guard (a poisoned sample is zero-filled and counted by both)
    n = 7
    x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
    x[4, 2, 2, 0] = np.nan
    xd = torch.from_numpy(x).cuda()
    for odt in (torch.float32, torch.bfloat16, torch.float16):
        outs = []
        for tail in (None, "s"):
            if tail is None:
                monkeypatch.delenv("SRCFD_TAIL", raising=False)
            else:
                monkeypatch.setenv("SRCFD_TAIL", tail)
            y = torch.empty((n, 400, 400, 1), dtype=odt, device="cuda")
            bad = torch.zeros(1, dtype=torch.int64, device="cuda")
            m.predict_device(xd, y, nan_guard=True, nonfinite=bad)
            torch.cuda.synchronize()
            assert int(bad.item()) == 160000
            outs.append(y.cpu())
        assert torch.equal(outs[0].view(torch.int16 if odt != torch.float32 else torch.int32), outs[1].view(torch.int16 if odt != torch.float32 else torch.int32))
    monkeypatch.delenv("SRCFD_TAIL", raising=False)
