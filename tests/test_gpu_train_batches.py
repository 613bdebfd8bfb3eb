"""The SR network's training step at batches 9 .. 32 (and 7) on a max_batch = 32 handle -- the one bench.py times -- against float64
autograd, under the unchanged `check` of tests/test_gpu_training_oracle.py (ratio 8, ceiling 2e-4, bias floor 2^-24 cond).  The
batches and what they reach: tests/train_batches.py, proved in tests/test_train_batches.py.  Every path is asserted through
Trainer.plan and Trainer.last_step() (srcfd_trainer_last_step: the segment count of tail32<TRAIN>, its workgroups, the workgroups of
tail_bwd32, and whether the step ran as plain launches, was captured, or replayed), against the rules restated in
tests/train_plan_ref.py for the device's CU count.

(a) every batch x SRCFD_TRAIN_TAIL x SRCFD_TRAIN_ENC against float64: a fresh handle's first, plain call;
(b) the benchmark's call form: 32 samples as an overwriting call of 16 and a same-params accumulating call of 16, and as one
    overwriting call over NaN-filled buffers;
(c) the recorded bits of tests/golden/train_step_digests.json (max_batch = 8) on max_batch = 13 and 32;
(d) one handle through twelve (n, flags) keys, large and small batches in turn, each key three times: the first eight are captured
    and replayed, the rest stay plain launches, and every call gives the bits of (a)'s fresh handle;
(e) Adam over steps of 32, 32, 29, 32 samples (the helper of test_gpu_training_oracle.py, the same rules)."""
import importlib
import json
import os
import time

import numpy as np
import pytest

import train_batches as tb
from conftest import require_gpu
from train_plan_ref import tail32_blocks, tail32_segments, tail_bwd32_blocks

pytestmark = pytest.mark.gpu

MAX_BATCH = 32
ARMS = [(1, 1), (1, 0), (0, 1), (0, 0)]   # (SRCFD_TRAIN_TAIL, SRCFD_TRAIN_ENC)


def _orc():
    return importlib.import_module("test_gpu_training_oracle")


def _bits():
    return importlib.import_module("test_gpu_train_step_bits")


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def make_trainer(srcfd, specs, tail, enc, max_batch=MAX_BATCH):
    """A fresh handle with the two switches set while it is created (the trainer reads them then)."""
    env = {"SRCFD_TRAIN_TAIL": str(tail), "SRCFD_TRAIN_ENC": str(enc)}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        t = _orc()._tr().Trainer(srcfd.SRModel.from_layers(specs, (10, 10, 1), device=0), max_batch=max_batch)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert t.plan == {"fused_tail": tail, "fused_encoder": enc}
    assert t.n_params == 2_709_491
    return t


def want_step(n, tail, launch):
    """what Trainer.last_step() must say after a step of n samples on this device"""
    cus = _cus()
    seg = tail32_segments(n, tb.TAIL_H, cus)
    return {"n": n, "tail_seg": seg if tail else 0, "tail_blocks": tail32_blocks(n, seg, cus) if tail else 0,
            "bwd_blocks": tail_bwd32_blocks(n, tb.TAIL_H, tb.TAIL_W, cus) if tail else 0, "launch": launch}


_DEV = {}


def device_batch(x, y, n):
    """the batch of sr_case(n) on the device, uploaded once"""
    import torch
    if n not in _DEV:
        _DEV[n] = (torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    return _DEV[n]


def call(t, xd, yd, overwrite=False, same_params=False, global_batch=None, prefill=True):
    """One forward_backward; grads and sse are NaN-filled in front of an overwriting call and zeroed in front of an accumulating one
    (prefill=False: left as they are, to accumulate further).  -> (float32 gradient, float64 sse array), copies on the host."""
    import torch
    if prefill:
        if overwrite:
            t.grads.fill_(float("nan"))
            t.sse.fill_(float("nan"))
        else:
            t.grads.zero_()
            t.sse.zero_()
    t.forward_backward(xd, yd, global_batch=global_batch, overwrite=overwrite, same_params=same_params)
    torch.cuda.synchronize()
    return t.grads.cpu().numpy(), t.sse.cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


_FIRST = {}


def first_plain(srcfd, enc_weights, dec_weights, n, tail, enc):
    """(gradient, sse) of a fresh max_batch = 32 handle's first call at n samples -- plain launches, accumulating over zeroed
    buffers -- held to float64 under `check` and to the restated launch sizes; once per (n, switches)."""
    key = (n, tail, enc)
    if key not in _FIRST:
        specs, x, y, ref = tb.sr_case(srcfd, enc_weights, dec_weights, n)
        xd, yd = device_batch(x, y, n)
        t0 = time.perf_counter()
        t = make_trainer(srcfd, specs, tail, enc)
        t1 = time.perf_counter()
        try:
            assert t.last_step() == {"n": 0, "tail_seg": 0, "tail_blocks": 0, "bwd_blocks": 0, "launch": 0}
            g, sse = call(t, xd, yd)
            assert t.last_step() == want_step(n, tail, 0), (n, tail, enc, t.last_step())
        finally:
            t.close()
        print(f"[n={n} tail={tail} enc={enc}] handle {1e3 * (t1 - t0):.0f} ms, first step {1e3 * (time.perf_counter() - t1):.0f} ms")
        _orc().check(f"sr max_batch={MAX_BATCH} n={n} tail={tail} enc={enc}", ref, float(sse[0]) / (n * 160000), g)
        _FIRST[key] = (g, sse)
    return _FIRST[key]


# ---------------------------------------------------------------------------
# (a) against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", tb.RUN)
def test_every_batch_and_path_matches_oracle(srcfd, enc_weights, dec_weights, n):
    require_gpu(srcfd)
    if _cus() != tb.CUS:
        print(f"{_cus()} CUs: the reach proof of tests/test_train_batches.py was made for {tb.CUS}; same bounds")
    _, _, _, ref = tb.sr_case(srcfd, enc_weights, dec_weights, n)   # float64 and float32 once, shared by the four arms
    assert ref.sizes == [(k, {**enc_weights, **dec_weights}[k].size) for k in _orc()._ag().flat_order(enc_weights, dec_weights)]
    for tail, enc in ARMS:
        first_plain(srcfd, enc_weights, dec_weights, n, tail, enc)


# ---------------------------------------------------------------------------
# (b) the benchmark's call form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tail,enc", ARMS)
def test_the_benchmarks_call_form_at_32(srcfd, enc_weights, dec_weights, tail, enc):
    """bench.py: Trainer(max_batch=32), one overwriting call, then same_params accumulating calls, the loss scaled by the global
    batch.  Two calls of 16 make the 32-sample gradient; one overwriting call of 32 over NaN gives the accumulating call's bits."""
    require_gpu(srcfd)
    specs, x, y, ref = tb.sr_case(srcfd, enc_weights, dec_weights, 32)
    xd, yd = device_batch(x, y, 32)
    t = make_trainer(srcfd, specs, tail, enc)
    try:
        call(t, xd[:16], yd[:16], overwrite=True, global_batch=32)
        assert t.last_step() == want_step(16, tail, 0)
        g, sse = call(t, xd[16:], yd[16:], same_params=True, global_batch=32, prefill=False)
        assert t.last_step() == want_step(16, tail, 0)   # another key (flags): its first call
        _orc().check(f"sr 16 + 16 of global batch 32 tail={tail} enc={enc}", ref, float(sse[0]) / (32 * 160000), g)
        g1, sse1 = call(t, xd, yd, overwrite=True)
        assert t.last_step() == want_step(32, tail, 0)
    finally:
        t.close()
    g0, sse0 = first_plain(srcfd, enc_weights, dec_weights, 32, tail, enc)
    assert same_bits(sse1, sse0) and same_bits(g1, g0), "overwriting over NaN differs from accumulating over zeros"


# ---------------------------------------------------------------------------
# (c) bits do not depend on max_batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_batch", [13, 32])
@pytest.mark.parametrize("n", [1, 5, 8])
def test_recorded_bits_do_not_depend_on_max_batch(srcfd, enc_weights, dec_weights, n, max_batch):
    """max_batch sizes buffers (slab space, the encoder partials' pitch, the split-K workspace) and nothing else: the plain,
    captured, replayed and overwriting calls of a larger handle give the digests recorded on max_batch = 8."""
    require_gpu(srcfd)
    bits = _bits()
    doc = json.load(open(bits.GOLDEN_JSON))
    golden = doc["cases"][bits.case_id(("sr", 8, n, {}))]
    inputs, got = bits.run_case(srcfd, enc_weights, dec_weights, ("sr", max_batch, n, {}))
    assert inputs == golden["input_sha256"]
    for name, (grads, sse) in zip(bits.CALLS, got):
        assert grads == golden["grads_sha256"], f"max_batch={max_batch} n={n} {name}: gradient bits differ from the max_batch=8 record"
        assert sse == golden["sse_bits"], f"max_batch={max_batch} n={n} {name}: sse bits differ from the max_batch=8 record"


# ---------------------------------------------------------------------------
# (d) one handle, many batch sizes
# ---------------------------------------------------------------------------
O, S = "overwrite", "same_params"
# (n, flags), large and small in turn; the first eight get the handle's eight graph slots, the last four never do
KEYS = [(32, {O}), (9, {O}), (32, set()), (13, {S}), (26, {O, S}), (9, set()), (20, {O}), (12, set()),
        (17, {O}), (16, {S}), (32, {O, S}), (17, set())]


@pytest.mark.parametrize("tail,enc", [(1, 1), (0, 0)])
def test_one_handle_alternating_between_batches_and_past_eight_graphs(srcfd, enc_weights, dec_weights, tail, enc):
    """Three rounds over KEYS on one handle: launch is 0, 1, 2 for the first eight keys and 0, 0, 0 for the others.  All graphs and
    plain steps share one set of activation, gradient and slab buffers, and a small step follows a large one that left more slabs
    behind; every call must give the bits of a fresh handle's first call at that n."""
    require_gpu(srcfd)
    assert len(KEYS) >= 10 and len({(n, frozenset(f)) for n, f in KEYS}) == len(KEYS) and all(n in tb.BATCHES for n, _ in KEYS)
    assert all((a[0] >= 20) != (b[0] >= 20) for a, b in zip(KEYS[:8], KEYS[1:8]))   # large, small, large, ...
    specs = tb.sr_case(srcfd, enc_weights, dec_weights, 32)[0]
    t = make_trainer(srcfd, specs, tail, enc)
    try:
        for rnd in range(3):
            for i, (n, flags) in enumerate(KEYS):
                _, x, y, _ = tb.sr_case(srcfd, enc_weights, dec_weights, n)
                g, sse = call(t, *device_batch(x, y, n), overwrite=O in flags, same_params=S in flags)
                assert t.last_step() == want_step(n, tail, rnd if i < 8 else 0), (rnd, i, n, flags, t.last_step())
                g0, sse0 = first_plain(srcfd, enc_weights, dec_weights, n, tail, enc)
                assert same_bits(sse, sse0), (rnd, i, n, flags, sse, sse0)
                assert same_bits(g, g0), (rnd, i, n, flags, int((g.view(np.uint32) != g0.view(np.uint32)).sum()))
    finally:
        t.close()


# ---------------------------------------------------------------------------
# (e) Adam at the benchmarked size
# ---------------------------------------------------------------------------
def test_adam_at_batch_32_with_a_ragged_step(srcfd, enc_weights, dec_weights):
    require_gpu(srcfd)
    _orc().adam_steps_match_reference(srcfd, enc_weights, dec_weights, max_batch=MAX_BATCH, batches=(32, 32, 29, 32))
