"""Every stream-taking entry point on a NON-default stream.

The rest of the suite enqueues on torch's current stream, the legacy default stream, which waits for every blocking stream
and is waited for by them: a launch, memset or copy that ignores its `hip_stream` argument, or an internal stream
(the forward's capture stream, the trainer's second stream) that is not fenced against the caller's, gives the right
answer there and stale data anywhere else.  Here each call is made on a non-blocking side stream with its inputs arriving
behind a delay (tests/stream_order.py, `delayed_call`), and its outputs, cloned on that stream, must equal the same
call's result on the default stream BIT FOR BIT.  That default-stream result is what the parity, error-map and
training-oracle tests pin to the float64 oracle; one sample per precision is anchored to the oracle here too, at the bar
of the corresponding parity test.  No tolerance is new.

Two conditions keep the method honest, both asserted: the side stream is still busy when the call under test returns
(`assert_pending`: the delay outlasted the enqueue, and the call did not synchronise), and side streams really run
independently of the default stream on this machine (`test_negative_control_...`: a default-stream call made while the real
input still waits behind the delay sees the decoy).
"""
import ctypes as C
import importlib
import signal

import numpy as np
import pytest

from conftest import ENCODER_H5, STATS_TXT, require_gpu
from test_gpu_parity_bf16 import TOL as TOL_16
from test_gpu_parity_bf16 import _coarse_batch
from test_gpu_parity_fp32 import TOL_FP32

import stream_order as so

gpu = pytest.mark.gpu
RESAMPLE_REL = 1e-12          # the bar of tests/test_resample.py: |out - einsum|_max <= 1e-12 |einsum|_max
ORACLE_BAR = {"fp32": TOL_FP32, "fp32x3": TOL_FP32, "fp32_naive": TOL_FP32, "bf16": TOL_16["bf16"][1], "f16": TOL_16["f16"][1]}
PRECISIONS = ["bf16", "f16", "fp32", "fp32x3", "fp32_naive"]

# include/srcfd.h function with a `hip_stream` parameter -> the tests below that call it on a side stream
COVERED = {
    "srcfd_predict_device": ["test_predict_device_on_a_side_stream", "test_predict_device_16_bit_outputs", "test_predict_device_other_tail",
                             "test_predict_device_affines_guard_and_counter", "test_predict_device_cold_handle",
                             "test_two_handles_on_two_streams", "test_pipeline_batch_on_a_side_stream"],
    "srcfd_resample_device": ["test_resample_device_on_a_side_stream", "test_pipeline_batch_on_a_side_stream"],
    "srcfd_prepare_inputs_device": ["test_prepare_inputs_device_on_a_side_stream", "test_pipeline_batch_on_a_side_stream"],
    "srcfd_trainer_forward_backward": ["test_training_on_a_side_stream[c_entry]"],
    "srcfd_trainer_forward_backward_ex": ["test_training_on_a_side_stream[step]", "test_training_on_a_side_stream[step_no_graph]",
                                          "test_training_on_a_side_stream[accumulate]"],
    "srcfd_adam_step": ["test_training_on_a_side_stream[step]", "test_training_on_a_side_stream[step_no_graph]",
                        "test_training_on_a_side_stream[accumulate]", "test_training_on_a_side_stream[c_entry]"],
}


def test_every_stream_taking_entry_point_is_covered():
    """A function of include/srcfd.h that takes a `hip_stream` and is not listed in COVERED (or a listed one that is gone, or a
    listed test that does not exist) fails here: a new stream-taking entry point cannot be added without a side-stream test."""
    declared = so.stream_entry_points()
    assert len(declared) >= 6, declared
    assert declared == set(COVERED), f"not covered: {sorted(declared - set(COVERED))}; no longer declared: {sorted(set(COVERED) - declared)}"
    for fn, tests in COVERED.items():
        assert tests, fn
        for t in tests:
            assert callable(globals().get(t.split("[")[0])), (fn, t)
    # the parser itself: comments and other parameters do not confuse it
    sample = "/* f(void* hip_stream); */ int srcfd_a(int n, void* hip_stream);\nint srcfd_b(int hip_streams);\n" \
             "int srcfd_c(const float* x,\n            void* hip_stream);  // srcfd_d(void* hip_stream);\n"
    assert so.stream_entry_points(sample) == {"srcfd_a", "srcfd_c"}


@pytest.fixture(autouse=True)
def _time_limit(request):
    """Every test here runs under its own time limit (each takes a few seconds)."""
    def _alarm(*_):
        raise TimeoutError(f"{request.node.name} exceeded its time limit")
    old = signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def ctx(srcfd):
    """torch, the calibrated delay, and two non-blocking side streams."""
    require_gpu(srcfd)
    import torch

    class Ctx:
        pass
    c = Ctx()
    c.torch = torch
    c.delay = so.Delay(torch)
    c.S, c.S2 = torch.cuda.Stream(), torch.cuda.Stream()
    print(f"[stream order] delay {so.DELAY_MS:g} ms asked, {c.delay.measured_ms:.1f} ms measured "
          f"({'spin kernel, %d cycles' % c.delay.cycles if c.delay.cycles else '%d matrix products' % c.delay.matmuls})")
    yield c
    print(f"[stream order] longest enqueue of a call under test: {so.longest_enqueue[0] * 1e3:.2f} ms ({so.longest_enqueue[1]})")


@pytest.fixture(scope="module")
def data(srcfd, oracle, enc_weights, dec_weights, coarse_cases):
    """Seeded inputs shared by the predict tests: `real`, `other` and `decoy`, 100 samples each (a test takes the first n).
    Sample 0 of `real` is a real standardised coarse field, the kind the parity tests hold to their bars; its float64
    oracle result is computed once."""
    rng = np.random.default_rng(20260)
    real, other, decoy = (rng.standard_normal((100, 10, 10, 1)).astype(np.float32) for _ in range(3))
    real[0] = _coarse_batch(coarse_cases, srcfd)[0]
    return {"real": real, "other": other, "decoy": decoy, "oracle0": oracle.superres_forward(real[:1], enc_weights, dec_weights, np.float64)}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _default_stream_predict(torch, m, x, out_dtype=None, **kw):
    """The reference: the call as every other test makes it, on the default stream, into a buffer of its own."""
    y = torch.empty((x.shape[0], 400, 400, 1), dtype=out_dtype or torch.float32, device="cuda")
    m.predict_device(x, y, **kw)
    torch.cuda.synchronize()
    return y


def _side_stream_predicts(ctx, m, n, reals, refs, decoy, ref_decoy, plans, out_dtype=None, label=""):
    """`len(reals)` identical calls (one x, one y: the hipGraph key of engine.hip) on ctx.S; before each, x holds `decoy` and
    y the decoy's result; the real input of call i arrives behind the delay.  Checks results, the plan of each call and that
    the stream was busy when each call returned."""
    torch = ctx.torch
    x = torch.empty_like(decoy)
    y = torch.empty_like(ref_decoy)
    for i, (real, ref, plan) in enumerate(zip(reals, refs, plans)):
        what = f"{label} n={n} call {i + 1} ({plan})"
        o = so.delayed_call(torch, ctx.delay, ctx.S, [so.Arrival(x, decoy, real)], lambda: m.predict_device(x, y, stream=ctx.S), [y],
                            stale=[(y, ref_decoy)], label=what)
        got_plan = m.last_plan()
        print(f"[stream order] {what}: enqueue {o.enqueue_s * 1e3:.2f} ms, stream busy at return: {o.pending}, plan {got_plan}")
        assert got_plan["graph"] == plan, (what, got_plan)
        so.assert_pending(o, what)
        so.assert_bit_equal(o.clones[0], ref, what)


@gpu
def test_negative_control_side_streams_do_not_wait_for_the_default_stream(srcfd, ctx, data, enc_weights, dec_weights):
    """No product code is under test here.  Same set-up as everywhere below, but the forward is enqueued on the DEFAULT stream
    while the real input still waits behind the delay on the side stream: it must see the decoy.  If it sees the real input,
    this machine serialises the two streams and every other test of this file proves nothing."""
    torch = ctx.torch
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = "bf16"
    real, decoy = _dev(torch, data["real"][:3]), _dev(torch, data["decoy"][:3])
    ref_real = _default_stream_predict(torch, m, real)
    ref_decoy = _default_stream_predict(torch, m, decoy)
    assert not torch.equal(ref_real, ref_decoy)
    x, y = decoy.clone(), torch.zeros_like(ref_decoy)
    torch.cuda.synchronize()
    ctx.delay.enqueue(ctx.S)
    with torch.cuda.stream(ctx.S):
        x.copy_(real, non_blocking=True)
    m.predict_device(x, y)                       # default stream
    got = y.clone()
    torch.cuda.current_stream().synchronize()
    still_waiting = not ctx.S.query()
    ctx.S.synchronize()
    assert still_waiting, "the delay on the side stream ended before the default-stream forward did: lengthen stream_order.DELAY_MS"
    assert not torch.equal(got, ref_real), ("the default-stream forward saw the input that was still queued behind the delay on the side "
                                            "stream: streams are serialised here, the delayed-arrival tests of this file prove nothing")
    so.assert_bit_equal(got, ref_decoy, "negative control (expects the DECOY's result)")
    print("[stream order] negative control: the default-stream call saw the decoy, as it must")


@gpu
@pytest.mark.parametrize("n", [3, 65, 100])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_predict_device_on_a_side_stream(srcfd, oracle, ctx, data, enc_weights, dec_weights, precision, n):
    """n = 3: the graph path -- plain launches, capture, replay, replay, the last with NEW contents at the same address.
    n = 65: fp32x3's split-bf16 launches (from 64 samples on; asserted from the profile), a graph of more launches and another
    tail segmentation.  n = 100: above the 96-sample graph threshold, plain launches every time."""
    torch = ctx.torch
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = precision
    real, other, decoy = (_dev(torch, data[k][:n]) for k in ("real", "other", "decoy"))
    ref_real = _default_stream_predict(torch, m, real)
    err = oracle.rel_l2(ref_real[:1].cpu().numpy(), data["oracle0"])
    print(f"[stream order] {precision} n={n}: sample 0 vs float64 oracle {err:.2e} (bar {ORACLE_BAR[precision]:g})")
    assert err <= ORACLE_BAR[precision]
    if precision == "fp32x3":
        m.set_profiling(True)
        m.predict_device(real, torch.empty_like(ref_real))
        names = [nm for nm, _ in m.get_profile()]
        m.set_profiling(False)
        assert sum(nm.endswith("(x3)") for nm in names) == (3 if n >= 64 else 0), names
    ref_other = _default_stream_predict(torch, m, other)
    ref_decoy = _default_stream_predict(torch, m, decoy)      # last: what the handle's buffers hold now derives from the decoy
    assert not torch.equal(ref_real, ref_decoy) and not torch.equal(ref_other, ref_decoy)
    if n == 3:
        reals, refs, plans = [real, real, real, other], [ref_real, ref_real, ref_real, ref_other], ["eager", "capture", "replay", "replay"]
    elif n == 65:
        reals, refs, plans = [real, other, real], [ref_real, ref_other, ref_real], ["eager", "capture", "replay"]
    else:
        reals, refs, plans = [real, other], [ref_real, ref_other], ["eager", "eager"]
    _side_stream_predicts(ctx, m, n, reals, refs, decoy, ref_decoy, plans, label=precision)


@gpu
@pytest.mark.parametrize("precision,out", [("bf16", "bfloat16"), ("f16", "float16")])
def test_predict_device_16_bit_outputs(srcfd, ctx, data, enc_weights, dec_weights, precision, out):
    torch = ctx.torch
    odt = getattr(torch, out)
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = precision
    n = 5
    real, decoy = _dev(torch, data["real"][:n]), _dev(torch, data["decoy"][:n])
    ref_real = _default_stream_predict(torch, m, real, out_dtype=odt)
    ref_decoy = _default_stream_predict(torch, m, decoy, out_dtype=odt)
    assert not torch.equal(so.bits(ref_real), so.bits(ref_decoy))
    _side_stream_predicts(ctx, m, n, [real] * 3, [ref_real] * 3, decoy, ref_decoy, ["eager", "capture", "replay"], label=f"{precision}->{out}")


@gpu
def test_predict_device_other_tail(srcfd, ctx, data, enc_weights, dec_weights, monkeypatch):
    """The second tail kernel (SRCFD_TAIL=s) at a segmentation the launcher would not choose itself (13 samples: 10)."""
    torch = ctx.torch
    monkeypatch.setenv("SRCFD_TAIL", "s")
    monkeypatch.setenv("SRCFD_TAIL_SEG", "5")
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = "bf16"
    n = 13
    real, decoy = _dev(torch, data["real"][:n]), _dev(torch, data["decoy"][:n])
    ref_real = _default_stream_predict(torch, m, real)
    assert m.last_plan()["tail"] == "tail16s" and m.last_plan()["tail_seg"] == "5", m.last_plan()
    ref_decoy = _default_stream_predict(torch, m, decoy)
    _side_stream_predicts(ctx, m, n, [real] * 3, [ref_real] * 3, decoy, ref_decoy, ["eager", "capture", "replay"], label="bf16 tail16s seg 5")
    assert m.last_plan()["tail"] == "tail16s" and m.last_plan()["tail_seg"] == "5", m.last_plan()


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_predict_device_affines_guard_and_counter(srcfd, ctx, data, enc_weights, dec_weights, precision):
    """in_affine, out_affine and the NaN guard on a poisoned sample; x, both affines and the `nonfinite` counter all arrive
    behind the delay.  The counter is ADDED to: it holds 3 (the decoy), becomes 7 behind the delay, and must end at 7 + the
    default-stream count -- the add happened in stream order, after the write of the 7."""
    torch = ctx.torch
    m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    m.precision = precision
    n = 7
    rng = np.random.default_rng(7)

    def affine():
        return _dev(torch, np.stack([rng.standard_normal(n) * 0.1, rng.uniform(0.05, 0.3, n)], 1).astype(np.float32))
    xr = data["real"][:n].copy()
    xr[4, 2, 2, 0] = np.nan                     # poisons the whole of sample 4 through the dense layers
    real, decoy = _dev(torch, xr), _dev(torch, data["decoy"][:n])
    ain_r, aout_r, ain_d, aout_d = affine(), affine(), affine(), affine()
    cnt_ref = torch.zeros(1, dtype=torch.int64, device="cuda")
    ref_real = _default_stream_predict(torch, m, real, in_affine=ain_r, out_affine=aout_r, nan_guard=True, nonfinite=cnt_ref)
    bad = int(cnt_ref.item())
    assert bad > 0 and bool(torch.isfinite(ref_real).all()) and bool((ref_real[4] == 0).all())
    ref_decoy = _default_stream_predict(torch, m, decoy, in_affine=ain_d, out_affine=aout_d, nan_guard=True,
                                        nonfinite=torch.zeros(1, dtype=torch.int64, device="cuda"))
    x, ain, aout, y = torch.empty_like(real), torch.empty_like(ain_r), torch.empty_like(aout_r), torch.empty_like(ref_real)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    three, seven = torch.full_like(cnt, 3), torch.full_like(cnt, 7)
    arrivals = [so.Arrival(x, decoy, real), so.Arrival(ain, ain_d, ain_r), so.Arrival(aout, aout_d, aout_r), so.Arrival(cnt, three, seven)]
    for i, plan in enumerate(["eager", "capture", "replay"]):
        what = f"{precision} affines + guard call {i + 1} ({plan})"
        o = so.delayed_call(torch, ctx.delay, ctx.S, arrivals,
                            lambda: m.predict_device(x, y, in_affine=ain, out_affine=aout, nan_guard=True, nonfinite=cnt, stream=ctx.S),
                            [y, cnt], stale=[(y, ref_decoy)], label=what)
        assert m.last_plan()["graph"] == plan, (what, m.last_plan())
        so.assert_pending(o, what)
        so.assert_bit_equal(o.clones[0], ref_real, what)
        assert int(o.clones[1].item()) == 7 + bad, (what, int(o.clones[1].item()))


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_predict_device_cold_handle(srcfd, ctx, data, enc_weights, dec_weights, precision):
    """The FIRST call of a fresh handle, on the side stream: lazy packing and allocation happen inside it and may synchronise,
    so only the result is checked (against another handle's default-stream call), not that the stream was still busy."""
    torch = ctx.torch
    n = 4
    real, decoy = _dev(torch, data["real"][:n]), _dev(torch, data["decoy"][:n])
    warm = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    warm.precision = precision
    ref_real = _default_stream_predict(torch, warm, real)
    ref_decoy = _default_stream_predict(torch, warm, decoy)
    cold = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    cold.precision = precision
    x, y = torch.empty_like(real), torch.empty_like(ref_real)
    o = so.delayed_call(torch, ctx.delay, ctx.S, [so.Arrival(x, decoy, real)], lambda: cold.predict_device(x, y, stream=ctx.S), [y],
                        stale=[(y, ref_decoy)], label=f"{precision} cold handle")
    print(f"[stream order] {precision} cold first call: enqueue {o.enqueue_s * 1e3:.2f} ms, stream busy at return: {o.pending} (not asserted)")
    so.assert_bit_equal(o.clones[0], ref_real, f"{precision} cold handle")


@gpu
def test_two_handles_on_two_streams(srcfd, ctx, data, enc_weights, dec_weights):
    """"Distinct handles may be used" at once: a bf16 handle on one side stream and an fp32 handle on another, each behind a
    delay of its own, enqueued A, B, A, B over three rounds with nothing synchronised in between.  Each result equals its
    handle's serial default-stream result."""
    torch = ctx.torch
    n = 3
    handles = []
    for precision, stream in (("bf16", ctx.S), ("fp32", ctx.S2)):
        m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
        m.precision = precision
        ins = [_dev(torch, data[k][:n]) for k in ("real", "other", "real")]
        decoy = _dev(torch, data["decoy"][:n])
        refs = [_default_stream_predict(torch, m, v) for v in ins]
        ref_decoy = _default_stream_predict(torch, m, decoy)
        handles.append(dict(m=m, S=stream, ins=ins, refs=refs, decoy=decoy, x=torch.empty_like(decoy), y=torch.empty_like(ref_decoy),
                            ref_decoy=ref_decoy, got=[], name=precision))
    for h in handles:
        h["x"].copy_(h["decoy"])
        h["y"].copy_(h["ref_decoy"])
    torch.cuda.synchronize()
    pending = []
    for rnd in range(3):
        for h in handles:
            with torch.cuda.stream(h["S"]):
                ctx.delay.enqueue(h["S"])
                h["x"].copy_(h["ins"][rnd], non_blocking=True)
                h["m"].predict_device(h["x"], h["y"], stream=h["S"])
                pending.append(not h["S"].query())
                h["got"].append(h["y"].clone())
                h["x"].copy_(h["decoy"], non_blocking=True)       # the decoy is back before the next round's delay
    for h in handles:
        h["S"].synchronize()
    assert all(pending), f"a stream had drained when a call returned: {pending}"
    for h in handles:
        assert h["m"].last_plan()["graph"] == "replay", h["m"].last_plan()
        for rnd in range(3):
            so.assert_bit_equal(h["got"][rnd], h["refs"][rnd], f"two handles: {h['name']} round {rnd + 1}")


@gpu
@pytest.mark.parametrize("case", ["two_gemms", "ry_identity", "rx_identity", "both_identity"])
def test_resample_device_on_a_side_stream(srcfd, ctx, case):
    """Resampler.apply_device(stream=): the two chained float64 GEMMs (the second reads d_T, which the first writes) at the
    ragged 37x53 -> 41x29 of tests/test_resample.py, and each identity-skip path, two planes."""
    torch = ctx.torch
    rs = importlib.import_module("sr-for-cfd_amd.resample")
    rng = np.random.default_rng(41)
    H, W, OH, OW = 37, 53, 41, 29
    Ry, Rx = rng.standard_normal((OH, H)), rng.standard_normal((OW, W))
    if case in ("ry_identity", "both_identity"):
        Ry, OH = np.eye(H), H
    if case in ("rx_identity", "both_identity"):
        Rx, OW = np.eye(W), W
    r = rs.Resampler(Ry, Rx, 0)
    g_real, g_decoy = (rng.standard_normal((2, H, W)).astype(np.float32) for _ in range(2))
    real, decoy = _dev(torch, g_real), _dev(torch, g_decoy)
    ref_real = r.apply_device(real)
    torch.cuda.synchronize()
    want = np.einsum("oh,zhw,pw->zop", Ry, g_real.astype(np.float64), Rx)
    assert np.abs(ref_real.cpu().numpy() - want).max() <= RESAMPLE_REL * np.abs(want).max()
    ref_decoy = r.apply_device(decoy)                     # last: d_T now holds the decoy's intermediate
    torch.cuda.synchronize()
    x, out = torch.empty_like(real), torch.empty_like(ref_real)
    for i in range(2):
        what = f"resample {case} call {i + 1}"
        o = so.delayed_call(torch, ctx.delay, ctx.S, [so.Arrival(x, decoy, real)],
                            lambda: r.apply_device(x, out=out, stream=ctx.S.cuda_stream), [out], stale=[(out, ref_decoy)], label=what)
        so.assert_pending(o, what)
        so.assert_bit_equal(o.clones[0], ref_real, what)
        if i == 0:                                        # the handle's intermediate derives from the decoy again before the second call
            r.apply_device(decoy)
            torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("resample", [True, False], ids=["resampled", "as_is"])
def test_prepare_inputs_device_on_a_side_stream(srcfd, ctx, coarse_cases, resample):
    """srcfd_prepare_inputs_device, 6 samples of 10 x 10, adaptive blend on, with and without Ry / Rx: the fields and the
    training statistics arrive behind the delay; x and the (mean, std) pairs equal the default-stream call's bit for bit."""
    torch = ctx.torch
    rs = importlib.import_module("sr-for-cfd_amd.resample")
    L = importlib.import_module("sr-for-cfd_amd._lib")
    rng = np.random.default_rng(6)
    base = coarse_cases["bfs_Re400"]
    n = 6

    def fields():
        two = [{c: base[c] * (1 + 0.05 * rng.standard_normal()) + 0.01 * rng.standard_normal((10, 10)) for c in "uvp"} for _ in range(2)]
        return _dev(torch, np.stack([np.stack([b[c] for c in "uvp"]) for b in two]).reshape(n, 10, 10).astype(np.float64))

    def stats():
        return _dev(torch, np.stack([rng.standard_normal(n) * 0.2, rng.uniform(0.1, 2.0, n)], 1))
    f_real, f_decoy, t_real, t_decoy = fields(), fields(), stats(), stats()
    Ry = Rx = None
    if resample:
        ry, rx = rs.rect_to_square_matrices(10, 10, 10.0, 3.0)
        Ry, Rx = _dev(torch, np.array(ry)), _dev(torch, np.array(rx))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def prepare(f, t, x, ain, stream):
        L.check(L.lib.srcfd_prepare_inputs_device(p(f), n, 10, 10, p(Ry), p(Rx), 10, p(t), 1, 0.3, p(x), p(ain), C.c_void_p(stream)))
    new = lambda: (torch.empty((n, 10, 10), dtype=torch.float32, device="cuda"), torch.empty((n, 2), dtype=torch.float32, device="cuda"))
    (x_ref, a_ref), (x_dec, a_dec), (x, ain) = new(), new(), new()
    prepare(f_real, t_real, x_ref, a_ref, None)
    prepare(f_decoy, t_decoy, x_dec, a_dec, None)
    torch.cuda.synchronize()
    assert not torch.equal(x_ref, x_dec) and not torch.equal(a_ref, a_dec)
    f, t = torch.empty_like(f_real), torch.empty_like(t_real)
    what = f"prepare_inputs {'resampled' if resample else 'as is'}"
    o = so.delayed_call(torch, ctx.delay, ctx.S, [so.Arrival(f, f_decoy, f_real), so.Arrival(t, t_decoy, t_real)],
                        lambda: prepare(f, t, x, ain, ctx.S.cuda_stream), [x, ain], stale=[(x, x_dec), (ain, a_dec)], label=what)
    so.assert_pending(o, what)
    so.assert_bit_equal(o.clones[0], x_ref, what + ": x")
    so.assert_bit_equal(o.clones[1], a_ref, what + ": (mean, std)")


BATCHES = (8, 8, 8, 7, 8, 8)      # one graph key for the full batches (plain, capture, replay ...) and a second one for the ragged step


def _training_batches():
    rng = np.random.default_rng(900)
    out = []
    for n in BATCHES + (8,):       # the last one is the decoy
        x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
        y = rng.standard_normal((n, 400, 400, 1)).astype(np.float32)
        y[:, :1] += 2.0
        y[:, :, -1:] -= 2.0
        out.append((x, y))
    return out


@gpu
@pytest.mark.parametrize("mode", ["step", "step_no_graph", "accumulate", "c_entry"])
def test_training_on_a_side_stream(srcfd, ctx, enc_weights, dec_weights, mode, monkeypatch):
    """Six optimiser steps on batches of 8, 8, 8, 7, 8, 8 samples under `with torch.cuda.stream(S)`, every batch arriving behind
    the delay (and, at the first step, the parameters too): the plain pass, the capture, replays, a second graph key for the
    ragged step, the staging copy in front of a replayed graph, the fork to the trainer's second stream and the join back,
    Adam.  After each step params, grads, m, v and sse -- cloned on S -- equal, bit for bit, those of a second fresh Trainer fed
    the same batches on the default stream.
    step: Trainer.step(return_loss=False).  step_no_graph: the same with SRCFD_TRAIN_GRAPH=0 (plain launches fork and join on
    every call).  accumulate: grads.zero_() and sse.zero_() enqueued on S, forward_backward(overwrite=False), apply_adam().
    c_entry: accumulate through srcfd_trainer_forward_backward, the entry without flags, called directly."""
    torch = ctx.torch
    tr = importlib.import_module("sr-for-cfd_amd.train")
    L = importlib.import_module("sr-for-cfd_amd._lib")
    if mode == "step_no_graph":
        monkeypatch.setenv("SRCFD_TRAIN_GRAPH", "0")      # read when a trainer is created
    specs = srcfd.layers_from_weights(enc_weights, dec_weights)
    host = _training_batches()
    dev = [(_dev(torch, x), _dev(torch, y)) for x, y in host]
    batches, (x_decoy, y_decoy) = dev[:-1], dev[-1]

    def one_step(t, x, y):
        n = int(x.shape[0])
        if mode in ("step", "step_no_graph"):
            t.step(x, y, return_loss=False)
            return
        t.grads.zero_()
        t.sse.zero_()
        if mode == "accumulate":
            t.forward_backward(x, y, overwrite=False)
        else:
            st = torch.cuda.current_stream()
            L.check(L.lib.srcfd_trainer_forward_backward(t._h, C.c_void_p(t.params.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                                         n, C.c_float(1.0 / (n * t.out_elems)), C.c_void_p(t.grads.data_ptr()),
                                                         C.c_void_p(t.sse.data_ptr()), C.c_void_p(st.cuda_stream)))
        t.apply_adam()

    def state(t):
        return [t.params, t.grads, t.m, t.v, t.sse]

    # the reference: a fresh trainer, the same batches, the default stream
    t_ref = tr.Trainer(srcfd.SRModel.from_layers(specs, (10, 10, 1), device=0), max_batch=8)
    want = []
    for x, y in batches:
        one_step(t_ref, x, y)
        torch.cuda.synchronize()
        want.append([v.cpu() for v in state(t_ref)])
    assert all(bool(torch.isfinite(v).all()) for v in want[-1]) and not torch.equal(want[0][0], want[-1][0])
    t_ref.close()

    t = tr.Trainer(srcfd.SRModel.from_layers(specs, (10, 10, 1), device=0), max_batch=8)
    p_real = t.params.clone()
    p_decoy = p_real * 0.5
    xb, yb = torch.empty_like(x_decoy), torch.empty_like(y_decoy)
    seen = {}
    for i, (x, y) in enumerate(batches):
        n = int(x.shape[0])
        xs, ys = xb[:n], yb[:n]
        arrivals = [so.Arrival(xs, x_decoy[:n], x), so.Arrival(ys, y_decoy[:n], y)]
        if i == 0:
            arrivals.append(so.Arrival(t.params, p_decoy, p_real))
        what = f"training[{mode}] step {i + 1} (n={n})"
        o = so.delayed_call(torch, ctx.delay, ctx.S, arrivals, lambda: one_step(t, xs, ys), state(t), label=what)
        seen[n] = seen.get(n, 0) + 1
        print(f"[stream order] {what}: enqueue {o.enqueue_s * 1e3:.2f} ms, stream busy at return: {o.pending}")
        if seen[n] >= 2:
            so.assert_pending(o, what)
        for name, got, ref in zip(("params", "grads", "m", "v", "sse"), o.clones, want[i]):
            so.assert_bit_equal(got, ref, f"{what}: {name}")
    assert t.t == len(BATCHES)


@gpu
def test_pipeline_batch_on_a_side_stream(srcfd, ctx, dec_weights, coarse_cases, tmp_path):
    """pipeline.ml_super_resolution_batch end to end (upload, srcfd_prepare_inputs_device, the network, the resampling back, the
    read-back) with a side stream as torch's current stream, the stream busy with a delay when the call starts: 4 BFS fields
    with aspect-ratio correction and the adaptive blend, and an LDC pair without resampling, equal the default-stream call
    bit for bit."""
    torch = ctx.torch
    pl = importlib.import_module("sr-for-cfd_amd.pipeline")
    dec = str(tmp_path / "vanilla_decoder400_from_10_synthetic.h5")
    srcfd.SRModel.from_weights(None, dec_weights, device=-1).save_h5(None, dec)
    rng = np.random.default_rng(77)
    base = coarse_cases["bfs_Re400"]
    bfs = [base] + [{c: base[c] * (1 + 0.05 * rng.standard_normal()) + 0.01 * rng.standard_normal((10, 10)) for c in "uvp"} for _ in range(3)]
    ldc = [coarse_cases["ldc_Re800_double"], coarse_cases["ldc_Re1000_single"]]
    calls = {"bfs": lambda: pl.ml_super_resolution_batch(bfs, 10, 400, STATS_TXT, ENCODER_H5, dec, use_adaptive_normalization=True,
                                                         use_aspect_ratio_correction=True, lx=10.0, ly=3.0, blend_factor=0.3),
             "ldc": lambda: pl.ml_super_resolution_batch(ldc, 10, 400, STATS_TXT, ENCODER_H5, dec)}
    for name, call in calls.items():
        want = call()
        torch.cuda.synchronize()
        with torch.cuda.stream(ctx.S):
            ctx.delay.enqueue(ctx.S)
            got = call()
        ctx.S.synchronize()
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            for c in "uvp":
                assert g[c].dtype == w[c].dtype and g[c].shape == (400, 400)
                np.testing.assert_array_equal(g[c].view(np.uint64 if g[c].dtype == np.float64 else np.uint32),
                                              w[c].view(np.uint64 if w[c].dtype == np.float64 else np.uint32), err_msg=f"{name} field {i} {c}")
