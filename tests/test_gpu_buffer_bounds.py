"""Where the kernels read and write, on an MI355X (tests/guard_bands.py; include/srcfd.h, "conventions").

Every test follows one pattern:
  1. the call once on plain tensors on the same handle: `want`, the project's already-pinned behaviour (no new reference);
  2. the call again with every caller buffer replaced: outputs inside [guard | payload | guard] allocations pre-filled with a NaN
     sentinel, inputs and affine tables with quiet NaNs in both guards, the `nonfinite` counter as the middle of three int64 words,
     starting at 5;
  3. the payload has `want`'s bits and holds no sentinel, every guard word is intact, the counter is 5 + the plain call's count.
Under a graph-capturing path the guarded call is made three times into the same addresses (plain launches, capture, replay).
Every arm asserts the implementation that ran.  A defect shows as a changed guard word, a left-over sentinel or a NaN that the plain
call did not produce -- never as a fault: every guard lies inside an allocation the test owns.

Guards: one full sample on each side of a batch-indexed buffer, 64 floats around an affine table, 4096 elements around a flat
parameter array.  Only srcfd_prepare_inputs_device also gets a value check (its rectangular and lr != h shapes have no history)."""
import ctypes as C
import importlib
import signal

import numpy as np
import pytest

import guard_bands as gb
import lowp16_plan_ref as lref
from conftest import require_gpu

pytestmark = pytest.mark.gpu
OUT_TYPES = ["f32", "bf16", "f16"]


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
def torch_(srcfd):
    require_gpu(srcfd)
    import torch
    return torch


def _mod(name):
    return importlib.import_module("sr-for-cfd_amd." + name)


def _odt(torch, name):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[name]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _affines(rng, n):
    ain = np.stack([rng.standard_normal(n) * 0.1, rng.uniform(0.5, 2.0, n)], 1).astype(np.float32)
    aout = np.stack([rng.standard_normal(n) * 0.1, rng.uniform(0.05, 0.3, n)], 1).astype(np.float32)
    return ain, aout


# ------------------------------------------------------------------------------------------------ predict_device: the pattern
def guarded_predict_device(torch, m, x, out_type, ain, aout, expect, what):
    """The pattern of the module docstring for srcfd_predict_device with the NaN guard on.  `expect(m, n)` asserts the
    implementation that ran.  With two samples or more, sample 0 carries one NaN: the guard zero-fills it and counts it, so the
    counter moves."""
    n = x.shape[0]
    x = x.copy()
    if n >= 2:
        x[(0,) + tuple(s // 2 for s in x.shape[1:])] = np.nan
    odt = _odt(torch, out_type)
    oshape = (n,) + tuple(m.output_shape)
    sample, in_sample = int(np.prod(m.output_shape)), int(np.prod(x.shape[1:]))
    # 1. plain tensors
    xd = dev(torch, x)
    want = torch.empty(oshape, dtype=odt, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    m.predict_device(xd, want, None if ain is None else dev(torch, ain), None if aout is None else dev(torch, aout), nan_guard=True, nonfinite=cnt)
    torch.cuda.synchronize()
    expect(m, n)
    count = int(cnt.item())
    assert (count > 0) == (n >= 2) and count <= sample, (what, count)
    # 2. every caller buffer replaced
    _, xg = gb.poisoned(torch, x, in_sample)
    aing = None if ain is None else gb.poisoned(torch, ain, gb.affine_guard())[1]
    aoutg = None if aout is None else gb.poisoned(torch, aout, gb.affine_guard())[1]
    big, out = gb.guarded(torch, oshape, odt, sample)
    three, c = gb.guarded_counter(torch, 5)
    graphs = []
    for rep in range(3 if n <= 96 else 1):
        if rep:
            gb.refill(big)
            three[1] = 5
        m.predict_device(xg, out, aing, aoutg, nan_guard=True, nonfinite=c)
        torch.cuda.synchronize()
        expect(m, n)
        graphs.append(m.last_plan()["graph"])
        label = f"{what}, guarded call {rep + 1} ({graphs[-1]})"
        # 3.
        gb.assert_guards_intact(big, out, what=label)
        gb.assert_fully_written(out, what=label)
        gb.assert_same_bits(out, want, what=label)
        gb.assert_counter(three, 5 + count, what=label)
    assert graphs == (["eager", "capture", "replay"] if n <= 96 else ["eager"]), (what, graphs)


# ------------------------------------------------------------------------------------------------ 10 -> 400: bf16 and f16 operands
_SR = {}


def _sr(srcfd, enc_weights, dec_weights):
    if "m" not in _SR:
        _SR["m"] = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    return _SR["m"]


def _expect16(torch, kind, tail, mid="mid16_4x64"):
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def expect(m, n):
        p = m.last_plan()
        assert p["precision"] == kind and p["encoder"] == "enc16" and p["dense_1"] == "dense1_16" and p["middle"] == mid and p["tail"] == tail, p
        assert int(p["tail_seg"]) == lref.tail_seg(lref.DEFAULT, min(n, 1024), cus), (p, n, cus)
    return expect


def _sr_x(n, seed=0):
    return np.random.default_rng(1000 * n + seed).standard_normal((n, 10, 10, 1)).astype(np.float32)


def test_the_batch_sizes_of_the_16_bit_arm_differ_where_they_should(torch_):
    """n = 1 and n = 13 run different segmentations; 5 and 6 are the full and the partial last workgroup of enc16 (5 samples per
    workgroup); 300 samples of up to 25 segments exceed the workgroups of the tail, so one workgroup walks several samples."""
    cus = torch_.cuda.get_device_properties(0).multi_processor_count
    assert lref.tail_seg(lref.DEFAULT, 1, cus) != lref.tail_seg(lref.DEFAULT, 13, cus)
    assert lref.E_G == 5 and lref.ceil_div(5, lref.E_G) == 1 and lref.ceil_div(6, lref.E_G) == 2
    assert 300 * lref.tail_seg(lref.DEFAULT, 300, cus) > cus


@pytest.mark.parametrize("affine", [False, True], ids=["raw", "affine"])
@pytest.mark.parametrize("n", [1, 2, 5, 6, 13])
@pytest.mark.parametrize("tail", ["tail16", "tail16s"])
@pytest.mark.parametrize("out_type", OUT_TYPES)
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_predict_device_16_bit(srcfd, torch_, enc_weights, dec_weights, monkeypatch, kind, out_type, tail, n, affine):
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = kind
    if tail == "tail16s":
        monkeypatch.setenv("SRCFD_TAIL", "s")
    ain, aout = _affines(np.random.default_rng(n), n) if affine else (None, None)
    guarded_predict_device(torch_, m, _sr_x(n), out_type, ain, aout, _expect16(torch_, kind, tail), f"{kind} -> {out_type}, {tail}, n={n}")


def test_predict_device_bf16_300_samples(srcfd, torch_, enc_weights, dec_weights):
    """More samples than workgroups: one workgroup walks several samples.  About 0.4 GB goes through the comparisons, on the device."""
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "bf16"
    guarded_predict_device(torch_, m, _sr_x(300), "f32", None, None, _expect16(torch_, "bf16", "tail16"), "bf16 -> f32, tail16, n=300")


@pytest.mark.parametrize("mid", ["0", "1", "2"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_predict_device_16_bit_other_middles(srcfd, torch_, enc_weights, dec_weights, monkeypatch, kind, mid):
    """SRCFD_MID = 0, 1, 2 at n = 3: the generic GEMM middle and the other workgroup shapes of mid16 write their last tiles."""
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = kind
    monkeypatch.setenv("SRCFD_MID", mid)
    name = {"0": "gemm16", "1": "mid16_8x32", "2": "mid16_8x64"}[mid]
    ain, aout = _affines(np.random.default_rng(3), 3)
    guarded_predict_device(torch_, m, _sr_x(3), "f32", ain, aout, _expect16(torch_, kind, "tail16", mid=name), f"{kind}, SRCFD_MID={mid}")


# ------------------------------------------------------------------------------------------------ 10 -> 400: the f32-grade precisions
def _expect32(precision, first, last, x3=False):
    """`first`, `last`: the kernels of the forward's first and last step (srcfd_model_f32_steps under the environment's switches)."""
    def expect(m, n):
        assert m.last_plan()["precision"] == precision, m.last_plan()
        steps = m.f32_steps(n)
        assert steps[0][1] == first and steps[-1][1] == last, steps
        assert any(k == "x3" for _, k, _ in steps) == x3, steps
    return expect


@pytest.mark.parametrize("n", [1, 3, 13])
@pytest.mark.parametrize("out_type", OUT_TYPES)
def test_predict_device_fp32(srcfd, torch_, enc_weights, dec_weights, out_type, n):
    """enc32 through tail32."""
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32"
    ain, aout = _affines(np.random.default_rng(n), n)
    guarded_predict_device(torch_, m, _sr_x(n), out_type, ain, aout, _expect32("fp32", "enc32", "tail32"), f"fp32 -> {out_type}, n={n}")


@pytest.mark.parametrize("out_type", OUT_TYPES)
def test_predict_device_fp32_without_the_streaming_tail(srcfd, torch_, enc_weights, dec_weights, monkeypatch, out_type):
    """SRCFD_NO_TAIL32=1: the last layer is the tiled one-channel output convolution, which also converts and guards."""
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32"
    monkeypatch.setenv("SRCFD_NO_TAIL32", "1")
    ain, aout = _affines(np.random.default_rng(3), 3)
    guarded_predict_device(torch_, m, _sr_x(3), out_type, ain, aout, _expect32("fp32", "enc32", "finalize"), f"fp32 -> {out_type}, SRCFD_NO_TAIL32=1")


def test_predict_device_fp32_layer_by_layer_encoder(srcfd, torch_, enc_weights, dec_weights, monkeypatch):
    """SRCFD_NO_ENC32=1: the standardize_f32 launch in front of the layer-by-layer encoder."""
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32"
    monkeypatch.setenv("SRCFD_NO_ENC32", "1")
    ain, aout = _affines(np.random.default_rng(3), 3)
    guarded_predict_device(torch_, m, _sr_x(3), "f32", ain, aout, _expect32("fp32", "mfma", "tail32"), "fp32, SRCFD_NO_ENC32=1")
    m.set_profiling(True)
    m.predict(_sr_x(3), in_affine=ain)
    names = [nm for nm, _ in m.get_profile()]
    m.set_profiling(False)
    assert names[0] == "standardize", names


@pytest.mark.parametrize("out_type", OUT_TYPES)
def test_predict_device_fp32_naive(srcfd, torch_, enc_weights, dec_weights, out_type):
    """The bring-up path: every layer materialised, finalize_out converts, de-standardises and guards."""
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32_naive"
    ain, aout = _affines(np.random.default_rng(2), 2)
    guarded_predict_device(torch_, m, _sr_x(2), out_type, ain, aout, _expect32("fp32_naive", "naive", "naive"), f"fp32_naive -> {out_type}")
    m.set_profiling(True)
    m.predict(_sr_x(2))
    names = [nm for nm, _ in m.get_profile()]
    m.set_profiling(False)
    assert names[-1] == "finalize", names


@pytest.mark.parametrize("n", [64, 70])
def test_predict_device_fp32x3(srcfd, torch_, enc_weights, dec_weights, n):
    """From 64 samples on: ConvT#0, ConvT#1 and the first two layers of the streaming tail on the split-bf16 kernels."""
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32x3"
    ain, aout = _affines(np.random.default_rng(n), n)
    x = _sr_x(n)
    guarded_predict_device(torch_, m, x, "f32", ain, aout, _expect32("fp32x3", "enc32", "tail32", x3=True), f"fp32x3, n={n}")
    m.set_profiling(True)           # a separate call: profiling disables graphs
    m.predict(x)
    names = [nm for nm, _ in m.get_profile()]
    m.set_profiling(False)
    assert sum(nm.endswith("(x3)") for nm in names) == 3 and names[-1].endswith("(x3)"), names     # ConvT#0, ConvT#1, tail32<X3>


# ------------------------------------------------------------------------------------------------ the model family
_FAMILY = {}


def _family_model(srcfd, enc_weights, hr):
    if hr not in _FAMILY:
        _FAMILY[hr] = srcfd.SRModel.from_weights(enc_weights, _mod("family").synthetic_decoder_weights(hr, seed=20 + hr), device=0)
    return _FAMILY[hr]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("out_type", OUT_TYPES)
@pytest.mark.parametrize("precision", ["bf16", "f16", "fp32"])
@pytest.mark.parametrize("hr", [20, 50])
def test_predict_device_model_family(srcfd, torch_, enc_weights, hr, precision, out_type, n):
    """encoder_10 + decoder_20 / decoder_50, weights as tests/test_gpu_model_family.py builds them: the 'same' transposed
    convolutions crop their last row and column."""
    m = _family_model(srcfd, enc_weights, hr)
    assert m.output_shape == (hr, hr, 1)
    m.precision = precision
    if precision == "fp32":
        expect = _expect32("fp32", "enc32", "mfma")
    else:
        def expect(mm, _n):
            p = mm.last_plan()
            assert p["precision"] == precision and p["decoder"] == "any16" and p["encoder"] == "enc16", p
    ain, aout = _affines(np.random.default_rng(hr + n), n)
    guarded_predict_device(torch_, m, _sr_x(n, seed=hr), out_type, ain, aout, expect, f"decoder_{hr} {precision} -> {out_type}, n={n}")


# ------------------------------------------------------------------------------------------------ generic graphs
def _conv(rng, k, cin, cout, stride=1, same=True, act="swish"):
    return dict(kind="conv2d", k=k, stride=stride, same=same, act=act, w=(rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32),
                b=(0.1 * rng.standard_normal(cout)).astype(np.float32))


def _generic(name):
    """(specs, input shape, n, the kernel of the last step)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "dense_7":           # 3 x 7 = 21 output elements: an odd count of 16-bit values
        w = (rng.standard_normal((5 * 6 * 4, 7)) / np.sqrt(120)).astype(np.float32)
        return [_conv(rng, 3, 2, 4), dict(kind="flatten"), dict(kind="dense", act="linear", w=w, b=(0.1 * rng.standard_normal(7)).astype(np.float32))], (5, 6, 2), 3, "mfma"
    if name == "convt_3x3_s2_to_3":  # multi-channel transposed-convolution output, 11 x 15 x 3
        w = (rng.standard_normal((3, 3, 3, 4)) / 2).astype(np.float32)
        return [_conv(rng, 3, 2, 4), dict(kind="conv2d_transpose", k=3, stride=2, same=False, act="linear", w=w, b=(0.1 * rng.standard_normal(3)).astype(np.float32))], (5, 7, 2), 3, "group"
    if name == "strided_same_conv":  # 5 x 7 -> 3 x 4: cropped output
        return [_conv(rng, 3, 2, 4), _conv(rng, 3, 4, 3, stride=2, act="linear")], (5, 7, 2), 3, "mfma"
    if name == "conv_n1_17x65":      # one past the one-channel output convolution's 16 x 64 tile in both directions
        return [_conv(rng, 3, 2, 8), _conv(rng, 3, 8, 1, act="linear")], (17, 65, 2), 3, "finalize"
    raise KeyError(name)


@pytest.mark.parametrize("out_type", OUT_TYPES)
@pytest.mark.parametrize("name", ["dense_7", "convt_3x3_s2_to_3", "strided_same_conv", "conv_n1_17x65"])
def test_predict_device_generic_graphs(srcfd, torch_, name, out_type):
    specs, in_shape, n, last = _generic(name)
    m = srcfd.SRModel.from_layers(specs, in_shape, device=0)
    want_shape = {"dense_7": (1, 1, 7), "convt_3x3_s2_to_3": (11, 15, 3), "strided_same_conv": (3, 4, 3), "conv_n1_17x65": (17, 65, 1)}[name]
    assert m.output_shape == want_shape
    x = np.random.default_rng(5).standard_normal((n,) + in_shape).astype(np.float32)
    ain, aout = _affines(np.random.default_rng(6), n)
    guarded_predict_device(torch_, m, x, out_type, ain, aout, _expect32("fp32", "mfma", last), f"{name} -> {out_type}")
    m.close()


# ------------------------------------------------------------------------------------------------ Resampler.apply_device
def _resample_form(Ry, Rx):
    """The form csrc/resample.hip picks: a factor within 1e-13 of the identity is skipped."""
    ident = lambda R: R.shape[0] == R.shape[1] and bool(np.all(np.abs(R - np.eye(R.shape[0])) <= 1e-13))
    return {(False, False): "two_gemms", (True, False): "ry_identity", (False, True): "rx_identity", (True, True): "widen_f64"}[(ident(Ry), ident(Rx))]


def _resample_case(name):
    rs = _mod("resample")
    if name == "37x53_to_41x29":
        return np.array(rs.interp_matrix(37, 1.0, 41, 1.0)), np.array(rs.interp_matrix(53, 2.0, 29, 2.0)), 2, "two_gemms"
    if name == "ry_identity":
        return np.eye(37), np.array(rs.interp_matrix(53, 2.0, 29, 2.0)), 2, "ry_identity"
    if name == "rx_identity":
        return np.array(rs.interp_matrix(37, 1.0, 41, 1.0)), np.eye(53), 2, "rx_identity"
    if name == "double_identity":
        return np.eye(37), np.eye(53), 2, "widen_f64"
    ry, rx = rs.square_to_rect_matrices(400, 400, 400, 10.0, 3.0)     # the BFS pair: the square and the rectangle share their x nodes
    return np.array(ry), np.array(rx), 3, "rx_identity"


@pytest.mark.parametrize("name", ["37x53_to_41x29", "ry_identity", "rx_identity", "double_identity", "bfs_400x400"])
def test_resampler_apply_device(srcfd, torch_, name):
    torch = torch_
    Ry, Rx, n, form = _resample_case(name)
    assert _resample_form(Ry, Rx) == form
    (oh, h), (ow, w) = Ry.shape, Rx.shape
    if form == "widen_f64":
        assert n * h * w % 256 != 0
    r = _mod("resample").Resampler(Ry, Rx, 0)
    x = np.random.default_rng(h + w).standard_normal((n, h, w)).astype(np.float32)
    want = r.apply_device(dev(torch, x))
    torch.cuda.synchronize()
    assert tuple(want.shape) == (n, oh, ow) and want.dtype == torch.float64 and bool(torch.isfinite(want).all())
    if form == "widen_f64":
        gb.assert_same_bits(want, dev(torch, x.astype(np.float64)), what="widen_f64")
    _, xg = gb.poisoned(torch, x, h * w)
    big, out = gb.guarded(torch, (n, oh, ow), torch.float64, oh * ow)
    for rep in range(2):
        if rep:
            gb.refill(big)
        assert r.apply_device(xg, out=out) is out
        torch.cuda.synchronize()
        gb.assert_guards_intact(big, out, what=f"{name} call {rep + 1}")
        gb.assert_fully_written(out, what=f"{name} call {rep + 1}")
        gb.assert_same_bits(out, want, what=f"{name} call {rep + 1}")
    r.close()


# ------------------------------------------------------------------------------------------------ srcfd_prepare_inputs_device
PREPARE = [(10, 10, 10), (7, 13, 9), (13, 7, 32), (32, 32, 32), (1, 1, None)]


@pytest.mark.parametrize("adaptive", [1, 0], ids=["adaptive", "train_stats"])
@pytest.mark.parametrize("h,w,lr", PREPARE, ids=["10x10_to_10", "7x13_to_9", "13x7_to_32", "32x32_to_32", "1x1_as_is"])
def test_prepare_inputs_device(srcfd, torch_, h, w, lr, adaptive):
    """Through ctypes, as tests/test_dropin.py calls it; n = 7.  (32, 32 -> 32): the kernel's LDS arrays exactly full; (1, 1): the
    n < 8 serial-sum branch of the statistics.  One kernel does all of it: there is no second implementation to tell apart.
    Rectangular inputs and lr != h have no history, so x is also compared with Ry @ F @ Rx.T in float64 -- elementwise within
    2^-24 |ref| + (h + w + 2) 2^-53 (|Ry| |F| |Rx|^T) + the smallest float32 subnormal: one float32 rounding and the standard forward
    bound of the two float64 dot-product chains -- and the (mean, std) pairs with numpy's on the device's own float32 field, bit
    for bit (the method of test_batched_call_prepares_its_inputs_on_the_device)."""
    torch = torch_
    L, rs = _mod("_lib"), _mod("resample")
    rng = np.random.default_rng(100 * h + w)
    n, blend = 7, 0.3
    fields = rng.standard_normal((n, h, w)) * rng.uniform(0.1, 30.0, (n, 1, 1)) + rng.standard_normal((n, 1, 1))
    stats = np.stack([rng.standard_normal(n) * 0.2, rng.uniform(0.1, 2.0, n)], 1)
    if lr is None:
        Ry = Rx = None
        oh, ow = h, w
    else:
        Ry, Rx = np.array(rs.interp_matrix(h, 3.0, lr, 10.0)), np.array(rs.interp_matrix(w, 10.0, lr, 10.0))
        assert Ry.shape == (lr, h) and Rx.shape == (lr, w)
        oh = ow = lr
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(f, ry, rx, tr, x, a):
        L.check(L.lib.srcfd_prepare_inputs_device(p(f), n, h, w, p(ry), p(rx), lr or h, p(tr), adaptive, blend, p(x), p(a), None))
        torch.cuda.synchronize()

    # 1. plain tensors
    want_x = torch.empty((n, oh, ow), dtype=torch.float32, device="cuda")
    want_a = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    call(dev(torch, fields), None if Ry is None else dev(torch, Ry), None if Rx is None else dev(torch, Rx), dev(torch, stats), want_x, want_a)
    # 2. guarded outputs, poisoned inputs
    fg = gb.poisoned(torch, fields, h * w)[1]
    tg = gb.poisoned(torch, stats, 2)[1]
    ryg = None if Ry is None else gb.poisoned(torch, Ry, h)[1]
    rxg = None if Rx is None else gb.poisoned(torch, Rx, w)[1]
    big_x, x = gb.guarded(torch, (n, oh, ow), torch.float32, oh * ow)
    big_a, a = gb.guarded(torch, (n, 2), torch.float32, gb.affine_guard())
    call(fg, ryg, rxg, tg, x, a)
    # 3.
    for big, view, want, nm in ((big_x, x, want_x, "x_dev"), (big_a, a, want_a, "in_affine_dev")):
        gb.assert_guards_intact(big, view, what=nm)
        gb.assert_fully_written(view, what=nm)
        gb.assert_same_bits(view, want, what=nm)
    # the value check
    xg, ag = x.cpu().numpy(), a.cpu().numpy()
    ry64, rx64 = (np.eye(h), np.eye(w)) if Ry is None else (Ry, Rx)
    ref = ry64 @ fields @ rx64.T
    bound = 2.0 ** -24 * np.abs(ref) + (h + w + 2) * 2.0 ** -53 * (np.abs(ry64) @ np.abs(fields) @ np.abs(rx64).T) + 2.0 ** -149
    err = np.abs(xg.astype(np.float64) - ref)
    print(f"prepare_inputs ({h}, {w} -> {lr}) adaptive={adaptive}: worst error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), (np.max(err / bound), np.unravel_index(np.argmax(err / bound), err.shape))
    for i in range(n):
        mean_lr, std_lr = float(stats[i, 0]), float(stats[i, 1])
        if adaptive:
            g32 = xg[i]                # statistics of the device's own float32 field
            input_mean, input_std = g32.reshape(1, -1).mean(axis=1)[0], g32.reshape(1, -1).std(axis=1)[0]
            mean_lr = (1 - blend) * mean_lr + blend * input_mean
            std_lr = (1 - blend) * std_lr + blend * max(input_std, 1e-8)
        want = np.array([mean_lr, std_lr], np.float32)
        np.testing.assert_array_equal(ag[i].view(np.uint32), want.view(np.uint32), err_msg=f"sample {i}")


# ------------------------------------------------------------------------------------------------ the trainer
def _guard_trainer(torch, t, p0, prefill_grads):
    """Replaces t.params / grads / m / v / sse by guarded tensors: params = p0, m = v = 0, grads zero or the sentinel, sse 0 or the
    sentinel.  Returns {name: (big, view)}."""
    g = {}
    for name in ("params", "grads", "m", "v"):
        g[name] = gb.guarded(torch, (t.n_params,), torch.float32, gb.FLAT_GUARD)
    g["sse"] = gb.guarded(torch, (1,), torch.float64, 1)
    g["params"][1].copy_(p0)
    g["m"][1].zero_()
    g["v"][1].zero_()
    if not prefill_grads:
        g["grads"][1].zero_()
        g["sse"][1].zero_()
    for name, (_, view) in g.items():
        setattr(t, name, view)
    return g


def _trainer_pattern(torch, t, x, y, what):
    n = x.shape[0]
    p0 = t.params.clone()
    xd, yd = dev(torch, x), dev(torch, y)
    # 1. plain tensors: the accumulating call over zeros, the storing call over garbage, one Adam step
    t.grads.zero_()
    t.sse.zero_()
    t.forward_backward(xd, yd)
    torch.cuda.synchronize()
    want_g, want_sse = t.grads.clone(), t.sse.clone()
    t.grads.fill_(7.0)
    t.sse.fill_(7.0)
    t.forward_backward(xd, yd, overwrite=True)
    torch.cuda.synchronize()
    want_go, want_sseo = t.grads.clone(), t.sse.clone()
    assert bool(torch.isfinite(want_g).all()) and bool(torch.isfinite(want_go).all())
    t.t = 0
    t.apply_adam()
    torch.cuda.synchronize()
    want_p, want_m, want_v = t.params.clone(), t.m.clone(), t.v.clone()
    assert not torch.equal(want_p, p0)
    # 2. guarded; x, y poisoned; params between sentinels (NaNs in front of and behind it)
    xg, yg = gb.poisoned(torch, x, int(np.prod(x.shape[1:])))[1], gb.poisoned(torch, y, int(np.prod(y.shape[1:])))[1]
    for overwrite, wg, ws in ((False, want_g, want_sse), (True, want_go, want_sseo)):
        g = _guard_trainer(torch, t, p0, prefill_grads=overwrite)
        for rep in range(3):        # plain launches, capture, replay
            if rep and not overwrite:
                t.grads.zero_()
                t.sse.zero_()
            elif rep:
                gb.refill(g["grads"][0])
                gb.refill(g["sse"][0])
            t.forward_backward(xg, yg, overwrite=overwrite)
            torch.cuda.synchronize()
            label = f"{what}, {'overwrite' if overwrite else 'accumulate'}, call {rep + 1}"
            for name in ("grads", "sse", "params"):
                gb.assert_guards_intact(*g[name], what=f"{label}: {name}")
            gb.assert_fully_written(t.grads, what=label)
            gb.assert_fully_written(t.sse, what=label)
            gb.assert_same_bits(t.grads, wg, what=f"{label}: grads")
            gb.assert_same_bits(t.sse, ws, what=f"{label}: sse")
            gb.assert_same_bits(t.params, p0, what=f"{label}: params are an input")
        if overwrite:
            t.t = 0
            t.apply_adam()
            torch.cuda.synchronize()
            for name, want in (("params", want_p), ("m", want_m), ("v", want_v), ("grads", wg)):
                gb.assert_guards_intact(*g[name], what=f"{what}: Adam, {name}")
                gb.assert_same_bits(getattr(t, name), want, what=f"{what}: Adam, {name}")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("enc", [1, 0])
@pytest.mark.parametrize("tail", [1, 0])
def test_trainer_sr_network(srcfd, torch_, enc_weights, dec_weights, monkeypatch, tail, enc, n):
    """Graph (a): the SR network, max_batch 8, SRCFD_TRAIN_TAIL x SRCFD_TRAIN_ENC."""
    monkeypatch.setenv("SRCFD_TRAIN_TAIL", str(tail))
    monkeypatch.setenv("SRCFD_TRAIN_ENC", str(enc))
    t = _mod("train").Trainer(srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0), max_batch=8)
    assert t.plan == {"fused_tail": tail, "fused_encoder": enc} and t.n_params == 2_709_491
    rng = np.random.default_rng(10 * n + 2 * tail + enc)
    x = rng.standard_normal((n, 10, 10, 1)).astype(np.float32)
    y = rng.standard_normal((n, 400, 400, 1)).astype(np.float32)
    _trainer_pattern(torch_, t, x, y, f"sr n={n} tail={tail} enc={enc}")
    t.close()


def test_trainer_small_graph(srcfd, torch_):
    """Graph (b): 'convt_3s2' of tests/test_gpu_training_oracle.py's table, 809 parameters (not a multiple of 256), n = 2."""
    from test_gpu_training_oracle import TABLE, out_shape
    specs, in_shape, _, _ = TABLE["convt_3s2"]
    t = _mod("train").Trainer(srcfd.SRModel.from_layers(specs, in_shape, device=0), max_batch=3)
    assert t.plan == {"fused_tail": 0, "fused_encoder": 0} and t.n_params == 809 and t.n_params % 256 != 0
    rng = np.random.default_rng(809)
    x = rng.standard_normal((2,) + tuple(in_shape)).astype(np.float32)
    y = rng.standard_normal((2,) + out_shape(specs, in_shape)).astype(np.float32)
    _trainer_pattern(torch_, t, x, y, "convt_3s2 n=2")
    t.close()


# ------------------------------------------------------------------------------------------------ host destinations (the numpy twin)
def _np_check(big, view, want, what):
    gb.assert_guards_intact(big, view, what=what)
    gb.assert_fully_written(view, what=what)
    gb.assert_same_bits(view, want, what=what)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("memory", ["pageable", "page_locked"])
@pytest.mark.parametrize("n", [3, 130])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_host_predict(srcfd, torch_, enc_weights, dec_weights, precision, n, memory):
    """srcfd_predict into pageable and page-locked memory; 130 samples cross the 128-sample chunk of the page-locked path."""
    L = _mod("_lib")
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = precision
    x = _sr_x(n, seed=7)
    x[0, 5, 5, 0] = np.nan
    ain, aout = _affines(np.random.default_rng(n), n)
    want, count = m.predict(x, in_affine=ain, out_affine=aout, nan_guard=True, return_nonfinite=True, out=np.empty((n, 400, 400, 1), np.float32))
    assert count == 160000
    shape, sample = (n, 400, 400, 1), 160000
    free = None
    if memory == "pageable":
        big, y = gb.guarded(np, shape, np.float32, sample)
    else:
        nbytes = gb.guarded_nbytes(shape, np.float32, sample)
        ptr = C.c_void_p()
        L.check(L.lib.srcfd_host_alloc(nbytes, C.byref(ptr)))
        free = lambda: L.lib.srcfd_host_free(ptr)
        big, y = gb.guarded_in(np, np.frombuffer((C.c_char * nbytes).from_address(ptr.value), dtype=np.uint8), shape, np.float32, sample)
    try:
        xg, aing, aoutg = gb.poisoned(np, x, 100)[1], gb.poisoned(np, ain, gb.affine_guard())[1], gb.poisoned(np, aout, gb.affine_guard())[1]
        bad = np.array([gb.SENTINEL_I64, 5, gb.SENTINEL_I64], np.int64)
        L.check(L.lib.srcfd_predict(m._h, _vp(xg), n, _vp(aing), _vp(aoutg), _vp(y), L.FLAG_NAN_GUARD, bad[1:].ctypes.data_as(C.POINTER(C.c_int64))))
        p = m.last_plan()
        assert p["precision"] == precision and p["encoder"] == ("enc16" if precision == "bf16" else "enc32"), p
        _np_check(big, y, want, f"srcfd_predict {precision} n={n} {memory}")
        assert bad.tolist() == [gb.SENTINEL_I64, count, gb.SENTINEL_I64]     # the host count is set, not added to (include/srcfd.h)
    finally:
        del big, y
        if free:
            free()


def test_host_predict_resampled(srcfd, torch_, enc_weights, dec_weights):
    L, rs = _mod("_lib"), _mod("resample")
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32"
    Ry, Rx = rs.square_to_rect_matrices(400, 37, 23, 10.0, 3.0)
    r = rs.Resampler(np.array(Ry), np.array(Rx), 0)
    x = _sr_x(3, seed=8)
    want = m.predict_resampled(x, r)
    assert want.shape == (3, 23, 37) and np.isfinite(want).all()
    big, y = gb.guarded(np, want.shape, np.float64, 23 * 37)
    xg = gb.poisoned(np, x, 100)[1]
    bad = C.c_int64(0)
    L.check(L.lib.srcfd_predict_resampled(m._h, r._h, _vp(xg), 3, None, None, _vp(y), 0, C.byref(bad)))
    assert m.last_plan()["precision"] == "fp32" and m.last_plan()["encoder"] == "enc32"
    _np_check(big, y, want, "srcfd_predict_resampled")
    r.close()


@pytest.mark.parametrize("resampled", [False, True], ids=["as_is", "resampled"])
def test_host_predict_into_solver_state(srcfd, torch_, enc_weights, dec_weights, resampled):
    rs = _mod("resample")
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32"
    r = None
    if resampled:
        Ry, Rx = rs.square_to_rect_matrices(400, 37, 23, 10.0, 3.0)
        r = rs.Resampler(np.array(Ry), np.array(Rx), 0)
    ny, nx = (23, 37) if resampled else (400, 400)
    x = _sr_x(3, seed=9)
    bt = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 1, 0, 1]], np.int32)
    bv = np.random.default_rng(1).standard_normal((3, 4))
    want = m.predict_into_solver_state(x, bt, bv, resampler=r)
    assert want.shape == (3, nx + 2, ny + 2)
    big, var = gb.guarded(np, want.shape, np.float64, (nx + 2) * (ny + 2))
    got = m.predict_into_solver_state(gb.poisoned(np, x, 100)[1], bt, bv, resampler=r, Var=var)
    assert got is var and m.last_plan()["precision"] == "fp32"
    _np_check(big, var, want, "srcfd_predict_into_solver_state")
    if r is not None:
        r.close()


def test_host_fine_solver_state(srcfd, torch_):
    L, fine = _mod("_lib"), _mod("fine")
    s = fine.FineSolver(fine.problem(100.0, 12, 9))
    assert not s.resident
    s.run(3)
    want = s.Var
    assert want.shape == (3, 14, 11) and np.isfinite(want).all() and want.any()
    big, var = gb.guarded(np, want.shape, np.float64, 14 * 11)
    L.check(L.lib.srcfd_fine_solver_get_state(s._h, _vp(var)))
    _np_check(big, var, want, "srcfd_fine_solver_get_state")
    s.close()


@pytest.mark.parametrize("case", [1, -1])
def test_host_fine_batch_state(srcfd, torch_, case):
    L, fine = _mod("_lib"), _mod("fine")
    b = fine.FineSolverBatch([fine.problem(Re, 12, 9) for Re in (100.0, 200.0, 300.0)])
    assert not b.resident
    b.run(3)
    want = b.Var if case < 0 else b.case_var(case)
    assert want.shape == ((3, 3, 14, 11) if case < 0 else (3, 14, 11)) and np.isfinite(want).all() and want.any()
    big, var = gb.guarded(np, want.shape, np.float64, 3 * 14 * 11)
    L.check(L.lib.srcfd_fine_batch_get_state(b._h, case, _vp(var)))
    _np_check(big, var, want, f"srcfd_fine_batch_get_state case {case}")
    b.close()


def test_host_trainer_params(srcfd, torch_):
    from test_gpu_training_oracle import TABLE
    L = _mod("_lib")
    specs, in_shape, _, _ = TABLE["convt_3s2"]
    t = _mod("train").Trainer(srcfd.SRModel.from_layers(specs, in_shape, device=0), max_batch=2)
    want = t.params.cpu().numpy()          # Trainer.__init__ read them into a plain array
    assert want.size == t.n_params == 809
    np.testing.assert_array_equal(want, np.concatenate([np.concatenate([s["w"].ravel(), s["b"].ravel()]) for s in specs if "w" in s]))
    big, p = gb.guarded(np, (t.n_params,), np.float32, gb.FLAT_GUARD)
    L.check(L.lib.srcfd_trainer_get_params(t._h, _vp(p)))
    _np_check(big, p, want, "srcfd_trainer_get_params")
    t.close()


def test_host_score_fields(srcfd, torch_):
    L, score = _mod("_lib"), _mod("score")
    rng = np.random.default_rng(8193)
    n, elems = 3, 8193
    pred, truth = (rng.standard_normal((n, elems)).astype(np.float32) for _ in range(2))
    pa, ta = _affines(rng, n)
    want = score.score_fields(pred, truth, pa, ta)
    want = np.stack([want[k] for k in L.SCORE_NAMES], 1)
    assert want.shape == (n, 8) and want.dtype == np.float32
    assert score.score_plan(elems)
    big, metrics = gb.guarded(np, (n, L.SCORE_FIELDS), np.float32, L.SCORE_FIELDS)
    predg, truthg = gb.poisoned(np, pred, elems)[1], gb.poisoned(np, truth, elems)[1]
    L.check(L.lib.srcfd_score_fields(0, _vp(predg), _vp(truthg), n, elems, _vp(gb.poisoned(np, pa, gb.affine_guard())[1]),
                                     _vp(gb.poisoned(np, ta, gb.affine_guard())[1]), _vp(metrics)))
    _np_check(big, metrics, want, "srcfd_score_fields")
