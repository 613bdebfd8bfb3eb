"""What a caller hands the device entry points, on an MI355X (include/srcfd.h, "device pointers").

A. Refusals: a table of (entry point, argument, defect).  Every row raises ValueError naming the argument, and after a device
   synchronisation every output of the call still holds the NaN sentinel it was filled with and the counter its start value: the
   refusal came before anything was enqueued.  These rows launch no project kernel.
B. Offset views: every caller tensor `skew` = 1, 2, 3 elements behind a 256-byte boundary (tests/guard_bands.py, skew=), one tensor at
   a time and then all at once.  The outputs are compared bit for bit with the same call on unskewed buffers -- an address does not
   enter any kernel's arithmetic, and the unskewed call is what the parity tests pin to the oracle -- and every guard stays intact.
   Only pointers the audit of DESIGN.md section 7 allows are launched: element alignment is the contract of every entry here.
C. Past one launch: predict_device with cap + 6 samples of the 10 -> 400 model, cap the chunk srcfd_model_workspace reports.

No test here is meant to fault the device; the guards lie inside allocations the test owns."""
import ctypes as C
import importlib
import signal

import numpy as np
import pytest

import guard_bands as gb
from conftest import require_gpu
from test_gpu_parity_bf16 import TOL
from test_gpu_parity_fp32 import TOL_FP32

pytestmark = pytest.mark.gpu
SKEWS = (1, 2, 3)
SAMPLE = 160000


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


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _odt(torch, name):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[name]


_MODELS = {}


def _sr(srcfd, enc_weights, dec_weights):
    if "sr" not in _MODELS:
        _MODELS["sr"] = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
    return _MODELS["sr"]


def _d10(srcfd, enc_weights):
    """encoder_10 + decoder_10: 100 output elements per sample, 200 bytes as a 16-bit type."""
    if "d10" not in _MODELS:
        _MODELS["d10"] = srcfd.SRModel.from_weights(enc_weights, _mod("family").synthetic_decoder_weights(10, seed=30), device=0)
        assert _MODELS["d10"].output_shape == (10, 10, 1)
    return _MODELS["d10"]


def _small_tail_specs():
    """The (6, 7) graph of tests/test_training.py::test_fused_tail_on_other_image_sizes: Conv 3x3 3 -> 64, ConvT 64 -> 32 -> 16 -> 8,
    Conv 8 -> 1; (6, 7, 3) -> (48, 56, 1)."""
    rng = np.random.default_rng(100 + 42)

    def glorot(shape, fan_in, fan_out):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        return rng.uniform(-lim, lim, shape).astype(np.float32)

    specs = [dict(kind="conv2d", name="front", k=3, stride=1, same=True, act="swish", w=glorot((3, 3, 3, 64), 27, 576), b=(0.1 * rng.standard_normal(64)).astype(np.float32))]
    cin = 64
    for i, cout in enumerate((32, 16, 8)):
        specs.append(dict(kind="conv2d_transpose", name=f"up{i}", k=2, stride=2, same=False, act="swish", w=glorot((2, 2, cout, cin), 4 * cin, 4 * cout),
                          b=(0.1 * rng.standard_normal(cout)).astype(np.float32)))
        cin = cout
    specs.append(dict(kind="conv2d", name="out", k=3, stride=1, same=True, act="linear", w=glorot((3, 3, 8, 1), 72, 9), b=np.array([0.05], np.float32)))
    return specs, (6, 7, 3), (48, 56, 1)


def _small_trainer(srcfd):
    specs, in_shape, out_shape = _small_tail_specs()
    m = srcfd.SRModel.from_layers(specs, in_shape, device=0)
    assert m.output_shape == out_shape
    return _mod("train").Trainer(m, max_batch=3)


def _affines(rng, n):
    ain = np.stack([rng.standard_normal(n) * 0.1, rng.uniform(0.5, 2.0, n)], 1).astype(np.float32)
    aout = np.stack([rng.standard_normal(n) * 0.1, rng.uniform(0.05, 0.3, n)], 1).astype(np.float32)
    return ain, aout


def _counter(torch, start, skew=0):
    """(words, the counter as a 1-element view): int64 sentinels around the counter, which sits at word 2 + skew -- 16-byte aligned in a
    fresh allocation for skew 0, 8 bytes behind such a boundary for skew 1."""
    words = [gb.SENTINEL_I64] * (5 + skew)
    words[2 + skew] = start
    t = torch.tensor(words, dtype=torch.int64, device="cuda")
    c = t[2 + skew:3 + skew]
    assert c.data_ptr() % 16 == 8 * (skew % 2)
    return t, c


def _assert_counter(words, skew, expect, what):
    got = [int(v) for v in words.cpu()]
    at = 2 + skew
    assert all(v == gb.SENTINEL_I64 for i, v in enumerate(got) if i != at), f"{what}: a neighbour of the counter was written: {[hex(v) for v in got]}"
    assert got[at] == expect, f"{what}: counter {got[at]}, expected {expect}"


def _untouched(torch, big, what):
    """Every word of a guarded allocation (guards AND payload) still holds its sentinel."""
    fill = {2: gb.SENTINEL16, 4: gb.SENTINEL32, 8: gb.SENTINEL64}[big.element_size()]
    n = int((big != fill).sum())
    assert n == 0, f"{what}: {n} word(s) of an output changed although the call was refused"


# ================================================================================================ A. refusals
def _defect(torch, good, defect):
    """A tensor with exactly one defect, made from a good one."""
    shape = tuple(good.shape)
    if defect == "none":
        return None
    if defect == "cpu":
        return good.cpu()
    if defect == "numpy":
        return good.cpu().numpy()
    if defect == "dtype":
        other = {torch.float32: torch.float64, torch.float64: torch.float32, torch.int64: torch.int32, torch.int32: torch.int64,
                 torch.bfloat16: torch.float64, torch.float16: torch.float64}[good.dtype]
        return good.to(other)
    if defect == "int_dtype":
        return torch.zeros(shape, dtype=torch.int32, device=good.device)
    if defect == "channel_slice":        # the right shape, every k-th element of the memory
        wide = torch.zeros(shape[:-1] + (3 * shape[-1],), dtype=good.dtype, device=good.device)
        t = wide[..., 0:shape[-1]]
    elif defect == "every_other_row":
        t = torch.zeros((2 * shape[0],) + shape[1:], dtype=good.dtype, device=good.device)[::2]
    elif defect == "transposed":
        t = torch.zeros(shape[:-2] + (shape[-1], shape[-2]), dtype=good.dtype, device=good.device).transpose(-1, -2)
    elif defect == "per_sample_shape":
        return torch.zeros(shape[:-1] + (shape[-1] + 1,), dtype=good.dtype, device=good.device)
    elif defect == "undersized":         # one row short
        return torch.zeros((shape[0] - 1,) + shape[1:], dtype=good.dtype, device=good.device)
    elif defect == "empty":
        return torch.zeros((0,), dtype=good.dtype, device=good.device)
    else:
        raise KeyError(defect)
    assert tuple(t.shape) == shape and not t.is_contiguous(), (defect, tuple(t.shape), shape)
    return t


class _Entry:
    """One entry point with good arguments: `args` (name -> tensor), `outputs` (guarded allocations that must stay untouched),
    `counter` ((words, skew, start) or None) and `call(args)`."""


def _entry_predict(torch, srcfd, enc_weights, dec_weights):
    e = _Entry()
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "bf16"          # the precision whose tail stores 16 bytes per lane: an undersized y must never reach it
    n = 3
    ain, aout = _affines(np.random.default_rng(3), n)
    big, y = gb.guarded(torch, (n, 400, 400, 1), torch.float32, SAMPLE)
    words, c = _counter(torch, 7)
    e.args = dict(x=dev(torch, np.random.default_rng(1).standard_normal((n, 10, 10, 1)).astype(np.float32)), y=y, in_affine=dev(torch, ain),
                  out_affine=dev(torch, aout), nonfinite=c)
    e.outputs, e.counter = [big], (words, 0, 7)
    e.call = lambda a: m.predict_device(a["x"], a["y"], a["in_affine"], a["out_affine"], nan_guard=True, nonfinite=a["nonfinite"])
    return e


def _entry_trainer(method):
    def make(torch, srcfd, enc_weights, dec_weights):
        e = _Entry()
        t = _small_trainer(srcfd)
        n = 3
        rng = np.random.default_rng(5)
        bg, t.grads = gb.guarded(torch, (t.n_params,), torch.float32, gb.FLAT_GUARD)
        bs, t.sse = gb.guarded(torch, (1,), torch.float64, 1)
        p0 = t.params.clone()
        e.args = dict(x=dev(torch, rng.standard_normal((n, 6, 7, 3)).astype(np.float32)), y=dev(torch, rng.standard_normal((n, 48, 56, 1)).astype(np.float32)))
        e.outputs, e.counter = [bg, bs], None
        if method == "forward_backward":
            e.call = lambda a: t.forward_backward(a["x"], a["y"], overwrite=True)
        else:
            e.call = lambda a: t.step(a["x"], a["y"])

        def after():
            assert t.t == 0 and torch.equal(t.params, p0) and not bool(t.m.any()) and not bool(t.v.any())
        e.after = after
        e.keep = t
        return e
    return make


def _entry_resampler(torch, srcfd, enc_weights, dec_weights):
    e = _Entry()
    rng = np.random.default_rng(4)
    r = _mod("resample").Resampler(rng.standard_normal((41, 37)), rng.standard_normal((29, 53)), 0)
    big, out = gb.guarded(torch, (2, 41, 29), torch.float64, 41 * 29)
    e.args = dict(x=dev(torch, rng.standard_normal((2, 37, 53)).astype(np.float32)), out=out)
    e.outputs, e.counter = [big], None
    e.call = lambda a: r.apply_device(a["x"], out=a["out"])
    e.keep = r
    return e


def _tiler_model(srcfd):
    if "tile" not in _MODELS:
        spec = [dict(kind="conv2d", name="one", k=1, stride=1, same=True, act="linear", w=np.full((1, 1, 1, 1), 1.5, np.float32), b=np.full(1, 0.25, np.float32))]
        _MODELS["tile"] = srcfd.SRModel.from_layers(spec, (10, 10, 1), device=0)
    return _MODELS["tile"]


def _entry_tiler(method):
    def make(torch, srcfd, enc_weights, dec_weights):
        e = _Entry()
        t = srcfd.Tiler(_tiler_model(srcfd), 2, 3, 3)
        rng = np.random.default_rng(6)
        field = dev(torch, rng.standard_normal((20, 30, 3)).astype(np.float32))
        ain, aout = (dev(torch, a) for a in _affines(rng, 3))
        big, out = gb.guarded(torch, (20, 30, 3), torch.float32, 600)
        words, c = _counter(torch, 7)
        e.outputs, e.counter = [big], (words, 0, 7)
        if method == "run":
            e.args = dict(field=field, out=out, in_affine=ain, out_affine=aout, nonfinite=c)
            e.call = lambda a: t.run(a["field"], a["out"], a["in_affine"], a["out_affine"], nan_guard=True, nonfinite=a["nonfinite"])
        elif method == "cut":
            e.args = dict(field=field, in_affine=ain, out_affine=aout)
            e.call = lambda a: t.cut(a["field"], a["in_affine"], a["out_affine"])
        else:
            e.args = dict(y=dev(torch, rng.standard_normal((18, 10, 10)).astype(np.float32)), out=out,
                          src_index=dev(torch, rng.permutation(18).astype(np.int32)))
            e.call = lambda a: t.stitch(a["y"], a["out"], src_index=a["src_index"])
        e.keep = t
        return e
    return make


ENTRIES = {"predict_device": _entry_predict, "Trainer.forward_backward": _entry_trainer("forward_backward"), "Trainer.step": _entry_trainer("step"),
           "Resampler.apply_device": _entry_resampler, "Tiler.run": _entry_tiler("run"), "Tiler.cut": _entry_tiler("cut"),
           "Tiler.stitch": _entry_tiler("stitch")}
ARGUMENTS = {"predict_device": ("x", "y", "in_affine", "out_affine", "nonfinite"), "Trainer.forward_backward": ("x", "y"), "Trainer.step": ("x", "y"),
             "Resampler.apply_device": ("x", "out"), "Tiler.run": ("field", "out", "in_affine", "out_affine", "nonfinite"),
             "Tiler.cut": ("field", "in_affine", "out_affine"), "Tiler.stitch": ("y", "out", "src_index")}
REFUSALS = [
    ("predict_device", "x", "dtype"), ("predict_device", "x", "channel_slice"), ("predict_device", "x", "per_sample_shape"), ("predict_device", "x", "cpu"),
    ("predict_device", "x", "none"), ("predict_device", "x", "every_other_row"),
    ("predict_device", "y", "undersized"), ("predict_device", "y", "per_sample_shape"), ("predict_device", "y", "int_dtype"),
    ("predict_device", "y", "every_other_row"), ("predict_device", "y", "channel_slice"), ("predict_device", "y", "cpu"),
    ("predict_device", "in_affine", "dtype"), ("predict_device", "in_affine", "undersized"), ("predict_device", "in_affine", "transposed"),
    ("predict_device", "out_affine", "per_sample_shape"), ("predict_device", "out_affine", "channel_slice"), ("predict_device", "out_affine", "cpu"),
    ("predict_device", "nonfinite", "dtype"), ("predict_device", "nonfinite", "empty"), ("predict_device", "nonfinite", "cpu"),
    ("Trainer.forward_backward", "x", "channel_slice"), ("Trainer.forward_backward", "x", "dtype"), ("Trainer.forward_backward", "y", "channel_slice"),
    ("Trainer.forward_backward", "y", "per_sample_shape"), ("Trainer.forward_backward", "y", "undersized"),
    ("Trainer.step", "x", "channel_slice"), ("Trainer.step", "x", "every_other_row"), ("Trainer.step", "x", "cpu"), ("Trainer.step", "y", "dtype"),
    ("Trainer.step", "y", "every_other_row"),
    ("Resampler.apply_device", "x", "dtype"), ("Resampler.apply_device", "x", "transposed"), ("Resampler.apply_device", "x", "per_sample_shape"),
    ("Resampler.apply_device", "out", "dtype"), ("Resampler.apply_device", "out", "undersized"), ("Resampler.apply_device", "out", "every_other_row"),
    ("Tiler.run", "field", "per_sample_shape"), ("Tiler.run", "field", "channel_slice"), ("Tiler.run", "out", "transposed"), ("Tiler.run", "out", "dtype"),
    ("Tiler.run", "in_affine", "dtype"), ("Tiler.run", "out_affine", "undersized"), ("Tiler.run", "nonfinite", "dtype"),
    ("Tiler.cut", "field", "undersized"), ("Tiler.cut", "in_affine", "transposed"), ("Tiler.cut", "out_affine", "cpu"),
    ("Tiler.stitch", "y", "dtype"), ("Tiler.stitch", "y", "every_other_row"), ("Tiler.stitch", "out", "channel_slice"), ("Tiler.stitch", "src_index", "dtype"),
]


def test_the_table_covers_every_argument_of_every_entry_point():
    assert set(ENTRIES) == set(ARGUMENTS)
    seen = {(e, a) for e, a, _ in REFUSALS}
    for entry, names in ARGUMENTS.items():
        for a in names:
            assert (entry, a) in seen, (entry, a)
    for wanted in (("predict_device", "y", "undersized"), ("Trainer.step", "x", "channel_slice"), ("Trainer.forward_backward", "x", "channel_slice"),
                   ("Resampler.apply_device", "x", "dtype")):
        assert wanted in REFUSALS, wanted
    assert len(set(REFUSALS)) == len(REFUSALS)


_ENTRY_CACHE = {}


@pytest.mark.parametrize("entry,arg,defect", REFUSALS, ids=[f"{e}-{a}-{d}" for e, a, d in REFUSALS])
def test_refused_before_anything_is_enqueued(srcfd, torch_, enc_weights, dec_weights, entry, arg, defect):
    torch = torch_
    if entry not in _ENTRY_CACHE:        # a refusal changes nothing, so one set of good arguments serves every row of an entry
        _ENTRY_CACHE[entry] = ENTRIES[entry](torch, srcfd, enc_weights, dec_weights)
    e = _ENTRY_CACHE[entry]
    assert set(e.args) == set(ARGUMENTS[entry])
    args = dict(e.args)
    args[arg] = _defect(torch, e.args[arg], defect)
    with pytest.raises(ValueError, match=rf"^{arg}\b") as err:
        e.call(args)
    print(f"{entry}({arg}: {defect}): {err.value}")
    torch.cuda.synchronize()
    for big in e.outputs:
        _untouched(torch, big, f"{entry}({arg}: {defect})")
    if e.counter:
        words, skew, start = e.counter
        _assert_counter(words, skew, start, f"{entry}({arg}: {defect})")
    if hasattr(e, "after"):
        e.after()


@pytest.mark.parametrize("which", ["hr_dim", "lr_dim"])
def test_batched_pipeline_refuses_a_size_that_is_not_the_models(srcfd, torch_, enc_weights, dec_weights, which):
    """_super_resolution_batch_on_device builds x and y from the caller's lr_dim / hr_dim: an hr_dim of 200 on the 10 -> 400 model gave a
    y a quarter of the size the tail writes.  Refused before the preparation kernel or the forward is enqueued."""
    torch = torch_
    pl = _mod("pipeline")
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32"
    rng = np.random.default_rng(8)
    side = 10 if which == "hr_dim" else 12
    batch = [{c: rng.standard_normal((side, side)) for c in "uvp"} for _ in range(2)]
    stats = {c: (0.1, 1.5) for c in "uvp"}
    lr_dim, hr_dim = (10, 200) if which == "hr_dim" else (12, 400)
    with pytest.raises(ValueError, match=rf"^[xy] .*{which} = ") as err:
        pl._super_resolution_batch_on_device(batch, 2, m, torch.device("cuda", 0), stats, stats, lr_dim, hr_dim, False, 1.0, 1.0, True, 0.3, True)
    print(err.value)
    torch.cuda.synchronize()
    # the legal call still works, and what it returns has the model's size
    if which == "hr_dim":
        out = pl._super_resolution_batch_on_device(batch, 2, m, torch.device("cuda", 0), stats, stats, 10, 400, False, 1.0, 1.0, True, 0.3, True)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (2, 3, 400, 400) and bool(torch.isfinite(out).all())


# ================================================================================================ B. offset views
def _configs(names, skew, counter_name="nonfinite"):
    """One tensor skewed at a time, then all at once; the int64 counter only takes skew 1."""
    out = [{n: (skew if n == one else 0) for n in names} for one in names if not (one == counter_name and skew != 1)]
    out.append({n: (1 if n == counter_name else skew) for n in names})
    return out


def _assert_skewed(t, skew, what):
    assert t.data_ptr() % gb.ALIGN == skew * t.element_size(), (what, t.data_ptr() % gb.ALIGN, skew)


def _predict_with_skews(torch, m, x, out_type, ain, aout, what, expect, singles=("x", "y", "in_affine", "out_affine", "nonfinite")):
    """predict_device with the NaN guard on and the counter starting at 7: once on unskewed guarded buffers (`want`), then for every
    skew with each tensor of `singles` skewed alone (one call) and all five at once (three calls into the same addresses: plain
    launches, capture, replay)."""
    n = x.shape[0]
    x = x.copy()
    x[(0,) + tuple(s // 2 for s in x.shape[1:])] = np.nan     # sample 0 carries one NaN: the guard zero-fills and counts
    odt = _odt(torch, out_type)
    oshape = (n,) + tuple(m.output_shape)
    sample, in_sample = int(np.prod(m.output_shape)), int(np.prod(x.shape[1:]))
    names = ("x", "y", "in_affine", "out_affine", "nonfinite")

    def run(sk, reps, want=None, count=None):
        xg = gb.poisoned(torch, x, in_sample, skew=sk["x"])[1]
        aing = gb.poisoned(torch, ain, gb.affine_guard(), skew=sk["in_affine"])[1]
        aoutg = gb.poisoned(torch, aout, gb.affine_guard(), skew=sk["out_affine"])[1]
        big, out = gb.guarded(torch, oshape, odt, sample, skew=sk["y"])
        words, c = _counter(torch, 7, sk["nonfinite"])
        for t, nm in ((xg, "x"), (aing, "in_affine"), (aoutg, "out_affine"), (out, "y")):
            _assert_skewed(t, sk[nm], nm)
        graphs = []
        for rep in range(reps):
            if rep:
                gb.refill(big)
                words[2 + sk["nonfinite"]] = 7
            m.predict_device(xg, out, aing, aoutg, nan_guard=True, nonfinite=c)
            torch.cuda.synchronize()
            expect(m)
            graphs.append(m.last_plan()["graph"])
            label = f"{what}, skews {sk}, call {rep + 1} ({graphs[-1]})"
            gb.assert_guards_intact(big, out, what=label)
            gb.assert_fully_written(out, what=label)
            if want is not None:
                gb.assert_same_bits(out, want, what=label)
                _assert_counter(words, sk["nonfinite"], 7 + count, label)
        if reps == 3:
            assert graphs == ["eager", "capture", "replay"], (what, sk, graphs)
        return out, int(words[2 + sk["nonfinite"]].item()) - 7

    want, count = run({nm: 0 for nm in names}, 1)
    assert 0 < count <= sample, (what, count)
    for skew in SKEWS:
        cfgs = _configs(names, skew)
        for sk in cfgs[:-1]:
            if [k for k, v in sk.items() if v][0] in singles:
                run(sk, 1, want, count)
        run(cfgs[-1], 3 if n <= 96 else 1, want, count)


def _expect16(kind, tail):
    def expect(m):
        p = m.last_plan()
        assert p["precision"] == kind and p["encoder"] == "enc16" and p["dense_1"] == "dense1_16" and p["middle"] == "mid16_4x64" and p["tail"] == tail, p
    return expect


def _expect32(precision, n, x3=False):
    def expect(m):
        assert m.last_plan()["precision"] == precision, m.last_plan()
        steps = m.f32_steps(n)
        assert steps[0][1] == "enc32" and steps[-1][1] == "tail32", steps
        assert any(k == "x3" for _, k, _ in steps) == x3, steps
    return expect


def _sr_x(n, seed=0):
    return np.random.default_rng(2000 * n + seed).standard_normal((n, 10, 10, 1)).astype(np.float32)


@pytest.mark.parametrize("tail", ["tail16", "tail16s"])
@pytest.mark.parametrize("out_type", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_predict_device_16_bit_on_offset_views(srcfd, torch_, enc_weights, dec_weights, monkeypatch, kind, out_type, tail):
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = kind
    if tail == "tail16s":
        monkeypatch.setenv("SRCFD_TAIL", "s")
    ain, aout = _affines(np.random.default_rng(3), 3)
    _predict_with_skews(torch_, m, _sr_x(3), out_type, ain, aout, f"{kind} -> {out_type}, {tail}", _expect16(kind, tail))


@pytest.mark.parametrize("out_type", ["f32", "bf16", "f16"])
def test_predict_device_fp32_on_offset_views(srcfd, torch_, enc_weights, dec_weights, out_type):
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32"
    ain, aout = _affines(np.random.default_rng(3), 3)
    _predict_with_skews(torch_, m, _sr_x(3), out_type, ain, aout, f"fp32 -> {out_type}", _expect32("fp32", 3))


def test_predict_device_fp32x3_on_offset_views(srcfd, torch_, enc_weights, dec_weights):
    """65 samples: one past the count from which the split-bf16 kernels take over."""
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = "fp32x3"
    ain, aout = _affines(np.random.default_rng(65), 65)
    _predict_with_skews(torch_, m, _sr_x(65), "f32", ain, aout, "fp32x3, n=65", _expect32("fp32x3", 65, x3=True), singles=("x", "y"))


@pytest.mark.parametrize("precision", ["bf16", "f16", "fp32"])
def test_decoder_10_f16_rows_of_200_bytes(srcfd, torch_, enc_weights, precision):
    """encoder_10 + decoder_10 with float16 output: a sample is 200 bytes, so `y[1:]` of a fresh (8, 10, 10, 1) tensor starts 200 bytes
    behind the allocation -- 8-byte aligned, no more -- and every later row alternates between 8 and 16."""
    torch = torch_
    m = _d10(srcfd, enc_weights)
    m.precision = precision
    n = 7
    x = _sr_x(n, seed=10)
    ain, aout = _affines(np.random.default_rng(7), n)
    xd, aind, aoutd = dev(torch, x), dev(torch, ain), dev(torch, aout)
    want = torch.empty((n, 10, 10, 1), dtype=torch.float16, device="cuda")
    m.predict_device(xd, want, aind, aoutd)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all())
    # the very call: a row slice of a plain tensor
    full = torch.full((n + 1, 10, 10, 1), float("nan"), dtype=torch.float16, device="cuda")
    view = full[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    m.predict_device(xd, view, aind, aoutd)
    torch.cuda.synchronize()
    gb.assert_same_bits(view, want, what=f"decoder_10 {precision}: y[1:]")
    assert bool(torch.isnan(full[0]).all()), "row 0 is not part of y[1:]"
    # and between guards, at one sample (100 elements) and at 1, 2, 3 elements behind a 256-byte boundary
    for skew in (100,) + SKEWS:
        big, out = gb.guarded(torch, (n, 10, 10, 1), torch.float16, 100, skew=skew)
        _assert_skewed(out, skew, "y")
        for rep in range(3):
            if rep:
                gb.refill(big)
            m.predict_device(xd, out, aind, aoutd)
            torch.cuda.synchronize()
            label = f"decoder_10 {precision}: y {2 * skew} bytes behind a boundary, call {rep + 1}"
            gb.assert_guards_intact(big, out, what=label)
            gb.assert_fully_written(out, what=label)
            gb.assert_same_bits(out, want, what=label)


# ------------------------------------------------------------------------------------------------ the trainer
def _train_with_skews(torch, t, x, y, what, expect_kernel_arm):
    """Three identical steps (plain launches, capture, replay) on aligned tensors, then the same three from the same start with x, y
    and the trainer's own arrays 1, 2, 3 elements behind a 256-byte boundary: losses, gradients, parameters and moments bit for bit."""
    n = x.shape[0]
    p0 = t.params.clone()
    names = ("x", "y", "params", "grads", "m", "v", "sse")

    sets = {}     # the trainer's own arrays per skew: the x-only and y-only runs reuse the unskewed set, so their steps replay its graph

    def run(sk):
        key = tuple(sk[nm] for nm in ("params", "grads", "m", "v", "sse"))
        if key not in sets:
            sets[key] = {nm: gb.guarded(torch, (t.n_params,), torch.float32, gb.FLAT_GUARD, skew=sk[nm]) for nm in ("params", "grads", "m", "v")}
            sets[key]["sse"] = gb.guarded(torch, (1,), torch.float64, 1, skew=sk["sse"])
        own = sets[key]
        for nm in ("grads", "sse"):
            gb.refill(own[nm][0])
        own["params"][1].copy_(p0)
        own["m"][1].zero_()
        own["v"][1].zero_()
        for nm, (_, view) in own.items():
            setattr(t, nm, view)
            _assert_skewed(view, sk[nm], nm)
        t.t = 0
        xg = gb.poisoned(torch, x, int(np.prod(x.shape[1:])), skew=sk["x"])[1]
        yg = gb.poisoned(torch, y, int(np.prod(y.shape[1:])), skew=sk["y"])[1]
        _assert_skewed(xg, sk["x"], "x")
        _assert_skewed(yg, sk["y"], "y")
        # which staging arm csrc/train.hip takes for these pointers and sizes: the 16-byte kernel or the two copies
        kernel_arm = (xg.data_ptr() | yg.data_ptr()) % 16 == 0 and xg.numel() % 4 == 0 and yg.numel() % 4 == 0
        trace = []
        for step in range(3):
            loss = t.step(xg, yg)
            torch.cuda.synchronize()
            label = f"{what}, skews {sk}, step {step + 1}"
            for nm in own:
                gb.assert_guards_intact(*own[nm], what=f"{label}: {nm}")
            gb.assert_fully_written(t.grads, what=label)
            assert np.isfinite(loss), label
            trace.append((loss, t.grads.clone(), t.params.clone(), t.m.clone(), t.v.clone(), t.sse.clone()))
        return trace, kernel_arm

    base, arm = run({nm: 0 for nm in names})
    assert arm == expect_kernel_arm, what
    assert base[0][0] != base[1][0] and not torch.equal(base[0][2], p0)       # the steps do train
    for skew in SKEWS:
        for sk in _configs(("x", "y"), skew, counter_name=None)[:2] + [{nm: (1 if nm == "sse" else skew) for nm in names}]:
            sk = {nm: sk.get(nm, 0) for nm in names}
            got, arm = run(sk)
            if sk["x"] or sk["y"]:
                assert not arm, "an x or y off a 16-byte boundary goes through the two copies"
            for step, (g, b) in enumerate(zip(got, base)):
                label = f"{what}, skews {sk}, step {step + 1}"
                assert g[0] == b[0], (label, g[0], b[0])
                for i, nm in enumerate(("grads", "params", "m", "v", "sse"), 1):
                    gb.assert_same_bits(g[i], b[i], what=f"{label}: {nm}")


def test_trainer_step_small_graph_on_offset_views(srcfd, torch_):
    t = _small_trainer(srcfd)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3, 6, 7, 3)).astype(np.float32)
    y = rng.standard_normal((3, 48, 56, 1)).astype(np.float32)
    assert x.size % 4 != 0          # 378 floats: this graph's x never takes the 16-byte staging kernel
    _train_with_skews(torch_, t, x, y, "small graph n=3", expect_kernel_arm=False)
    t.close()


def test_trainer_step_sr_network_on_offset_views(srcfd, torch_, enc_weights, dec_weights):
    """Aligned: the staging kernel's 16-byte copies; off a 16-byte boundary: the two hipMemcpyAsync of the launcher's other arm."""
    t = _mod("train").Trainer(srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0), max_batch=8)
    rng = np.random.default_rng(12)
    x = rng.standard_normal((3, 10, 10, 1)).astype(np.float32)
    y = rng.standard_normal((3, 400, 400, 1)).astype(np.float32)
    _train_with_skews(torch_, t, x, y, "sr n=3", expect_kernel_arm=True)
    t.close()


def test_adam_step_on_offset_views(srcfd, torch_):
    """srcfd_adam_step on 809 parameters (three full workgroups and 41 lanes of a fourth), all four arrays skewed."""
    torch = torch_
    L = _mod("_lib")
    n = 809
    rng = np.random.default_rng(809)
    init = {nm: rng.standard_normal(n).astype(np.float32) for nm in ("params", "grads", "m")}
    init["v"] = rng.uniform(0.0, 1.0, n).astype(np.float32)

    def run(skews):
        own = {}
        for nm in ("params", "grads", "m", "v"):
            own[nm] = gb.guarded(torch, (n,), torch.float32, gb.FLAT_GUARD, skew=skews[nm])
            own[nm][1].copy_(dev(torch, init[nm]))
            _assert_skewed(own[nm][1], skews[nm], nm)
        p = lambda nm: L.device_ptr(own[nm][1], nm, torch.float32, (n,), 0, exact=True)
        for step in (1, 2):
            L.check(L.lib.srcfd_adam_step(p("params"), p("grads"), p("m"), p("v"), n, step, C.c_float(1e-3), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-7), None))
        torch.cuda.synchronize()
        for nm in own:
            gb.assert_guards_intact(*own[nm], what=f"adam {skews}: {nm}")
        return {nm: own[nm][1].clone() for nm in own}

    names = ("params", "grads", "m", "v")
    want = run({nm: 0 for nm in names})
    assert not torch.equal(want["params"], dev(torch, init["params"])) and torch.equal(want["grads"], dev(torch, init["grads"]))
    for skew in SKEWS:
        for sk in _configs(names, skew, counter_name=None):
            got = run(sk)
            for nm in names:
                gb.assert_same_bits(got[nm], want[nm], what=f"adam {sk}: {nm}")


# ------------------------------------------------------------------------------------------------ the resampler and the preparation
def test_resampler_on_offset_views(srcfd, torch_):
    """37 x 53 -> 41 x 29, n = 2: against the float64 einsum at the bar of tests/test_resample.py, and bit for bit with the aligned call."""
    torch = torch_
    rng = np.random.default_rng(4)
    Ry, Rx = rng.standard_normal((41, 37)), rng.standard_normal((29, 53))
    g = rng.standard_normal((2, 37, 53)).astype(np.float32)
    ref = np.einsum("oh,zhw,pw->zop", Ry, g.astype(np.float64), Rx)
    r = _mod("resample").Resampler(Ry, Rx, 0)
    want = r.apply_device(dev(torch, g))
    torch.cuda.synchronize()
    assert np.abs(want.cpu().numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
    for skew in SKEWS:
        for sk in _configs(("x", "out"), skew, counter_name=None):
            xg = gb.poisoned(torch, g, 37 * 53, skew=sk["x"])[1]
            big, out = gb.guarded(torch, (2, 41, 29), torch.float64, 41 * 29, skew=sk["out"])
            _assert_skewed(xg, sk["x"], "x")
            _assert_skewed(out, sk["out"], "out")
            assert r.apply_device(xg, out=out) is out
            torch.cuda.synchronize()
            label = f"resampler, skews {sk}"
            gb.assert_guards_intact(big, out, what=label)
            gb.assert_fully_written(out, what=label)
            gb.assert_same_bits(out, want, what=label)
            err = np.abs(out.cpu().numpy() - ref).max()
            assert err <= 1e-12 * np.abs(ref).max(), (label, err)
    r.close()


@pytest.mark.parametrize("resampled", [True, False], ids=["resampled", "as_is"])
def test_prepare_inputs_on_offset_views(srcfd, torch_, resampled):
    """srcfd_prepare_inputs_device, h = w = 12 (144 elements: the pairwise sum of the statistics splits), 3 samples."""
    torch = torch_
    L, rs = _mod("_lib"), _mod("resample")
    n, h, w, lr = 3, 12, 12, 10
    rng = np.random.default_rng(12)
    data = {"fields": rng.standard_normal((n, h, w)) * 3.0 + 0.5, "train_stats": np.stack([rng.standard_normal(n) * 0.2, rng.uniform(0.1, 2.0, n)], 1)}
    side = h
    if resampled:
        data["Ry"], data["Rx"] = np.array(rs.interp_matrix(h, 3.0, lr, 10.0)), np.array(rs.interp_matrix(w, 10.0, lr, 10.0))
        side = lr
    names = tuple(data) + ("x", "in_affine")

    def run(sk):
        ins = {nm: gb.poisoned(torch, a, int(np.prod(a.shape[1:])), skew=sk[nm])[1] for nm, a in data.items()}
        bx, x = gb.guarded(torch, (n, side, side), torch.float32, side * side, skew=sk["x"])
        ba, a = gb.guarded(torch, (n, 2), torch.float32, gb.affine_guard(), skew=sk["in_affine"])
        for nm, t in list(ins.items()) + [("x", x), ("in_affine", a)]:
            _assert_skewed(t, sk[nm], nm)
        p = lambda nm: L.device_ptr(ins.get(nm), nm, torch.float64, None, 0, optional=True)
        L.check(L.lib.srcfd_prepare_inputs_device(p("fields"), n, h, w, p("Ry"), p("Rx"), side, p("train_stats"), 1, 0.3,
                                                  L.device_ptr(x, "x", torch.float32, (n, side, side), 0),
                                                  L.device_ptr(a, "in_affine", torch.float32, (n, 2), 0, exact=True), None))
        torch.cuda.synchronize()
        for big, view, nm in ((bx, x, "x"), (ba, a, "in_affine")):
            gb.assert_guards_intact(big, view, what=f"prepare {sk}: {nm}")
            gb.assert_fully_written(view, what=f"prepare {sk}: {nm}")
        return x.clone(), a.clone()

    want = run({nm: 0 for nm in names})
    assert bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[1]).all())
    for skew in SKEWS:
        for sk in _configs(names, skew, counter_name=None):
            got = run(sk)
            gb.assert_same_bits(got[0], want[0], what=f"prepare {sk}: x")
            gb.assert_same_bits(got[1], want[1], what=f"prepare {sk}: in_affine")


# ------------------------------------------------------------------------------------------------ the tiler
def test_tiler_on_offset_views(srcfd, torch_):
    """cut, stitch and run of a 2 x 3 x 3 field of 10 x 10 tiles.  The stitch picks its vector width from the alignment its two pointers
    share (tiles.hip, pointer_align): `plan(align_bytes)` for the alignment of the pointers handed in names the width that ran."""
    torch = torch_
    ty, tx, c = 2, 3, 3
    t = srcfd.Tiler(_tiler_model(srcfd), ty, tx, c)
    rng = np.random.default_rng(23)
    field = rng.standard_normal((20, 30, c)).astype(np.float32)
    ain, aout = _affines(rng, c)
    assert t.plan()["v"] == 2 and t.plan(align_bytes=4)["v"] == 1 and t.plan(align_bytes=8)["v"] == 2        # hw = 10: two floats at most

    def common_align(*ts):
        bits = 16
        for q in ts:
            bits |= q.data_ptr()
        return bits & -bits

    # cut
    want_x, want_in, want_out = t.cut(dev(torch, field), dev(torch, ain), dev(torch, aout))
    torch.cuda.synchronize()
    for skew in SKEWS:
        for sk in _configs(("field", "in_affine", "out_affine"), skew, counter_name=None):
            fg = gb.poisoned(torch, field, 30 * c, skew=sk["field"])[1]
            ag = gb.poisoned(torch, ain, gb.affine_guard(), skew=sk["in_affine"])[1]
            og = gb.poisoned(torch, aout, gb.affine_guard(), skew=sk["out_affine"])[1]
            _assert_skewed(fg, sk["field"], "field")
            x, a_in, a_out = t.cut(fg, ag, og)
            torch.cuda.synchronize()
            for got, want, nm in ((x, want_x, "x"), (a_in, want_in, "in_affine rows"), (a_out, want_out, "out_affine rows")):
                gb.assert_same_bits(got, want, what=f"cut, skews {sk}: {nm}")
    # stitch: y and out
    y = rng.standard_normal((ty * tx * c, 10, 10)).astype(np.float32)
    want = torch.empty((20, 30, c), dtype=torch.float32, device="cuda")
    t.stitch(dev(torch, y), want)
    torch.cuda.synchronize()
    for skew in SKEWS:
        for sk in _configs(("y", "out"), skew, counter_name=None):
            yg = gb.poisoned(torch, y, 100, skew=sk["y"])[1]
            big, out = gb.guarded(torch, (20, 30, c), torch.float32, 30 * c, skew=sk["out"])
            _assert_skewed(yg, sk["y"], "y")
            _assert_skewed(out, sk["out"], "out")
            v = t.plan(align_bytes=common_align(yg, out))["v"]
            assert v == (1 if skew % 2 else 2), (sk, v)
            t.stitch(yg, out)
            torch.cuda.synchronize()
            label = f"stitch, skews {sk} (v = {v})"
            gb.assert_guards_intact(big, out, what=label)
            gb.assert_fully_written(out, what=label)
            gb.assert_same_bits(out, want, what=label)
    # run: field, out, both affines and the counter
    fnan = field.copy()
    fnan[3, 4, 1] = np.nan
    names = ("field", "out", "in_affine", "out_affine", "nonfinite")

    def run(sk):
        fg = gb.poisoned(torch, fnan, 30 * c, skew=sk["field"])[1]
        ag = gb.poisoned(torch, ain, gb.affine_guard(), skew=sk["in_affine"])[1]
        og = gb.poisoned(torch, aout, gb.affine_guard(), skew=sk["out_affine"])[1]
        big, out = gb.guarded(torch, (20, 30, c), torch.float32, 30 * c, skew=sk["out"])
        words, cnt = _counter(torch, 7, sk["nonfinite"])
        t.run(fg, out, ag, og, nan_guard=True, nonfinite=cnt)
        torch.cuda.synchronize()
        label = f"run, skews {sk}"
        gb.assert_guards_intact(big, out, what=label)
        gb.assert_fully_written(out, what=label)
        _assert_counter(words, sk["nonfinite"], 7 + 1, label)         # the model is pointwise: one NaN in, one element zero-filled
        return out.clone()

    want = run({nm: 0 for nm in names})
    assert bool(torch.isfinite(want).all()) and float(want[3, 4, 1]) == 0.0 and int((want == 0).sum()) == 1
    for skew in SKEWS:
        for sk in _configs(names, skew):
            gb.assert_same_bits(run(sk), want, what=f"run, skews {sk}")
    t.close()


# ================================================================================================ C. past one launch
_TAIL = {}


def _tail_rows(oracle, enc_weights, dec_weights):
    """The six samples behind the chunk boundary (the same for every precision, whatever its chunk) with their affines, and the float64
    oracle of the first and the last of them in standardised space."""
    if not _TAIL:
        rng = np.random.default_rng(606)
        x = rng.standard_normal((6, 10, 10, 1)).astype(np.float32)
        ain, aout = _affines(rng, 6)
        xs = (x[[0, 5]].astype(np.float64) - ain[[0, 5], 0].reshape(2, 1, 1, 1)) / ain[[0, 5], 1].reshape(2, 1, 1, 1)
        _TAIL.update(x=x, ain=ain, aout=aout, ref=oracle.superres_forward(xs, enc_weights, dec_weights, np.float64))
    return _TAIL


@pytest.mark.parametrize("precision", ["bf16", "f16", "fp32"])
def test_predict_device_past_one_launch(srcfd, torch_, oracle, enc_weights, dec_weights, precision):
    """n = cap + 6 on the 10 -> 400 model: the chunk loop's second pass starts at x + cap * 100, y + cap * 160000, affine row cap, and
    adds to the counter the first pass left.  Every affine row is different, so a chunk that restarts its rows at 0 changes bits."""
    torch = torch_
    L = _mod("_lib")
    m = _sr(srcfd, enc_weights, dec_weights)
    m.precision = precision
    cap = L.check(L.lib.srcfd_model_workspace(m._h, 2048, None))
    assert 150 < cap <= 1024, cap
    if precision != "fp32":
        assert cap == 1024, cap     # the 16-bit forward cuts at 1024 samples (fused_bf16.hip, lowp16_chunk_cap): cap + 6 must cross THAT cut
    n = cap + 6
    tail = _tail_rows(oracle, enc_weights, dec_weights)
    rng = np.random.default_rng(cap)
    x = np.concatenate([rng.standard_normal((cap, 10, 10, 1)).astype(np.float32), tail["x"]])
    head_in, head_out = _affines(rng, cap)
    ain, aout = np.concatenate([head_in, tail["ain"]]), np.concatenate([head_out, tail["aout"]])
    assert len({a.tobytes() for a in ain}) == n and len({a.tobytes() for a in aout}) == n and len({s.tobytes() for s in x}) == n
    bad_rows = (17, cap + 2)
    for r in bad_rows:
        x[r, 4, 5, 0] = np.nan
    xd, aind, aoutd = dev(torch, x), dev(torch, ain), dev(torch, aout)

    def call(lo, hi):
        y = torch.full((hi - lo, 400, 400, 1), float("nan"), dtype=torch.float32, device="cuda")
        words, c = _counter(torch, 7)
        m.predict_device(xd[lo:hi], y, aind[lo:hi], aoutd[lo:hi], nan_guard=True, nonfinite=c)
        torch.cuda.synchronize()
        p = m.last_plan()
        assert p["precision"] == precision, p
        if precision != "fp32":
            assert p["encoder"] == "enc16" and p["dense_1"] == "dense1_16" and p["middle"].startswith("mid16") and p["tail"] == "tail16", p
        return y, words

    y, words = call(0, n)
    _assert_counter(words, 0, 7 + 2 * SAMPLE, f"{precision}: n = {n}")
    for r in bad_rows:
        assert not bool(y[r].any()), f"row {r} carried a NaN: zero-filled"
    y_head, words = call(0, cap)
    _assert_counter(words, 0, 7 + SAMPLE, f"{precision}: the first {cap}")
    assert torch.equal(y[:cap], y_head), f"{precision}: rows [0, {cap}) differ from a {cap}-sample call of the same rows and affines"
    del y_head
    y_tail, words = call(cap, n)
    _assert_counter(words, 0, 7 + SAMPLE, f"{precision}: the last 6")
    assert torch.equal(y[cap:], y_tail), f"{precision}: rows [{cap}, {n}) differ from a 6-sample call of the same rows and affines"
    assert bool(torch.isfinite(y).all())
    # rows cap and cap + 5 against the float64 oracle, in standardised space, at the bars of the parity tests
    rows = [cap, cap + 5]
    got = y[rows].cpu().numpy().astype(np.float64)
    got = (got - aout[rows, 0].reshape(2, 1, 1, 1)) / aout[rows, 1].reshape(2, 1, 1, 1)
    err = oracle.rel_l2(got, tail["ref"])
    tol = TOL_FP32 if precision == "fp32" else TOL[precision][1]
    print(f"{precision}: cap {cap}, rows {rows} vs the float64 oracle: rel L2 {err:.3e} (bar {tol:g})")
    assert err <= tol, (precision, err, tol)
