"""SRCFD_FLAG_NAN_GUARD held to numpy element by element on PARTLY bad fields, in every kernel that finishes an output
(the fast and the seam epilogue of tail16 and of tail16s, tail32 plain and split-operand, conv_n1_tile_f32<FIN>, finalize_out,
outconv16), on an MI355X.  The recipe, the reference and the planted defects: tests/guard_cases.py (CPU part:
test_guard_cases.py).

For one handle, one batch and one output type an arm makes three device calls,

    acc     no affine, no guard, float32 output      (the parity modules pin this result to the oracle)
    y_off   the affine trigger, guard off
    y_on    the affine trigger, guard on, a counter that starts at 7   (and once more without a counter)

and asserts, on integer views and without a tolerance: y_off == cast(affine_ref(acc)), infinities included; y_on ==
guard_ref(affine_ref(acc)); the counter reads 7 + the reference count; y_on is finite in its own type.  No tolerance is needed
because acc IS the kernel's value in front of the affine (std = 1, mean = 0 leave it unchanged), the affine is one fma or two
float32 roundings that numpy restates exactly, and the cast is round-to-nearest-even on both sides.  std comes from a quantile of
the device's own acc: an input choice; the share of bad elements and the coverage conditions of guard_cases.coverage are then
ASSERTED on the device's pattern, so a trigger that degenerated fails the arm.

Every arm asserts the kernel that finished the output (last_plan() / f32_steps()).
"""
import importlib

import numpy as np
import pytest

import error_maps as em
import guard_cases as gc
from conftest import STATS_TXT, require_gpu

pytestmark = pytest.mark.gpu
HW = gc.H * gc.W


@pytest.fixture(scope="module")
def torch_(srcfd):
    require_gpu(srcfd)
    import torch
    return torch


@pytest.fixture(scope="module")
def x3(srcfd, coarse_cases):
    x = em.fixed_batch(coarse_cases, srcfd.load_stats(STATS_TXT, 10, 400)[0], 3)
    x.setflags(write=False)
    return x


_MODELS = {}


def sr_model(srcfd, enc_weights, dec_weights, precision):
    """One handle per precision for the whole module (the switches are read on every call)."""
    if precision not in _MODELS:
        m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
        m.precision = precision
        _MODELS[precision] = m
    return _MODELS[precision]


def cycled(x3, n):
    return np.ascontiguousarray(x3[np.arange(n) % 3])


def tdtype(torch, out_dtype):
    return {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}[out_dtype]


def host(torch, t, out_dtype):
    """A device result in the representation of guard_cases (bfloat16: its uint16 bit pattern)."""
    if out_dtype == "bfloat16":
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Arm:
    """One handle, one batch: `acc` once, then the two triggered calls per output type and layout."""

    def __init__(self, torch, m, x, precision, label):
        self.torch, self.m, self.x, self.precision, self.label = torch, m, np.ascontiguousarray(x, np.float32), precision, label
        self.n = x.shape[0]
        self.oshape = (self.n,) + tuple(m.output_shape)
        self.xd = dev(torch, self.x)
        acc = torch.empty(self.oshape, dtype=torch.float32, device="cuda")
        m.predict_device(self.xd, acc)
        torch.cuda.synchronize()
        self.acc = acc.cpu().numpy()
        self.plan = m.last_plan()

    def rows(self, out_dtype, triggered, first=0, cycle=True):
        """(n, 2): the samples of `triggered` take the recipe's rows on the device's own acc, every other sample (mean, std) = (0, 1).
        cycle=False: every triggered sample takes ROWS[0] (Q = 0.90, mean 0) -- the small fields, where 3 % is a handful of values."""
        aout = np.tile(np.array([0.0, 1.0], np.float32), (self.n, 1))
        for j, i in enumerate(triggered):
            aout[i] = gc.trigger_rows(self.acc[i:i + 1], out_dtype, first=(first + j + j // 3) if cycle else 0)[0]
        return aout

    def check(self, out_dtype, triggered=None, first=0, full=True):
        """The three-call comparison.  triggered: the samples that take a trigger row (default: all).  full: the output is
        400 x 400 x 1 and the pattern must meet every condition of guard_cases.coverage.  -> (reference count, y_on, aout)."""
        torch, m, n = self.torch, self.m, self.n
        what = f"{self.label} -> {out_dtype}"
        triggered = list(range(n)) if triggered is None else list(triggered)
        aout = self.rows(out_dtype, triggered, first, cycle=full)
        ad = dev(torch, aout)
        dt = tdtype(torch, out_dtype)
        y_off, y_on, y_on2 = (torch.empty(self.oshape, dtype=dt, device="cuda") for _ in range(3))
        counter = torch.full((1,), gc.START, dtype=torch.int64, device="cuda")
        m.predict_device(self.xd, y_off, out_affine=ad)
        m.predict_device(self.xd, y_on, out_affine=ad, nan_guard=True, nonfinite=counter)
        m.predict_device(self.xd, y_on2, out_affine=ad, nan_guard=True, nonfinite=None)
        torch.cuda.synchronize()
        got_off, got_on, got_on2 = (host(torch, t, out_dtype) for t in (y_off, y_on, y_on2))
        v = gc.affine_ref(self.acc, aout, self.precision)
        want_off = gc.cast(v, out_dtype)
        want_on, count = gc.guard_ref(v, out_dtype)
        # the device's pattern: is it the partly bad field the arm is about?
        f_off = gc.to_f32(got_off, out_dtype)
        bad = ~np.isfinite(f_off)
        share = bad.reshape(n, -1).mean(1)
        print(f"{what}: n = {n}, bad share per triggered sample {np.array2string(share[triggered], precision=4)}, reference count {count}, "
              f"counter {int(counter.item())}, finite in float32 but not in y's type {int((np.isfinite(v) & ~gc.finite(want_off, out_dtype)).sum())}")
        assert np.all((share[triggered] >= gc.SHARE[0]) & (share[triggered] <= gc.SHARE[1])), f"{what}: the trigger degenerated, shares {share}"
        if full:
            t = np.asarray(triggered)
            adjacent = t if np.all(np.diff(t) == 1) else t[:1]     # the sample-seam condition is about neighbours in the batch
            cov, _ = gc.coverage(bad[adjacent, :, :, 0], (f_off == np.inf)[adjacent, :, :, 0], (f_off == -np.inf)[adjacent, :, :, 0])
            assert all(cov.values()), f"{what}: the device's pattern misses {[k for k, ok in cov.items() if not ok]}"
        else:
            assert bad.any() and not bad.all()
        # the assertions
        off_ok = gc.same_bits(got_off, want_off, out_dtype)
        assert off_ok.all(), f"{what}: guard off, {int((~off_ok).sum())} elements differ from cast(affine_ref(acc)), first at {np.argwhere(~off_ok)[:4].tolist()}"
        on_ok = gc.bits(got_on) == gc.bits(want_on)
        assert on_ok.all(), (f"{what}: guard on, {int((~on_ok).sum())} elements differ from guard_ref ({int((~gc.finite(got_on, out_dtype)).sum())} "
                             f"of y_on are not finite), first at {np.argwhere(~on_ok)[:4].tolist()}")
        assert int(counter.item()) == gc.START + count, f"{what}: counter {int(counter.item())}, want {gc.START} + {count}"
        assert gc.finite(got_on, out_dtype).all(), what
        np.testing.assert_array_equal(gc.bits(got_on2), gc.bits(got_on), err_msg=f"{what}: nonfinite=None")
        return count, got_on, aout

    def check_mixed(self, out_dtype):
        """Layout B on a batch of >= 3 whose sample 2 has a NaN input: sample 0 triggered, sample 1 with std = 1 keeps the bits of
        acc and adds nothing, sample 2 adds exactly H W."""
        assert self.n >= 3 and np.isnan(self.acc[2]).all() and np.isfinite(self.acc[:2]).all(), self.label
        count, got_on, _ = self.check(out_dtype, triggered=[0])
        per = np.prod(self.oshape[1:])
        c0 = gc.guard_ref(gc.affine_ref(self.acc[:1], self.rows(out_dtype, [0])[:1], self.precision), out_dtype)[1]
        assert count == c0 + per, (self.label, out_dtype, count, c0)
        np.testing.assert_array_equal(gc.bits(got_on[1]), gc.bits(gc.cast(self.acc[1], out_dtype)), err_msg=f"{self.label} -> {out_dtype}: std = 1")
        assert not gc.bits(got_on[2]).any()


def with_nan_input(x):
    x = np.array(x, np.float32)
    x[2, 3, 3, 0] = np.nan       # through the dense layers: every value of sample 2
    return x


def set_env(monkeypatch, env):
    for k in ("SRCFD_TAIL", "SRCFD_TAIL_SEG", "SRCFD_NO_TAIL32"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------------------------------
# the two 16-bit tails
# ------------------------------------------------------------------------------------------------------------------------
TAILS = {"tail16": {}, "tail16s": {"SRCFD_TAIL": "s"}}


def _ran_tail(arm, tail, seg):
    assert arm.plan["tail"] == tail and arm.plan["precision"] == arm.precision, arm.plan
    if seg is not None:
        assert arm.plan["tail_seg"] == seg, arm.plan
    return arm.plan["tail_seg"]


@pytest.mark.parametrize("seg", [None, "1", "5", "25"], ids=["seg_auto", "seg_1", "seg_5", "seg_25"])
@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_tail16_partly_bad_fields(srcfd, torch_, enc_weights, dec_weights, x3, kind, tail, seg, monkeypatch):
    """n = 1 and n = 3 (three triggered samples: both sides of two sample seams), then the mixed batch (triggered | std = 1 | NaN
    input), three output types each.  Under SRCFD_TAIL_SEG = 5 / 25 the segments' first row pairs go through the seam epilogue."""
    m = sr_model(srcfd, enc_weights, dec_weights, kind)
    set_env(monkeypatch, dict(TAILS[tail], **({"SRCFD_TAIL_SEG": seg} if seg else {})))
    for x, mixed in ((x3[:1], False), (x3, False), (with_nan_input(x3), True)):
        arm = Arm(torch_, m, x, kind, f"{kind} {tail} seg {seg or 'auto'} n = {len(x)}{' mixed' if mixed else ''}")
        ran = _ran_tail(arm, tail, seg)
        for out_dtype in gc.OUT_DTYPES:
            if mixed:
                arm.check_mixed(out_dtype)
            else:
                arm.check(out_dtype)
        assert m.last_plan()["tail"] == tail and m.last_plan()["tail_seg"] == ran, m.last_plan()


@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_tail16_sample_seams_inside_workgroups(srcfd, torch_, enc_weights, dec_weights, x3, kind, tail, monkeypatch):
    """n = 13 under the automatic segmentation (10 segments per sample on 256 CUs: 130 virtual samples, workgroups that walk from one
    sample into the next)."""
    m = sr_model(srcfd, enc_weights, dec_weights, kind)
    set_env(monkeypatch, TAILS[tail])
    arm = Arm(torch_, m, cycled(x3, 13), kind, f"{kind} {tail} n = 13")
    _ran_tail(arm, tail, None)
    for out_dtype in gc.OUT_DTYPES:
        arm.check(out_dtype)


# ------------------------------------------------------------------------------------------------------------------------
# the f32-grade precisions
# ------------------------------------------------------------------------------------------------------------------------
F32_ARMS = [("fp32", 1), ("fp32", 3), ("fp32x3", 64), ("fp32x3", 70)]


def _last_kernel(m, n):
    steps = m.f32_steps(n)
    return steps[-1][1], [k for _, k, _ in steps]


@pytest.mark.parametrize("no_tail32", [False, True], ids=["tail32", "NO_TAIL32"])
@pytest.mark.parametrize("precision,n", F32_ARMS, ids=[f"{p}-n{n}" for p, n in F32_ARMS])
def test_f32_partly_bad_fields(srcfd, torch_, enc_weights, dec_weights, x3, precision, n, no_tail32, monkeypatch):
    """tail32 (plain; split-operand from 64 samples on under fp32x3) and, under SRCFD_NO_TAIL32=1, the tiled one-channel output
    convolution conv_n1_tile_f32<FIN>; three output types each; the mixed batch at n >= 3."""
    m = sr_model(srcfd, enc_weights, dec_weights, precision)
    set_env(monkeypatch, {"SRCFD_NO_TAIL32": "1"} if no_tail32 else {})
    last, kernels = _last_kernel(m, n)
    assert last == ("finalize" if no_tail32 else "tail32"), kernels
    assert ("x3" in kernels) == (precision == "fp32x3"), kernels
    x = cycled(x3, n)
    arm = Arm(torch_, m, x, precision, f"{precision} {last} n = {n}")
    assert arm.plan["precision"] == precision, arm.plan
    for out_dtype in gc.OUT_DTYPES:
        arm.check(out_dtype)
    if n >= 3:
        mixed = Arm(torch_, m, with_nan_input(x), precision, f"{precision} {last} n = {n} mixed")
        for out_dtype in gc.OUT_DTYPES:
            mixed.check_mixed(out_dtype)


def test_fp32_naive_finalize_out(srcfd, torch_, enc_weights, dec_weights, x3):
    """The bring-up path: every layer materialised, finalize_out de-standardises, guards and converts."""
    m = sr_model(srcfd, enc_weights, dec_weights, "fp32_naive")
    last, kernels = _last_kernel(m, 3)
    assert set(kernels) == {"naive"}, kernels
    for x, mixed in ((x3, False), (with_nan_input(x3), True)):
        arm = Arm(torch_, m, x, "fp32_naive", f"fp32_naive finalize_out n = 3{' mixed' if mixed else ''}")
        for out_dtype in gc.OUT_DTYPES:
            if mixed:
                arm.check_mixed(out_dtype)
            else:
                arm.check(out_dtype)


# ------------------------------------------------------------------------------------------------------------------------
# other graphs: the family decoders (outconv16; finalize_out), generic graphs, a multi-channel output
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("hr", [10, 20])
def test_encoder10_decoder_x(srcfd, torch_, enc_weights, x3, hr, precision):
    """encoder_10 + decoder_10 / decoder_20: outconv16 in the 16-bit precisions; in fp32 the last layer is a generic GEMM and
    finalize_out follows.  100 / 400 values per sample: the share and 'partly bad' are asserted, the 400 x 400 conditions are not."""
    fam = importlib.import_module("sr-for-cfd_amd.family")
    m = srcfd.SRModel.from_weights(enc_weights, fam.synthetic_decoder_weights(hr, seed=20 + hr), device=0)
    m.precision = precision
    assert m.output_shape == (hr, hr, 1)
    for x, mixed in ((x3[:1], False), (x3, False), (with_nan_input(x3), True)):
        arm = Arm(torch_, m, x, precision, f"decoder_{hr} {precision} n = {len(x)}{' mixed' if mixed else ''}")
        if precision == "fp32":
            last, kernels = _last_kernel(m, len(x))
            assert last not in ("finalize", "tail32"), kernels          # finalize_out
        else:
            assert arm.plan["decoder"] == "any16" and arm.plan["precision"] == precision, arm.plan     # outconv16
        for out_dtype in gc.OUT_DTYPES:
            if mixed:
                assert np.isnan(arm.acc[2]).all()
                count, got_on, _ = arm.check(out_dtype, triggered=[0], full=False)
                np.testing.assert_array_equal(gc.bits(got_on[1]), gc.bits(gc.cast(arm.acc[1], out_dtype)))
                assert count >= hr * hr and not gc.bits(got_on[2]).any()
            else:
                arm.check(out_dtype, triggered=[0, 1][:len(x)], full=False)     # (sample 2's |acc| stays below 1: float32 cannot overflow it)
    m.close()


def _conv(rng, k, ci, co, act="swish"):
    return dict(kind="conv2d", k=k, stride=1, same=True, act=act, w=(0.5 * rng.standard_normal((k, k, ci, co))).astype(np.float32),
                b=(0.1 * rng.standard_normal(co)).astype(np.float32))


GRAPHS = {  # last layer -> (kernel, input channels, output channels, the last step's kernel)
    "last_1x1": (1, 8, 1, "mfma"),           # not a 3x3: finalize_out
    "three_channels": (3, 8, 3, "mfma"),     # a multi-channel output: finalize_out
    "last_3x3_one_channel": (3, 8, 1, "finalize"),   # conv_n1_tile_f32<FIN> on 17 x 65: partial tiles in x and y
}


@pytest.mark.parametrize("graph", list(GRAPHS))
def test_generic_graphs(srcfd, torch_, graph):
    k, ci, co, want_last = GRAPHS[graph]
    rng = np.random.default_rng(len(graph))
    m = srcfd.SRModel.from_layers([_conv(rng, 3, 2, 8), _conv(rng, k, ci, co, "linear")], (17, 65, 2), device=0)
    assert m.output_shape == (17, 65, co)
    for n in (1, 3):
        last, kernels = _last_kernel(m, n)
        assert last == want_last, kernels
        arm = Arm(torch_, m, rng.standard_normal((n, 17, 65, 2)).astype(np.float32), "fp32", f"{graph} n = {n}")
        for out_dtype in gc.OUT_DTYPES:
            arm.check(out_dtype, triggered=[0, 2] if n == 3 else None, full=False)
    m.close()


# ------------------------------------------------------------------------------------------------------------------------
# graph capture and replay
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,out_dtype", [("bf16", "float16"), ("fp32", "bfloat16")])
def test_capture_and_replay_advance_the_counter_once_each(srcfd, torch_, enc_weights, dec_weights, x3, precision, out_dtype, monkeypatch):
    """The same guarded call three times on the same tensors: plain launches, capture + first launch, one replay."""
    torch = torch_
    set_env(monkeypatch, {})
    m = sr_model(srcfd, enc_weights, dec_weights, precision)
    arm = Arm(torch, m, x3, precision, f"{precision} graph")
    count, want_on, aout = arm.check(out_dtype)
    ad = dev(torch, aout)
    y = torch.empty(arm.oshape, dtype=tdtype(torch, out_dtype), device="cuda")
    counter = torch.full((1,), gc.START, dtype=torch.int64, device="cuda")
    seen = []
    for i in range(3):
        y.zero_()
        m.predict_device(arm.xd, y, out_affine=ad, nan_guard=True, nonfinite=counter)
        torch.cuda.synchronize()
        seen.append(m.last_plan()["graph"])
        assert int(counter.item()) == gc.START + (i + 1) * count, (seen, int(counter.item()), count)
        np.testing.assert_array_equal(gc.bits(host(torch, y, out_dtype)), gc.bits(want_on), err_msg=f"{precision} call {i}: {seen}")
    assert seen == ["eager", "capture", "replay"], seen


# ------------------------------------------------------------------------------------------------------------------------
# the host entry point across its staging seam
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_predict_across_the_staging_seam(srcfd, torch_, enc_weights, dec_weights, x3, precision, monkeypatch):
    """SRModel.predict at n = 130 (128 samples per staged chunk): the count and the bits of the device call."""
    torch = torch_
    set_env(monkeypatch, {})
    m = sr_model(srcfd, enc_weights, dec_weights, precision)
    small = Arm(torch, m, x3, precision, f"{precision} predict")
    n = 130
    x = cycled(x3, n)
    aout = np.stack([gc.trigger_rows(small.acc[i % 3:i % 3 + 1], "float32", first=i // 3)[0] for i in range(n)])
    aout[[5, 127, 128]] = (0.0, 1.0)
    y_host, bad_host = m.predict(x, out_affine=aout, nan_guard=True, return_nonfinite=True)
    y_dev = torch.empty((n, 400, 400, 1), dtype=torch.float32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    m.predict_device(dev(torch, x), y_dev, out_affine=dev(torch, aout), nan_guard=True, nonfinite=counter)
    torch.cuda.synchronize()
    got = y_dev.cpu().numpy()
    zeros = (got == 0).reshape(n, -1).mean(1)
    print(f"{precision} predict n = 130: count {bad_host}, zero-filled share per sample {zeros.min():.4f} ... {zeros.max():.4f}")
    assert bad_host == int(counter.item()) and HW * n * gc.SHARE[0] * 0.9 <= bad_host <= HW * n * gc.SHARE[1]
    np.testing.assert_array_equal(gc.bits(y_host), gc.bits(got))
    assert np.isfinite(y_host).all()
    assert not (got[[5, 127, 128]] == 0).any()        # std = 1: nothing zero-filled on either side of the seam


# ------------------------------------------------------------------------------------------------------------------------
# the tiler
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunked", [True, False], ids=["max_chunk_C", "unchunked"])
def test_tiler_run_counts_over_all_tiles(srcfd, torch_, chunked):
    """Tiler.run on the 5 x 5 -> 10 x 10 model of test_gpu_tiled_overlap.py with the trigger on one component: the counter is the
    sum over the tiles, the field is the host function's on the same handle (whose `predict` is given the guard)."""
    torch = torch_
    import tiled_overlap_ref as ref
    from test_gpu_tiled_overlap import field_shape, small_model
    pl = importlib.import_module("sr-for-cfd_amd.pipeline")
    m = small_model(srcfd)
    ty, tx, c, o = 3, 2, 3, (2, 1)
    n = ty * tx * c
    last, kernels = _last_kernel(m, c if chunked else n)
    assert last == "mfma", kernels       # finalize_out follows
    field = np.random.default_rng(5).standard_normal(field_shape(ty, tx, c, 5, 5, o)).astype(np.float32)
    rng = np.random.default_rng(6)
    ain, aout = (np.stack([rng.standard_normal(c) * 0.1, rng.uniform(0.5, 1.5, c)], 1).astype(np.float32) for _ in range(2))
    tiles = ref.cut(field, 5, o)
    acc = m.predict(tiles, in_affine=np.tile(ain, (ty * tx, 1)))
    comp = 1
    q = float(np.quantile(np.abs(acc[comp::c]), 0.90))
    aout[comp] = (0.0, min(float(gc.FLT_MAX) / q, float(gc.FLT_MAX)))
    want_tiles, count = gc.guard_ref(gc.affine_ref(acc, np.tile(aout, (ty * tx, 1)), "fp32"), "float32")
    per_tile = [gc.guard_ref(gc.affine_ref(acc[s:s + 1], aout[s % c][None], "fp32"), "float32")[1] for s in range(n)]
    assert count == sum(per_tile) and sum(1 for k in per_tile if k) >= 2 and 0.01 * 100 * ty * tx <= count <= 0.25 * 100 * ty * tx, per_tile

    class Guarded:
        bad = 0

        def predict(self, x, in_affine=None, out_affine=None):
            y, k = m.predict(x, in_affine=in_affine, out_affine=out_affine, nan_guard=True, return_nonfinite=True)
            self.bad += k
            return y

    g = Guarded()
    want = pl.tiled_super_resolution(field, g, 5, in_affine=ain, out_affine=aout, overlap=o)
    # (every tile is finite; the stitched field need not be: the blend a + w (b - a) of two values near +-FLT_MAX overflows)
    assert gc.same_bits(want, ref.stitch(want_tiles, ty, tx, c, 5, 5, o), "float32").all()
    assert g.bad == count and np.isfinite(want_tiles).all()
    tiler = srcfd.Tiler(m, ty, tx, c, max_chunk=c if chunked else None, overlap=o)
    assert tiler.plan()["n_chunks"] == (ty * tx if chunked else 1)
    out = torch.empty(tiler.out_shape, dtype=torch.float32, device="cuda")
    counter = torch.full((1,), gc.START, dtype=torch.int64, device="cuda")
    tiler.run(dev(torch, field), out, in_affine=dev(torch, ain), out_affine=dev(torch, aout), nan_guard=True, nonfinite=counter)
    torch.cuda.synchronize()
    print(f"tiler {'chunked' if chunked else 'unchunked'}: bad per tile sample {per_tile}, counter {int(counter.item())}")
    assert int(counter.item()) == gc.START + count
    assert gc.same_bits(out.cpu().numpy(), want, "float32").all()
    assert (np.isfinite(out.cpu().numpy()) == np.isfinite(want)).all() and np.isfinite(want[:, :, [0, 2]]).all()
    tiler.close()


# ------------------------------------------------------------------------------------------------------------------------
# a NaN that is local
# ------------------------------------------------------------------------------------------------------------------------
LOCAL = [("bf16", {}, "tail16"), ("bf16", {"SRCFD_TAIL": "s"}, "tail16s"), ("f16", {}, "tail16"), ("fp32", {}, "tail32"),
         ("fp32", {"SRCFD_NO_TAIL32": "1"}, "finalize")]


@pytest.mark.parametrize("precision,env,kernel", LOCAL, ids=[f"{p}-{k}" for p, _, k in LOCAL])
def test_a_nan_in_one_dense_1_unit(srcfd, torch_, enc_weights, dec_weights, x3, precision, env, kernel, monkeypatch):
    """One dense_1/bias unit is NaN, at latent pixels (5, 7) and (0, 11).  Device against device only: y_on == guard_ref(y_off), the
    count matches, and the bad set holds the unit's true footprint (guard_cases.nan_footprint).  How much further the NaN
    spreads through structural zeros of a kernel's operands is printed for the record and is not bounded."""
    torch = torch_
    set_env(monkeypatch, env)
    for (r, c) in ((5, 7), (0, 11)):
        dec = dict(dec_weights)
        dec["dense_1/bias"] = np.array(dec_weights["dense_1/bias"], np.float32)
        dec["dense_1/bias"][gc.nan_unit(r, c, 3)] = np.nan
        m = srcfd.SRModel.from_weights(enc_weights, dec, device=0)
        m.precision = precision
        foot = gc.nan_footprint(r, c)
        for n in (1, 3):
            xd = dev(torch, x3[:n])
            for out_dtype in ("float32", "float16"):
                dt = tdtype(torch, out_dtype)
                y_off, y_on = (torch.empty((n, 400, 400, 1), dtype=dt, device="cuda") for _ in range(2))
                counter = torch.full((1,), gc.START, dtype=torch.int64, device="cuda")
                m.predict_device(xd, y_off, nan_guard=False)
                m.predict_device(xd, y_on, nan_guard=True, nonfinite=counter)
                torch.cuda.synchronize()
                if precision in gc.SIXTEEN_BIT:
                    assert m.last_plan()["tail"] == kernel, m.last_plan()
                else:
                    assert _last_kernel(m, n)[0] == kernel
                got_off, got_on = host(torch, y_off, out_dtype), host(torch, y_on, out_dtype)
                want_on, count = gc.guard_ref(gc.to_f32(got_off, out_dtype), out_dtype)
                bad = ~gc.finite(got_off, out_dtype)[..., 0]
                rows, cols = np.flatnonzero(bad.any((0, 2))), np.flatnonzero(bad.any((0, 1)))
                print(f"{precision} {kernel} -> {out_dtype}, unit ({r}, {c}), n = {n}: {count} bad, footprint {int(foot.sum())} per sample, "
                      f"{int((bad & ~foot).sum())} outside it; rows {rows[0]}..{rows[-1]}, columns {cols[0]}..{cols[-1]}")
                assert (bad | ~foot).all(), f"{int((foot & ~bad).sum())} values of the footprint are finite"
                assert not bad.all()
                np.testing.assert_array_equal(gc.bits(got_on), gc.bits(want_on))
                assert int(counter.item()) == gc.START + count and gc.finite(got_on, out_dtype).all()
        m.close()
