"""tail16's two wave roles (waves 0-7: BC + A; waves 8-15: D + BC, every D item of a round) against `tail16s` (SRCFD_TAIL=s), bit for bit.

The role split only changes WHICH wave issues an item and when: per output element the MFMAs, their k order, the swish and the one
de-standardising fma are what they were.  So every comparison here is `np.array_equal` on the raw bits of the output -- no tolerance.
Shapes are the smallest at which the mapping of items to waves can go wrong:
  * n = 1, 3: one sample per workgroup (K = 1), pipeline fill and drain, the top and bottom seam rows, all 16 D items of a round --
    the fourth item of every row pair holds tiles 48 and 49 only;
  * n = CUs + 3, unsegmented: three workgroups walk two samples, so a sample seam runs through the waves that own the D items;
  * SRCFD_TAIL_SEG = 1, 2, 5 at n = 3: warm-up strips and segment seams;
  * the non-finite count of the fast path is taken per wave through a lane mask that moves with the items: exact counts;
  * one call on a non-default stream (tests/stream_order.py).
Encoder: the golden multiBC .h5; decoder: synthetic, seed 1 (conftest.py).
"""
import numpy as np
import pytest

from conftest import require_gpu

import stream_order as so

pytestmark = pytest.mark.gpu

PER_SAMPLE = 400 * 400


@pytest.fixture(scope="module")
def ctx(srcfd, enc_weights, dec_weights):
    require_gpu(srcfd)
    import torch

    class Ctx:
        pass
    c = Ctx()
    c.torch = torch
    c.cus = torch.cuda.get_device_properties(0).multi_processor_count
    c.models = {}
    for kind in ("bf16", "f16"):
        m = srcfd.SRModel.from_weights(enc_weights, dec_weights, device=0)
        m.precision = kind
        c.models[kind] = m
    rng = np.random.default_rng(1603)
    nmax = c.cus + 3
    c.x = torch.from_numpy(rng.standard_normal((nmax, 10, 10, 1)).astype(np.float32)).cuda()
    c.aout = torch.from_numpy(np.stack([rng.standard_normal(nmax) * 0.1, rng.uniform(0.05, 0.3, nmax)], 1).astype(np.float32)).cuda()
    c.cache = {}
    return c


def _raw(t):
    """The output's bits as a numpy integer array."""
    return so.bits(t).cpu().numpy()


NO_AFFINE = "none"


def _run(ctx, monkeypatch, kind, n, odt, tail, seg, aout=None, guard=True, stream=None):
    """One forward of the first n samples -> (raw bits, non-finite count, plan).  aout: None = the module's out_affine."""
    torch = ctx.torch
    for var, val in (("SRCFD_TAIL", tail), ("SRCFD_TAIL_SEG", seg)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    m = ctx.models[kind]
    y = torch.empty((n, 400, 400, 1), dtype=odt, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    a = ctx.aout[:n] if aout is None else (None if aout is NO_AFFINE else aout)
    m.predict_device(ctx.x[:n], y, out_affine=a, nan_guard=guard, nonfinite=bad, stream=stream)
    torch.cuda.synchronize()
    plan = m.last_plan()
    assert plan["tail"] == ("tail16s" if tail == "s" else "tail16"), plan
    if seg is not None:
        assert plan["tail_seg"] == seg, plan
    return _raw(y), int(bad.item()), plan


def _reference(ctx, monkeypatch, kind, n, odt, seg, aout=None):
    """tail16s's result, computed once per case and left unchanged."""
    key = (kind, n, str(odt), seg, aout is NO_AFFINE)
    if key not in ctx.cache:
        ctx.cache[key] = _run(ctx, monkeypatch, kind, n, odt, "s", seg, aout=aout)
    return ctx.cache[key]


@pytest.mark.parametrize("out", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("n", [1, 3])
def test_one_sample_per_workgroup_matches_tail16s(ctx, monkeypatch, n, kind, out):
    """f32 and bf16 output with an out_affine; f16 output without one, as tests/test_gpu_parity_bf16.py compares it.  (With an
    out_affine the two kernels round an f16 output differently, and did before the role split: the f16-output build of tail16s
    fuses the de-standardising fma and the conversion into one instruction with ONE rounding, v_fma_mixlo_f16, where tail16 rounds
    to f32 and then to f16 -- 5 of 160 000 values one f16 ulp apart at n = 1.  tail16s is the untouched arm here.)"""
    odt = getattr(ctx.torch, out)
    aout = NO_AFFINE if out == "float16" else None
    ref, bad_ref, _ = _reference(ctx, monkeypatch, kind, n, odt, None, aout=aout)
    got, bad, _ = _run(ctx, monkeypatch, kind, n, odt, None, None, aout=aout)
    assert bad == bad_ref == 0
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {got.size} outputs differ from tail16s"


def test_two_samples_per_workgroup_matches_tail16s(ctx, monkeypatch):
    """CUs + 3 samples, unsegmented: workgroups 0-2 run sample b and then sample CUs + b without draining the pipeline."""
    n = ctx.cus + 3
    ref, bad_ref, _ = _reference(ctx, monkeypatch, "bf16", n, ctx.torch.float32, "1")
    got, bad, _ = _run(ctx, monkeypatch, "bf16", n, ctx.torch.float32, None, "1")
    assert bad == bad_ref == 0
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {got.size} outputs differ from tail16s"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_segmented_equals_unsegmented(ctx, monkeypatch, kind):
    f32 = ctx.torch.float32
    ref, bad_ref, _ = _run(ctx, monkeypatch, kind, 3, f32, None, "1")
    s_ref, _, _ = _reference(ctx, monkeypatch, kind, 3, f32, None)
    assert np.array_equal(ref, s_ref)
    for seg in ("2", "5"):
        got, bad, _ = _run(ctx, monkeypatch, kind, 3, f32, None, seg)
        assert bad == bad_ref == 0
        assert np.array_equal(got, ref), f"segments={seg}: {int((got != ref).sum())} outputs differ from the unsegmented result"


@pytest.mark.parametrize("big", [False, True], ids=["n=3", "n=CUs+3"])
def test_nonfinite_count_is_exact(ctx, monkeypatch, big):
    """out_affine picks what becomes non-finite: std = inf (every value of the sample: inf, or NaN where the conv gave 0), mean = NaN
    (every value), and std = 3e38 with a mean that puts the overflow threshold at the median of the sample's positive conv outputs
    (y * std + mean > FLT_MAX above it, finite below: waves with some lanes bad and some not)."""
    torch = ctx.torch
    n = ctx.cus + 3 if big else 3
    aout = ctx.aout[:n].clone()
    whole = [1, ctx.cus, n - 1] if big else [1]       # the second sample of workgroup 0 and of workgroup 2 among them
    partial = [0, ctx.cus + 1] if big else [2]
    aout[whole[0], 1] = float("inf")
    for s in whole[1:]:
        aout[s, 0] = float("nan")
    seg = "1" if big else None
    ident = torch.zeros_like(aout)
    ident[:, 1] = 1.0            # y * 1 + 0: the conv output itself
    conv, _, _ = _run(ctx, monkeypatch, "bf16", n, torch.float32, "s", seg, aout=ident, guard=False)
    conv = conv.view(np.float32).reshape(n, -1).astype(np.float64)
    flt_max = float(np.finfo(np.float32).max)
    for s in partial:
        t = float(np.median(conv[s][conv[s] > 0]))
        assert 0.0 < t < 2.0, t  # keeps the mean below inside f32
        aout[s, 1] = 3.0e38
        aout[s, 0] = flt_max - 3.0e38 * t
    plain, bad_plain, _ = _run(ctx, monkeypatch, "bf16", n, torch.float32, None, seg, aout=aout, guard=False)
    plain = plain.view(np.float32)
    nonfinite = ~np.isfinite(plain)
    per_sample = nonfinite.reshape(n, -1).sum(1)
    assert bad_plain == 0                                            # no guard, no count
    assert all(per_sample[s] == PER_SAMPLE for s in whole)
    assert all(0 < per_sample[s] < PER_SAMPLE for s in partial), per_sample[partial]
    assert per_sample.sum() == sum(per_sample[s] for s in whole + partial)
    got, bad, _ = _run(ctx, monkeypatch, "bf16", n, torch.float32, None, seg, aout=aout, guard=True)
    assert bad == int(nonfinite.sum())
    assert np.array_equal(got[nonfinite], np.zeros(int(nonfinite.sum()), got.dtype))      # exactly +0.0
    assert np.array_equal(got[~nonfinite], plain.view(got.dtype)[~nonfinite])
    ref, bad_ref, _ = _run(ctx, monkeypatch, "bf16", n, torch.float32, "s", seg, aout=aout, guard=True)
    assert bad_ref == bad and np.array_equal(got, ref)


def test_on_a_side_stream(ctx, monkeypatch):
    torch = ctx.torch
    monkeypatch.delenv("SRCFD_TAIL", raising=False)
    monkeypatch.delenv("SRCFD_TAIL_SEG", raising=False)
    m = ctx.models["bf16"]
    n = 3
    real, aout = ctx.x[:n], ctx.aout[:n]
    decoy = ctx.x[n:2 * n].clone()
    ref, ref_decoy = torch.empty((n, 400, 400, 1), device="cuda"), torch.empty((n, 400, 400, 1), device="cuda")
    m.predict_device(real, ref, out_affine=aout, nan_guard=True)
    m.predict_device(decoy, ref_decoy, out_affine=aout, nan_guard=True)
    torch.cuda.synchronize()
    assert not torch.equal(ref, ref_decoy)
    delay, S = so.Delay(torch), torch.cuda.Stream()
    x, y = torch.empty_like(real), torch.empty_like(ref)
    o = so.delayed_call(torch, delay, S, [so.Arrival(x, decoy, real)], lambda: m.predict_device(x, y, out_affine=aout, nan_guard=True, stream=S),
                        [y], stale=[(y, ref_decoy)], label="tail16 roles n=3")
    assert m.last_plan()["tail"] == "tail16", m.last_plan()
    so.assert_pending(o, "tail16 roles n=3")
    assert np.array_equal(_raw(o.clones[0]), _raw(ref))
