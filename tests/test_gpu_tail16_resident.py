"""tail16 reads a BC item's constants (two ConvT#3 weight fragments, ConvT#4's fragment, the bias b4) ONCE per launch into
registers, where it used to read them from LDS for every item.

What can go wrong with that is a constant of the wrong launch, the wrong model or the wrong item staying in a register, so:
  * two models with different synthetic decoders (seeds 1 and 2) are called alternately on one stream, A B A B, without a
    synchronisation in between, at n = 1 and n = 3, bf16 and f16 operands; every one of the four results must equal the same
    model's `tail16s` (SRCFD_TAIL=s) result, which reads every constant from LDS for every item -- `np.array_equal` on raw bits;
  * SRCFD_TAIL_SEG=5 at n = 3, bf16: warm-up strips and segment seams, where the BC stage returns early (and waves 14 and 15, which
    have no BC item, load constants they never use); against the unsegmented result and against `tail16s`, bit for bit.
Encoder: the golden multiBC .h5.  References are computed once per case and left unchanged.
"""
import numpy as np
import pytest

from conftest import require_gpu

import stream_order as so

pytestmark = pytest.mark.gpu

SEEDS = (1, 2)


@pytest.fixture(scope="module")
def ctx(srcfd, oracle, enc_weights):
    require_gpu(srcfd)
    import torch

    class Ctx:
        pass
    c = Ctx()
    c.torch = torch
    c.models = {}
    for seed in SEEDS:
        dec = oracle.synthetic_decoder(seed)
        for kind in ("bf16", "f16"):
            m = srcfd.SRModel.from_weights(enc_weights, dec, device=0)
            m.precision = kind
            c.models[seed, kind] = m
    rng = np.random.default_rng(2903)
    c.x = torch.from_numpy(rng.standard_normal((3, 10, 10, 1)).astype(np.float32)).cuda()
    c.aout = torch.from_numpy(np.stack([rng.standard_normal(3) * 0.1, rng.uniform(0.05, 0.3, 3)], 1).astype(np.float32)).cuda()
    c.cache = {}
    return c


def _env(monkeypatch, tail, seg):
    for var, val in (("SRCFD_TAIL", tail), ("SRCFD_TAIL_SEG", seg)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


def _call(ctx, model, n, want):
    y = ctx.torch.empty((n, 400, 400, 1), dtype=ctx.torch.float32, device="cuda")
    bad = ctx.torch.zeros(1, dtype=ctx.torch.int64, device="cuda")
    model.predict_device(ctx.x[:n], y, out_affine=ctx.aout[:n], nan_guard=True, nonfinite=bad)
    assert model.last_plan()["tail"] == want, model.last_plan()
    return y, bad


def _reference(ctx, monkeypatch, seed, kind, n, seg=None):
    """tail16s's bits for one model and shape."""
    key = (seed, kind, n, seg)
    if key not in ctx.cache:
        _env(monkeypatch, "s", seg)
        y, bad = _call(ctx, ctx.models[seed, kind], n, "tail16s")
        ctx.torch.cuda.synchronize()
        assert int(bad.item()) == 0
        ctx.cache[key] = so.bits(y).cpu().numpy()
    return ctx.cache[key]


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("n", [1, 3])
def test_two_models_alternating_on_one_stream(ctx, monkeypatch, n, kind):
    refs = {seed: _reference(ctx, monkeypatch, seed, kind, n) for seed in SEEDS}
    assert not np.array_equal(refs[SEEDS[0]], refs[SEEDS[1]])      # the two decoders do differ: a stale constant would show
    _env(monkeypatch, None, None)
    order = [SEEDS[0], SEEDS[1], SEEDS[0], SEEDS[1]]
    outs = [_call(ctx, ctx.models[seed, kind], n, "tail16") for seed in order]   # back to back, no synchronisation in between
    ctx.torch.cuda.synchronize()
    for i, (seed, (y, bad)) in enumerate(zip(order, outs)):
        got = so.bits(y).cpu().numpy()
        assert int(bad.item()) == 0
        assert np.array_equal(got, refs[seed]), f"call {i} (decoder seed {seed}): {int((got != refs[seed]).sum())} of {got.size} outputs differ from tail16s"


def test_segmented_with_early_returns_from_bc(ctx, monkeypatch):
    n, kind, seed = 3, "bf16", SEEDS[0]
    ref = _reference(ctx, monkeypatch, seed, kind, n)
    ref_seg = _reference(ctx, monkeypatch, seed, kind, n, "5")
    assert np.array_equal(ref_seg, ref)
    m = ctx.models[seed, kind]
    _env(monkeypatch, None, "1")
    y, bad = _call(ctx, m, n, "tail16")
    assert m.last_plan()["tail_seg"] == "1", m.last_plan()
    ctx.torch.cuda.synchronize()
    plain = so.bits(y).cpu().numpy()
    assert int(bad.item()) == 0
    _env(monkeypatch, None, "5")
    y, bad = _call(ctx, m, n, "tail16")
    assert m.last_plan()["tail_seg"] == "5", m.last_plan()
    ctx.torch.cuda.synchronize()
    got = so.bits(y).cpu().numpy()
    assert int(bad.item()) == 0
    assert np.array_equal(got, plain), f"{int((got != plain).sum())} of {got.size} outputs differ from the unsegmented result"
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {got.size} outputs differ from tail16s"
