"""tail16 with 13 BC items per round -- item 12 carries BOTH ConvT#3 tap rows of 100-level pixels 192-199 on 16 of its 32 columns
(csrc/tail16_schedule.h) -- against `tail16s` (SRCFD_TAIL=s), bit for bit.

Per output element the merged item runs the MFMAs, A rows, B column, k order, swish and stores of the two quarter-full items it
replaces; only the column an element sits in changed.  So every comparison is `np.array_equal` on raw bits: no tolerance.
  * n = 1, 3: the plan cuts samples into segments, so warm-up strips (A and BC only) meet the merged item; n = 7; n = CUs + 1,
    unsegmented: workgroup 0 walks two samples across a seam.
  * bf16 and f16 operands; f32 / bf16 / f16 output; in_affine, out_affine and nan_guard on, non-finite count zero.  (f16 output
    runs without an out_affine, as in tests/test_gpu_tail16_roles.py: with one, tail16s rounds once where tail16 rounds twice.)
  * Besides the whole array, equality is asserted separately on what the merged item writes -- ring rows 8g + 4 .. 8g + 7, x 368-399
    of every strip g, which reach the image as output rows 8g + 4 .. 8g + 7 and columns 368-399 -- on the columns left of it
    (336-367, the last full item of the row) and on rows 8g .. 8g + 3 of both (100-level row 0, whose items kept their columns): a
    wrong lane-to-row select or a store from a clamped lane then names its position.
  * decoder_400 at n = 3 and n = 7 against the recorded sha256 of tests/golden/lowp16_output_digests.json (read only).
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, require_gpu

import stream_order as so
import test_gpu_lowp16_bits as bits16

pytestmark = pytest.mark.gpu

NO_AFFINE = "none"
ROWS = np.arange(400)
REGIONS = {   # name -> (row mask, column slice)
    "merged item: rows 8g+4..8g+7, columns 368-399": (ROWS % 8 >= 4, slice(368, 400)),
    "left neighbour: rows 8g+4..8g+7, columns 336-367": (ROWS % 8 >= 4, slice(336, 368)),
    "100-level row 0: rows 8g..8g+3, columns 368-399": (ROWS % 8 < 4, slice(368, 400)),
    "100-level row 0: rows 8g..8g+3, columns 336-367": (ROWS % 8 < 4, slice(336, 368)),
}


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
    rng = np.random.default_rng(1312)
    nmax = c.cus + 1
    c.x = torch.from_numpy((rng.standard_normal((nmax, 10, 10, 1)) * 0.2 + 0.5).astype(np.float32)).cuda()
    c.ain = torch.from_numpy(np.stack([np.full(nmax, 0.5) + rng.standard_normal(nmax) * 0.01, rng.uniform(0.15, 0.25, nmax)], 1).astype(np.float32)).cuda()
    c.aout = torch.from_numpy(np.stack([rng.standard_normal(nmax) * 0.1, rng.uniform(0.05, 0.3, nmax)], 1).astype(np.float32)).cuda()
    c.cache = {}
    return c


def _run(ctx, monkeypatch, kind, n, odt, tail, seg, aout):
    """One forward of the first n samples, in_affine and nan_guard on -> (raw bits as (n, 400, 400), non-finite count, plan)."""
    torch = ctx.torch
    for var, val in (("SRCFD_TAIL", tail), ("SRCFD_TAIL_SEG", seg)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    y = torch.empty((n, 400, 400, 1), dtype=odt, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    m = ctx.models[kind]
    m.predict_device(ctx.x[:n], y, in_affine=ctx.ain[:n], out_affine=None if aout is NO_AFFINE else ctx.aout[:n], nan_guard=True, nonfinite=bad)
    torch.cuda.synchronize()
    plan = m.last_plan()
    assert plan["tail"] == ("tail16s" if tail == "s" else "tail16"), plan
    return so.bits(y).cpu().numpy().reshape(n, 400, 400), int(bad.item()), plan


def _compare(ctx, monkeypatch, kind, n, out, seg):
    odt = getattr(ctx.torch, out)
    aout = NO_AFFINE if out == "float16" else None
    key = (kind, n, out, seg)
    if key not in ctx.cache:                         # tail16s's result: computed once per case and left unchanged
        ctx.cache[key] = _run(ctx, monkeypatch, kind, n, odt, "s", seg, aout)
    ref, bad_ref, _ = ctx.cache[key]
    got, bad, plan = _run(ctx, monkeypatch, kind, n, odt, None, seg, aout)
    assert bad == bad_ref == 0
    assert len(np.unique(ref[:, :, 368:400])) > 100, "a constant image checks nothing"
    for name, (rows, cols) in REGIONS.items():
        g, r = got[:, rows, cols], ref[:, rows, cols]
        if not np.array_equal(g, r):
            s, y, x = (int(v[0]) for v in np.nonzero(g != r))
            pytest.fail(f"{name}: {int((g != r).sum())} of {g.size} outputs differ from tail16s; first at sample {s}, row {int(ROWS[rows][y])}, "
                        f"column {cols.start + x}")
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {got.size} outputs differ from tail16s (outside the merged item's region)"
    return plan


@pytest.mark.parametrize("out", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("n", [1, 3])
def test_segmented_small_batches_match_tail16s(ctx, monkeypatch, n, kind, out):
    """The plan's own segmentation (> 1 at these sizes): every segment but a sample's first starts with a warm-up strip whose BC
    items -- the merged one among them -- refill the ring rows the segment's first output row pair reads."""
    plan = _compare(ctx, monkeypatch, kind, n, out, None)
    assert int(plan["tail_seg"]) > 1, plan


@pytest.mark.parametrize("kind,out", [("bf16", "float32"), ("f16", "bfloat16"), ("bf16", "float16")])
def test_seven_samples_match_tail16s(ctx, monkeypatch, kind, out):
    _compare(ctx, monkeypatch, kind, 7, out, None)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_two_samples_per_workgroup_match_tail16s(ctx, monkeypatch, kind):
    """CUs + 1 samples, unsegmented: workgroup 0 runs sample 0 and then sample CUs without draining the pipeline, so the merged item
    of the second sample's first strip runs in the round that finishes the first sample's last rows."""
    plan = _compare(ctx, monkeypatch, kind, ctx.cus + 1, "float32", "1")
    assert plan["tail_seg"] == "1", plan


@pytest.mark.parametrize("n", [3, 7])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_decoder_400_has_the_recorded_bits(srcfd, enc_weights, kind, n):
    """The golden file is read, never written: the merged item must not move a bit of the recorded outputs."""
    require_gpu(srcfd)
    case = next(c for c in bits16.CASES if c[0] == 400 and c[1] == n and c[2] == {} and c[4] == kind)
    doc = json.load(open(os.path.join(GOLDEN, "lowp16_output_digests.json")))
    assert doc["commit"] == bits16.RECORDED_ON
    golden = doc["cases"][bits16.case_id(case)]
    assert bits16.sha256(bits16.case_input(case)) == golden["input_sha256"]
    (y,), plan = bits16.run_case(srcfd, enc_weights, case)
    assert plan["tail"] == "tail16", plan
    assert y.shape == (n, 400, 400, 1) and bits16.sha256(y) == golden["output_sha256"], f"output bits differ from commit {doc['commit']}'s"
