"""What the batch table of tests/train_batches.py reaches, and that the tolerance of tests/test_gpu_training_oracle.py (`check`) has
room for those batches -- both without a device.

Reach: every form that the n-dependent rules of the step (tests/train_plan_ref.py) take for some n <= 32 on 256 CUs occurs at a
batch that a float64 comparison runs.  The fused kernels' forms come from the restated rules; the slices and slab-sum tiers come
from the plan the library itself makes, dumped by the sanitizer-built harness tools/pack_digest.cpp for every batch 1 .. 32
(tests/test_train_plan.py holds that dump to the restatement).

Headroom: a second float32 evaluation of the reference in another order (per-sample gradients, divided by n and added in float32)
stays within ratio 4 of the float64 one at every batch, half of what the device is allowed, so the rule's room does not depend
on the device.  Measured with the fixtures' weights (trained encoder, synthetic decoder), worst ratio and its tensor per batch:
see the table in DESIGN section 4.3.

Teeth: three defects planted on the float64 reference at n = 32, each a part of the last sample lost, fail `check`."""
import re

import numpy as np
import pytest

import train_batches as tb
from test_train_plan import plans   # noqa: F401  (the module-scoped fixture: the harness's dump)
from train_plan_ref import tail32_blocks, tail32_ragged, tail32_segments, tail_bwd32_blocks, tail_bwd32_tiles, train_enc_groups


def test_the_restated_rules_on_known_values():
    """The segment table of DESIGN section 4.3 (256 CUs), tail_bwd32's tile range, the encoder's groups."""
    table = {(1, 2): 100, (3, 5): 50, (6, 7): 34, (8, 10): 25, (11, 12): 20, (13, 15): 17, (16, 19): 13, (20, 25): 10, (26, 32): 8}
    for (lo, hi), seg in table.items():
        for n in range(lo, hi + 1):
            assert tail32_segments(n, 50, 256) == seg, n
            assert tail32_ragged(n, 50, 256) == (seg in (34, 17, 13, 8))
            assert tail32_blocks(n, seg, 256) == n * seg <= 256
    assert tail32_blocks(96, 1, 256) == 96 and tail32_blocks(300, 1, 256) == 256 and tail32_blocks(3, 0, 256) == 3
    assert [tail_bwd32_tiles(n, 50, 50)[0] for n in (1, 8, 9, 32)] == [157, 1250, 1407, 5000]
    assert tail_bwd32_tiles(1, 50, 50) == (157, 4, 79) and tail_bwd32_tiles(32, 50, 50) == (5000, 16, 2500)
    assert [tail_bwd32_blocks(n, 50, 50, 256) for n in (1, 2, 3, 4, 32)] == [79, 157, 235, 256, 256]
    assert tail_bwd32_blocks(1, 1, 2, 256) == 1
    assert [train_enc_groups(n) for n in (1, 16, 17, 32)] == [(0, 1), (1, 0), (1, 1), (2, 0)]


def test_table_is_small_and_names_the_required_batches():
    assert len(tb.BATCHES) <= 8 and all(9 <= n <= 32 for n in tb.BATCHES) and {16, 17, 32} <= set(tb.BATCHES)
    assert len(set(tb.RUN)) == len(tb.RUN) and not set(tb.RUN) & set(tb.ORACLE_BATCHES)
    assert all(n <= 8 for n in tb.SMALL)


def test_table_reaches_every_form_of_the_fused_kernels():
    """Fails with the name of the first form that no batch held to float64 reaches."""
    held = tb.ORACLE_BATCHES + tb.RUN
    wanted = set().union(*(tb.step_features(n) for n in range(1, 33)))
    reached = set().union(*(tb.step_features(n) for n in held))
    assert len([f for f in wanted if f.startswith("tail32 segments")]) == 9
    assert tb.first_unreached(wanted, reached) is None, tb.first_unreached(wanted, reached)
    # above 8 samples, from BATCHES alone: every segment count of 9 .. 32, at least two ragged and two dividing ones
    above = set().union(*(tb.step_features(n) for n in tb.BATCHES))
    wanted_above = {f for n in range(9, 33) for f in tb.step_features(n)}
    assert tb.first_unreached(wanted_above, above) is None, tb.first_unreached(wanted_above, above)
    assert len([f for f in above if f.startswith("tail32 ragged above 8")]) >= 2
    assert len([f for f in above if f.startswith("tail32 dividing above 8")]) >= 2
    for name in ("tail_bwd32 last tile full", "tail_bwd32 last tile partial", "tail_bwd32 pairs odd", "tail_bwd32 pairs even",
                 "train_enc 1 full group", "train_enc 1 full + partial", "train_enc 2 full groups"):
        assert name in above, name


def test_table_reaches_every_slab_sum_tier_and_slice_form(plans):
    """Per op of the layer-by-layer step, and with SRCFD_TRAIN_TAIL=0 also the four tail layers (tail = 0 in the dump): every
    slab-sum tier and every `short last slice: yes / no` that the library's plan gives anywhere in 9 .. 32 occurs at a held
    batch.  From the dump; the restatement must give the same features."""
    sr = plans["sr"]
    held = tb.ORACLE_BATCHES + tb.RUN
    for tail in (0, 1):
        wanted = set().union(*(tb.wgrad_features(sr.entries[(tail, n)], sr.ops, n) for n in range(9, 33)))
        reached = set().union(*(tb.wgrad_features(sr.entries[(tail, n)], sr.ops, n) for n in held))
        assert tb.first_unreached(wanted, reached) is None, (tail, tb.first_unreached(wanted, reached))
        assert len(wanted) >= 2 * (len(sr.ops) - 4 * tail)
        if tail == 0:
            for n in range(1, 33):
                assert tb.wgrad_features(sr.entries[(0, n)], sr.ops, n) == tb.wgrad_features_ref(sr.ops, n), n
    # the forms that only some batches above 8 have, by name: without them the table would prove less than it says
    ops = sr.ops
    convt1 = next(i for i, o in enumerate(ops) if o["layer"] == "conv2d_transpose_1")
    convt2 = next(i for i, o in enumerate(ops) if o["layer"] == "conv2d_transpose_2")
    above = set().union(*(tb.wgrad_features(sr.entries[(0, n)], ops, n) for n in tb.BATCHES))
    assert {f"op {convt1} conv2d_transpose_1: tier 4", f"op {convt1} conv2d_transpose_1: tier 8", f"op {convt2} conv2d_transpose_2: short last slice no",
            "op 0 conv2d: tier 1", "op 0 conv2d: tier 4"} <= above


def test_first_unreached_names_the_gap():
    """the reach proofs' own teeth: without 32 the table misses forms, and the first one is named"""
    held = [n for n in tb.ORACLE_BATCHES + tb.RUN if n != 32]
    wanted = set().union(*(tb.step_features(n) for n in range(1, 33)))
    assert tb.first_unreached(wanted, set().union(*(tb.step_features(n) for n in held))) == "train_enc 2 full groups"
    held = [n for n in tb.ORACLE_BATCHES + tb.RUN if n != 7]
    assert tb.first_unreached(wanted, set().union(*(tb.step_features(n) for n in held))) == "tail32 segments 34"


@pytest.mark.parametrize("n", tb.RUN)
def test_second_float32_evaluation_stays_within_half_the_allowance(srcfd, enc_weights, dec_weights, n):
    orc = tb._orc()
    _, _, _, ref = tb.sr_case(srcfd, enc_weights, dec_weights, n)
    loss, g = tb.second_evaluation_f32(srcfd, enc_weights, dec_weights, n)
    worst, name = orc.check(f"second float32 evaluation n={n}", ref, loss, g)
    lr = tb.loss_ratio(ref, loss)
    print(f"[second float32 evaluation n={n}] worst ratio {worst:.2f} ({name}), loss ratio {lr:.2f}")
    assert worst <= tb.HEADROOM and lr <= tb.HEADROOM, (n, worst, name, lr)


@pytest.mark.parametrize("defect", tb.DEFECTS)
def test_planted_defects_fail_the_check(srcfd, enc_weights, dec_weights, capsys, defect):
    orc = tb._orc()
    _, _, _, ref = tb.sr_case(srcfd, enc_weights, dec_weights, 32)
    loss, g = tb.planted(srcfd, enc_weights, dec_weights, 32, defect)
    with pytest.raises(AssertionError):
        orc.check(f"planted: {defect}", ref, loss, g)
    out = capsys.readouterr().out
    print(out, end="")
    worst = float(re.search(r"worst ratio ([0-9.]+(?:e[+-]?[0-9]+)?|inf)", out).group(1))
    assert worst > orc.RATIO, (defect, worst)
    # and the unplanted reference passes, so it is the defect that fails
    assert orc.check("float64 reference itself", ref, ref.l64, ref.g64)[0] == 0.0
