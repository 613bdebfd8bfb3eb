"""The batch sizes at which the SR network's training step is held to float64 autograd above 8 samples (tests/test_train_batches.py
proves what they reach and that the tolerance has room for them without a device, tests/test_gpu_train_batches.py runs them), and
what both modules share: the cases' inputs and references, a second float32 evaluation of the reference in another order, and the
planted defects.

The step changes form with the batch n in four places (tests/train_plan_ref.py restates the rules): the segments per sample of
tail32<TRAIN> (ragged where they do not divide the 100 strips), the tile and pair count of tail_bwd32, the 16-sample groups of
train_enc, and per op the slices and the slab-sum tier of the weight gradients.  test_gpu_training_oracle.py runs n = 1, 3, 8;
BATCHES adds eight sizes in 9 .. 32, the benchmarked 32 among them, and SMALL adds 7: the segment count 34 occurs at n = 6 and 7
only, below the range BATCHES is drawn from, and no other module holds it to float64 in a step of its own."""
import numpy as np

from train_plan_ref import short_last_slice, tail32_ragged, tail32_segments, tail_bwd32_tiles, tier, train_enc_groups, wgrad_slices

ORACLE_BATCHES = (1, 3, 8)                        # test_gpu_training_oracle.py: test_sr_network_every_path_matches_oracle
SMALL = (7,)
BATCHES = (9, 12, 13, 16, 17, 20, 26, 32)         # at most 8, in 9 .. 32, with 16, 17 and 32
RUN = SMALL + BATCHES                             # what test_gpu_train_batches.py runs against float64
CUS = 256                                         # the reach proof's CU count (MI355X)
TAIL_H = TAIL_W = 50                              # the fused tail's input level of the 10 -> 400 network
# n -> seed of its batch where it is not _sr_case's 500 + n.  With seed 517 the 17-sample batch's output bias gradient (one sum over
# 17 x 160 000 pixels, cond 5) did not fit the headroom rule: the second float32 evaluation's ratio was 1.5 .. 3.7 on 1 .. 8 CPU
# threads and 9.8 on 16 (torch cuts float32 reductions by the thread count, and the batched run's own error, the scale, fell to a
# third).  2517: at most 3.0 on 1, 2, 4, 8 and 16 threads; the other batches at most 3.0 on all of them with their own seeds.
SEEDS = {17: 2517}
HEADROOM = 4.0                                    # the second float32 evaluation: half the device's allowance of 8


def step_features(n, cus=CUS):
    """the n-dependent forms of the fused kernels at batch n, as a set of names"""
    seg = tail32_segments(n, TAIL_H, cus)
    tiles, last, pairs = tail_bwd32_tiles(n, TAIL_H, TAIL_W)
    full, part = train_enc_groups(n)
    enc = {(1, False): "1 full group", (1, True): "1 full + partial", (2, False): "2 full groups"}.get((full, part > 0))
    f = {f"tail32 segments {seg}", f"tail32 {'ragged' if tail32_ragged(n, TAIL_H, cus) else 'dividing'} above 8: {seg}" if n > 8 else None,
         f"tail_bwd32 last tile {'full' if last == 16 else 'partial'}", f"tail_bwd32 pairs {'odd' if pairs % 2 else 'even'}",
         f"train_enc {enc}" if enc else None}
    return f - {None}


def wgrad_features(entries, ops, n):
    """(op, tier) and (op, short last slice) of every slot of a dumped slab-sum table (test_train_plan.Plan.entries[(tail, n)]); the
    fused tail's slot is op -1, whose slabs are whole workgroups (never short)"""
    f = set()
    for e in entries:
        name = "fused tail" if e["op"] < 0 else f"op {e['op']} {ops[e['op']]['layer']}"
        f.add(f"{name}: tier {e['groups']}")
        if e["op"] >= 0:
            M = n * ops[e["op"]]["MH"] * ops[e["op"]]["MW"]
            f.add(f"{name}: short last slice {'yes' if e['nslices'] > 1 and M % e['rps'] else 'no'}")
    return f


def wgrad_features_ref(ops, n):
    """the same from tests/train_plan_ref.py alone, for all ops run layer by layer"""
    f = set()
    for i, d in enumerate(ops):
        f.add(f"op {i} {d['layer']}: tier {tier(wgrad_slices(d, n)[0])}")
        f.add(f"op {i} {d['layer']}: short last slice {'yes' if short_last_slice(d, n) else 'no'}")
    return f


def first_unreached(wanted, reached):
    """the first feature, in sorted order, that `reached` lacks; None when it has them all"""
    missing = sorted(set(wanted) - set(reached))
    return missing[0] if missing else None


# ---------------------------------------------------------------------------
# cases and references
# ---------------------------------------------------------------------------
def _orc():
    import importlib
    return importlib.import_module("test_gpu_training_oracle")


def sr_case(srcfd, enc_weights, dec_weights, n):
    """(specs, x, y, Ref) of test_gpu_training_oracle._sr_case: seed 500 + n (SEEDS names the exceptions), the border structure in
    the targets; computed once per n and process, and left unchanged by every user"""
    return _orc()._sr_case(srcfd, enc_weights, dec_weights, n, SEEDS.get(n))


_PER_SAMPLE = {}


def per_sample_f32(srcfd, enc_weights, dec_weights, n):
    """(losses, gradients) of the n one-sample batches of sr_case(n) in float32 on the CPU: gradient i is d/dparams of sample i's
    own mean squared error"""
    if n not in _PER_SAMPLE:
        import torch
        ag = _orc()._ag()
        specs, x, y, _ = sr_case(srcfd, enc_weights, dec_weights, n)
        runs = [ag.loss_and_grads_specs(specs, (10, 10, 1), x[i:i + 1], y[i:i + 1], torch.float32) for i in range(n)]
        _PER_SAMPLE[n] = (np.array([r[0] for r in runs], np.float32), np.stack([r[1].astype(np.float32) for r in runs]))
    return _PER_SAMPLE[n]


def second_evaluation_f32(srcfd, enc_weights, dec_weights, n):
    """(loss, flat gradient) of sr_case(n) as a float32 evaluation in another order than the batched one: every sample's gradient
    on its own, divided by n and added up in float32, sample after sample"""
    losses, grads = per_sample_f32(srcfd, enc_weights, dec_weights, n)
    g, l, fn = np.zeros(grads.shape[1], np.float32), np.float32(0), np.float32(n)
    for i in range(n):
        g += grads[i] / fn
        l += losses[i] / fn
    return float(l), g.astype(np.float64)


def loss_ratio(ref, loss):
    """the loss's error over its scale, as `check` of test_gpu_training_oracle.py bounds it (by 8)"""
    o = _orc()
    return abs(loss - ref.l64) / abs(ref.l64) / max(abs(ref.l32 - ref.l64) / abs(ref.l64), o.TINY)


# ---------------------------------------------------------------------------
# planted defects (float64): what a kernel that loses part of a batch would return
# ---------------------------------------------------------------------------
DEFECTS = ("last sample missing", "one output row of the last sample without dpred", "one pixel of the last sample without dpred")


def planted(srcfd, enc_weights, dec_weights, n, defect):
    """(loss, flat gradient) of the float64 reference of sr_case(n) with `defect` planted in its last sample.  The batch gradient is
    the mean of the samples' own, so only the last sample's float64 gradient is computed anew: y := pred on the affected pixels
    makes their dpred zero."""
    import torch
    ag = _orc()._ag()
    specs, x, y, ref = sr_case(srcfd, enc_weights, dec_weights, n)
    xl, yl = x[n - 1:], y[n - 1:].copy()
    l_good, g_good = ag.loss_and_grads_specs(specs, (10, 10, 1), xl, yl, torch.float64)
    if defect == DEFECTS[0]:
        l_bad, g_bad = 0.0, np.zeros_like(g_good)
    else:
        pred = ag.forward_specs(specs, xl).astype(np.float32)   # float32 targets, as every target is: dpred there is below 2^-24 |pred|
        if defect == DEFECTS[1]:
            yl[0, 237] = pred[0, 237]
        else:
            assert defect == DEFECTS[2]
            yl[0, 237, 141] = pred[0, 237, 141]
        l_bad, g_bad = ag.loss_and_grads_specs(specs, (10, 10, 1), xl, yl, torch.float64)
    return ref.l64 + (l_bad - l_good) / n, ref.g64 + (g_bad - g_good) / n
