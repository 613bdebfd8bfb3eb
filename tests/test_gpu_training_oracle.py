"""Training gradients against the float64 autograd oracle (oracle/sr_oracle_autograd.py: loss_and_grads_specs) on every layer
shape the trainer accepts.

Tolerance, per gradient tensor: the device's relative L2 error against float64 must be at most min(2e-4, 8 max(e32, 2^-24)),
e32 = the relative L2 error of the same graph run in float32 on the CPU (same inputs, computed here).  The device evaluates the
same sums in other orders (tile and slab partials, summed in slab order) and uses its own exp / reciprocal in swish; two
float32 evaluations of one sum in different orders have errors of the same order, and 8 (3 bits) leaves room for that while
staying far below what a dropped or doubled tile of pixels costs (>~1e-3).  2e-4 is the project's earlier bound, kept as a
ceiling.  The loss: relative error at most 8 max(float32 CPU loss error, 2^-24).

One class of tensors has a floor of its own: a BIAS gradient is one sum over every output pixel of the layer's dZ, and with
targets of either sign that sum cancels (sum |dZ| / |sum dZ| = cond reaches ~600 in this file).  Then any float32 evaluation's
error is set by the order of the additions times cond, and the CPU's own order is not the device's (the device adds rows one
after the other per slice and the slices in order; torch's CPU kernels use blocked / vectorised reductions that depend on the
host CPU).  Measured on the CPU for the output bias of a 864-pixel layer with cond 66: float32 CPU error 1.05e-7 on one host and
1.24e-6 on another for the same graph and inputs, the device 8.5e-7 (8.1x the first host's e32); for a 56-pixel output bias
with cond 592: torch float32 3.2e-6, a serial float32 sum of the same float32 terms 1.2e-5, a pairwise one 9.6e-6.  So for bias tensors the scale is max(e32, 2^-24, 2^-24 cond): the error of
rounding each float32 term once, amplified by the sum's conditioning -- independent of the CPU, and a dropped or doubled tile
of 16 pixels out of M moves such a sum by ~sqrt(16 / M) cond, orders above 8 x 2^-24 cond.  The 2e-4 ceiling still holds.

Every case prints its worst ratio device / scale (the table of DESIGN §4.3) and asserts the training path it is there for
(Trainer.plan)."""
import importlib

import numpy as np
import pytest

from conftest import require_gpu
from train_plan_ref import gemm_ops, tier, wgrad_slices

TINY = 2.0 ** -24
RATIO = 8.0
CEIL = 2e-4


def _ag():
    from oracle import sr_oracle_autograd as ag
    return ag


def _tr():
    return importlib.import_module("sr-for-cfd_amd.train")


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
class Ref:
    """float64 and float32 CPU oracle runs of one graph on one batch."""

    def __init__(self, specs, in_shape, x, y):
        import torch
        ag = _ag()
        self.l64, self.g64, self.cond = ag.loss_and_grads_specs(specs, in_shape, x, y, torch.float64, bias_cond=True)
        self.l32, self.g32 = ag.loss_and_grads_specs(specs, in_shape, x, y, torch.float32)
        self.sizes = ag.param_sizes_specs(specs)


def check(label, ref, loss, g):
    """Asserts the tolerance of the module docstring on every tensor and the loss; returns (worst ratio, its tensor)."""
    g = np.asarray(g, np.float64)
    assert g.size == ref.g64.size == sum(s for _, s in ref.sizes)
    assert len(ref.cond) * 2 == len(ref.sizes)
    worst, worst_name, rows = 0.0, None, []
    off = 0
    for i, (name, size) in enumerate(ref.sizes):
        a, r64, r32 = g[off:off + size], ref.g64[off:off + size], ref.g32[off:off + size]
        off += size
        nr = max(np.linalg.norm(r64), 1e-300)
        e32 = np.linalg.norm(r32 - r64) / nr
        ed = np.linalg.norm(a - r64) / nr
        scale = max(e32, TINY, TINY * ref.cond[i // 2]) if i % 2 else max(e32, TINY)   # odd entries: biases
        ratio = ed / scale
        rows.append((name, ed, scale, ratio))
        if ratio > worst:
            worst, worst_name = ratio, name
    el32 = abs(ref.l32 - ref.l64) / abs(ref.l64)
    eld = abs(loss - ref.l64) / abs(ref.l64)
    emax = max(rows, key=lambda r: r[1])
    print(f"[{label}] worst ratio {worst:.2f} ({worst_name}); largest error {emax[1]:.2e} ({emax[0]}); loss rel {eld:.2e} (f32 CPU {el32:.2e})")
    for name, ed, scale, ratio in rows:
        assert ed <= min(CEIL, RATIO * scale), (label, name, ed, scale, ratio)
    assert eld <= RATIO * max(el32, TINY), (label, "loss", eld, el32)
    return worst, worst_name


def device_step(t, x, y):
    """One accumulating forward_backward over zeroed buffers: (loss, flat gradient) of the batch."""
    import torch
    xd, yd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(y, np.float32)).cuda()
    t.grads.zero_()
    t.sse.zero_()
    t.forward_backward(xd, yd)
    torch.cuda.synchronize()
    return float(t.sse.item()) / (x.shape[0] * t.out_elems), t.grads.cpu().numpy().astype(np.float64)


def glorot(rng, shape, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, shape).astype(np.float32)


def conv(rng, name, k, cin, cout, stride=1, same=True, act="swish"):
    return dict(kind="conv2d", name=name, k=k, stride=stride, same=same, act=act, w=glorot(rng, (k, k, cin, cout), k * k * cin, k * k * cout),
                b=(0.1 * rng.standard_normal(cout)).astype(np.float32))


def convt(rng, name, k, stride, cin, cout, act="swish"):
    # fan of one output pixel ~ (k / s)^2 cin: keeps the activations O(1)
    fi = max(1.0, (k / stride) ** 2) * cin
    lim = np.sqrt(3.0 / fi)
    return dict(kind="conv2d_transpose", name=name, k=k, stride=stride, same=False, act=act,
                w=rng.uniform(-lim, lim, (k, k, cout, cin)).astype(np.float32), b=(0.1 * rng.standard_normal(cout)).astype(np.float32))


def dense(rng, name, cin, cout, act="swish"):
    return dict(kind="dense", name=name, act=act, w=glorot(rng, (cin, cout), cin, cout), b=(0.1 * rng.standard_normal(cout)).astype(np.float32))


def out_shape(specs, in_shape):
    return tuple(_ag().forward_specs(specs, np.zeros((1,) + tuple(in_shape), np.float32)).shape[1:])


def batch(rng, n, in_shape, oshape):
    x = rng.standard_normal((n,) + tuple(in_shape)).astype(np.float32)
    y = rng.standard_normal((n,) + tuple(oshape)).astype(np.float32)
    if len(oshape) == 3:   # structure at the borders of the targets (the SAME padding of the data gradient)
        y[:, :1] += 2.0
        y[:, :, -1:] -= 2.0
    return x, y


# gemm_ops / wgrad_slices / tier: a restatement of the trainer's forward GEMM descriptors and of wgrad_plan (tests/train_plan_ref.py),
# used only to PROVE which tier of slab-sum groups a case reaches, not to check a result


# ---------------------------------------------------------------------------
# (a) the SR network, every path
# ---------------------------------------------------------------------------
_SR_REFS = {}


def _sr_case(srcfd, enc_weights, dec_weights, n, seed=None):
    """seed: the batch's seed, 500 + n unless a caller's table names another for that n (tests/train_batches.py); one case per n"""
    seed = 500 + n if seed is None else seed
    if n not in _SR_REFS:
        specs = srcfd.layers_from_weights(enc_weights, dec_weights)
        rng = np.random.default_rng(seed)
        x, y = batch(rng, n, (10, 10, 1), (400, 400, 1))
        y[:, :2] += 3.0
        y[:, :, -2:] -= 3.0
        _SR_REFS[n] = (seed, specs, x, y, Ref(specs, (10, 10, 1), x, y))
    assert _SR_REFS[n][0] == seed, (n, seed, _SR_REFS[n][0])
    return _SR_REFS[n][1:]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 8])
def test_sr_network_every_path_matches_oracle(srcfd, enc_weights, dec_weights, monkeypatch, n):
    """enc_weights / dec_weights, max_batch 8, SRCFD_TRAIN_TAIL x SRCFD_TRAIN_ENC: all four combinations, each asserted
    through Trainer.plan, against float64 autograd."""
    require_gpu(srcfd)
    specs, x, y, ref = _sr_case(srcfd, enc_weights, dec_weights, n)
    assert ref.sizes == [(k, {**enc_weights, **dec_weights}[k].size) for k in _ag().flat_order(enc_weights, dec_weights)]
    for tail in (1, 0):
        for enc in (1, 0):
            monkeypatch.setenv("SRCFD_TRAIN_TAIL", str(tail))
            monkeypatch.setenv("SRCFD_TRAIN_ENC", str(enc))
            t = _tr().Trainer(srcfd.SRModel.from_layers(specs, (10, 10, 1), device=0), max_batch=8)
            assert t.plan == {"fused_tail": tail, "fused_encoder": enc}
            assert t.n_params == 2_709_491
            loss, g = device_step(t, x, y)
            check(f"sr n={n} tail={tail} enc={enc}", ref, loss, g)
            t.close()


# ---------------------------------------------------------------------------
# (b) one layer kind per graph: a small front layer, the layer under test ("lut"), a 1-channel output
# ---------------------------------------------------------------------------
def _table():
    """name -> (specs, in_shape, odd n > 1, tier of the layer under test's weight-gradient slabs)"""
    rng = np.random.default_rng(600)
    T = {}

    def add(name, specs, in_shape, n, want_tier):
        T[name] = (specs, in_shape, n, want_tier)

    # Conv2D stride 1: SAME k = 1..5, VALID k = 3; channel counts 1, 3, 33, 65; linear and swish
    add("conv_same_k1_c33", [conv(rng, "front", 3, 2, 8), conv(rng, "lut", 1, 8, 33), conv(rng, "out", 3, 33, 1, act="linear")], (9, 11, 2), 3, 1)
    add("conv_same_k2_linear", [conv(rng, "front", 3, 1, 3), conv(rng, "lut", 2, 3, 8, act="linear"), conv(rng, "out", 3, 8, 1, act="linear")], (8, 7, 1), 3, 1)
    add("conv_same_k3_c65", [conv(rng, "front", 1, 3, 8), conv(rng, "lut", 3, 8, 65), conv(rng, "out", 1, 65, 1, act="linear")], (7, 6, 3), 3, 1)
    add("conv_same_k4_c1", [conv(rng, "front", 3, 2, 3), conv(rng, "lut", 4, 3, 1), conv(rng, "out", 3, 1, 1, act="linear")], (9, 8, 2), 5, 1)
    add("conv_same_k5", [conv(rng, "front", 1, 1, 4), conv(rng, "lut", 5, 4, 8), conv(rng, "out", 5, 8, 1, act="linear")], (10, 9, 1), 3, 1)
    add("conv_valid_k3", [conv(rng, "front", 3, 2, 8), conv(rng, "lut", 3, 8, 33, same=False), conv(rng, "out", 3, 33, 1, act="linear")], (9, 10, 2), 3, 1)
    # strided first Conv2D SAME, stride 2, odd and even input sizes
    add("strided_first_odd", [conv(rng, "lut", 3, 1, 8, stride=2), conv(rng, "out", 3, 8, 1, act="linear")], (11, 9, 1), 3, 1)
    add("strided_first_even", [conv(rng, "lut", 4, 3, 33, stride=2), conv(rng, "out", 3, 33, 1, act="linear")], (10, 12, 3), 3, 1)
    # Conv2DTranspose 2x2 s2, 3x3 s2 (four phases of 4 / 2 / 2 / 1 taps), 4x4 s2, 3x3 s1
    add("convt_2s2", [conv(rng, "front", 3, 1, 33), convt(rng, "lut", 2, 2, 33, 3), conv(rng, "out", 3, 3, 1, act="linear")], (5, 6, 1), 3, 1)
    add("convt_3s2", [conv(rng, "front", 3, 2, 8), convt(rng, "lut", 3, 2, 8, 8), conv(rng, "out", 3, 8, 1, act="linear")], (5, 4, 2), 3, 1)
    add("convt_4s2_linear", [conv(rng, "front", 1, 1, 65), convt(rng, "lut", 4, 2, 65, 3, act="linear"), conv(rng, "out", 3, 3, 1, act="linear")], (4, 5, 1), 3, 1)
    add("convt_3s1", [conv(rng, "front", 3, 1, 3), convt(rng, "lut", 3, 1, 3, 8), conv(rng, "out", 1, 8, 1, act="linear")], (6, 5, 1), 3, 1)
    # Flatten -> Dense -> Reshape -> Conv
    add("dense_reshape_conv", [conv(rng, "front", 3, 1, 3), dict(kind="flatten", name="flatten"), dense(rng, "lut", 108, 128),
                                dict(kind="reshape", name="reshape", shape=(4, 4, 8)), conv(rng, "out", 3, 8, 1, act="linear")], (6, 6, 1), 3, 1)
    # both sides of wgrad_is_n1_k72 (the output layer is the one under test here)
    add("n1k72_taken_3x3_8to1", [conv(rng, "front", 3, 1, 8), conv(rng, "lut", 3, 8, 1, act="linear")], (40, 36, 1), 3, 1)
    add("n1k72_not_3x3_4to1", [conv(rng, "front", 3, 1, 4), conv(rng, "lut", 3, 4, 1, act="linear")], (10, 9, 1), 3, 1)
    add("n1k72_not_5x5_8to1", [conv(rng, "front", 3, 1, 8), conv(rng, "lut", 5, 8, 1, act="linear")], (12, 11, 1), 3, 1)
    # tiers of slab-sum groups: >= 8, >= 64, >= 256 slices (one 32 x 32 block, M >= 16384; 130^2 is not a multiple of 64 rows:
    # the last slice is short)
    add("slices_ge8", [conv(rng, "front", 1, 1, 3), conv(rng, "lut", 3, 3, 4), conv(rng, "out", 3, 4, 1, act="linear")], (24, 24, 1), 3, 4)
    add("slices_ge64", [conv(rng, "front", 1, 1, 3), conv(rng, "lut", 3, 3, 4), conv(rng, "out", 3, 4, 1, act="linear")], (72, 72, 1), 3, 8)
    add("slices_ge256_short_last", [conv(rng, "front", 1, 1, 3), conv(rng, "lut", 3, 3, 4), conv(rng, "out", 3, 4, 1, act="linear")], (130, 130, 1), 3, 32)
    return T


TABLE = _table()


def test_table_reaches_every_slab_sum_tier_and_layer_shape():
    """Coverage proof of the table (no GPU): every tier of wgrad_finish_all_f32's finishing groups, a short last slice, both
    sides of wgrad_is_n1_k72, the 4 / 2 / 2 / 1 taps of a 3x3 stride-2 transposed convolution, channel counts 1, 3, 33, 65."""
    tiers, short, n1k72 = set(), False, set()
    chans = set()
    for name, (specs, in_shape, n_odd, want) in TABLE.items():
        ops = gemm_ops(specs, in_shape)
        lut = [d for d in ops if d["layer"] == "lut"]
        assert lut, name
        for nn in (1, n_odd):
            for d in lut:
                ns, rps, M = wgrad_slices(d, nn)
                assert tier(ns) == want, (name, nn, ns)
                tiers.add(tier(ns))
                short = short or (M % rps != 0 and ns > 1)
        for d in ops:
            n1k72.add(d["N"] == 1 and d["TY"] == 3 and d["TX"] == 3 and d["CI"] == 8 and d["nphx"] == 1)
            chans.update((d["CI"], d["N"]))
    assert tiers == {1, 4, 8, 32} and short and n1k72 == {True, False}
    assert {1, 3, 33, 65} <= chans
    taps = sorted(d["TY"] * d["TX"] for d in gemm_ops(*TABLE["convt_3s2"][:2]) if d["layer"] == "lut")
    assert taps == [1, 2, 2, 4]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(TABLE))
def test_layer_table_matches_oracle(srcfd, case):
    require_gpu(srcfd)
    specs, in_shape, n_odd, want = TABLE[case]
    rng = np.random.default_rng(700 + list(TABLE).index(case))
    oshape = out_shape(specs, in_shape)
    m = srcfd.SRModel.from_layers(specs, in_shape, device=0)
    assert tuple(m.output_shape) == oshape
    t = _tr().Trainer(m, max_batch=n_odd)
    assert t.plan == {"fused_tail": 0, "fused_encoder": 0}
    for n in (1, n_odd):
        assert all(tier(wgrad_slices(d, n)[0]) == want for d in gemm_ops(specs, in_shape) if d["layer"] == "lut")
        x, y = batch(rng, n, in_shape, oshape)
        ref = Ref(specs, in_shape, x, y)
        assert t.n_params == ref.g64.size
        loss, g = device_step(t, x, y)
        check(f"{case} n={n}", ref, loss, g)


# ---------------------------------------------------------------------------
# (c) the fused tail on edge widths
# ---------------------------------------------------------------------------
def _tail_specs(h, w):
    rng = np.random.default_rng(100 + h * w)
    specs = [dict(kind="conv2d", name="front", k=3, stride=1, same=True, act="swish", w=glorot(rng, (3, 3, 3, 64), 27, 576),
                  b=(0.1 * rng.standard_normal(64)).astype(np.float32))]
    cin = 64
    for i, cout in enumerate((32, 16, 8)):
        specs.append(dict(kind="conv2d_transpose", name=f"up{i}", k=2, stride=2, same=False, act="swish", w=glorot(rng, (2, 2, cout, cin), 4 * cin, 4 * cout),
                          b=(0.1 * rng.standard_normal(cout)).astype(np.float32)))
        cin = cout
    specs.append(dict(kind="conv2d", name="out", k=3, stride=1, same=True, act="linear", w=glorot(rng, (3, 3, 8, 1), 72, 9), b=np.array([0.05], np.float32)))
    return specs, rng


# (H, W), n: the sizes of test_fused_tail_on_other_image_sizes, then W = 1 (declined: the fix of tail_bwd32's magic divisors),
# H = 1 with fewer pixels than one 16-pixel tile, 1 x 1, the widest row the plan accepts (50: 7 tiles at n = 1, 19 at n = 3 --
# odd counts) and the first it declines (51)
TAIL_SIZES = [((6, 7), 3), ((3, 18), 2), ((9, 4), 5), ((5, 1), 3), ((1, 6), 2), ((1, 1), 1), ((2, 50), 1), ((2, 50), 3), ((2, 51), 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("hw,n", TAIL_SIZES)
def test_fused_tail_edge_widths_match_oracle(srcfd, monkeypatch, hw, n):
    require_gpu(srcfd)
    h, w = hw
    specs, rng = _tail_specs(h, w)
    x, y = batch(rng, n, (h, w, 3), (8 * h, 8 * w, 1))
    ref = Ref(specs, (h, w, 3), x, y)
    fused = 1 if 2 <= w <= 50 else 0
    for env in ("1", "0"):
        monkeypatch.setenv("SRCFD_TRAIN_TAIL", env)
        m = srcfd.SRModel.from_layers(specs, (h, w, 3), device=0)
        assert m.output_shape == (8 * h, 8 * w, 1)
        t = _tr().Trainer(m, max_batch=8)
        assert t.plan == {"fused_tail": fused if env == "1" else 0, "fused_encoder": 0}
        loss, g = device_step(t, x, y)
        check(f"tail {h}x{w} n={n} TRAIN_TAIL={env} fused={t.plan['fused_tail']}", ref, loss, g)
        t.close()


# ---------------------------------------------------------------------------
# (d) seeded random training graphs
# ---------------------------------------------------------------------------
def random_training_graph(rng):
    """The generator of test_random_layer_graphs, restricted to what the trainer takes: a strided Conv2D only as the first
    layer, Conv2DTranspose whose kernel equals its stride or with stride <= 2 (at most four output phases), linear / swish;
    optionally a Flatten -> Dense -> Reshape sandwich."""
    h, w, c = int(rng.integers(3, 12)), int(rng.integers(3, 12)), int(rng.integers(1, 9))
    in_shape = (h, w, c)
    shape = in_shape
    specs = []
    n_layers = int(rng.integers(2, 5))
    for li in range(n_layers):
        kind = ["conv2d", "conv2d_transpose", "dense"][int(rng.integers(0, 3))]
        cin = shape[2]
        cout = int(rng.integers(1, 20)) if li < n_layers - 1 else int(rng.integers(1, 3))
        act = ["swish", "linear"][int(rng.integers(0, 2))]
        if kind == "dense" and shape[0] * shape[1] * cin <= 512:
            oh, ow = int(rng.integers(1, 6)), int(rng.integers(1, 6))
            specs += [dict(kind="flatten", name=f"f{li}"), dense(rng, f"d{li}", shape[0] * shape[1] * cin, oh * ow * cout, act),
                      dict(kind="reshape", name=f"r{li}", shape=(oh, ow, cout))]
            shape = (oh, ow, cout)
            continue
        k = int(rng.integers(1, 5))
        if kind == "conv2d":
            s = int(rng.integers(1, 4)) if li == 0 else 1
            same = bool(rng.integers(0, 2))
            if not same and (shape[0] < k or shape[1] < k):
                same = True
            oh = -(-shape[0] // s) if same else (shape[0] - k) // s + 1
            ow = -(-shape[1] // s) if same else (shape[1] - k) // s + 1
            spec = conv(rng, f"c{li}", k, cin, cout, stride=s, same=same, act=act)
        else:
            s = int(rng.integers(1, 4))
            if s == 3:
                k = 3
            oh, ow = (shape[0] - 1) * s + k, (shape[1] - 1) * s + k
            spec = convt(rng, f"t{li}", k, s, cin, cout, act=act)
        if oh * ow * cout > 20000:
            break
        specs.append(spec)
        shape = (oh, ow, cout)
    if not any("w" in s for s in specs):
        specs.append(conv(rng, "c_last", 1, shape[2], 1, act="linear"))
    return specs, in_shape


def trainer_accepts(specs, in_shape):
    """What trainer_build takes: a strided Conv2D only as the first layer, at most four GEMMs per layer and 23 in all, linear
    and swish activations."""
    ops = gemm_ops(specs, in_shape)
    per_layer = {}
    for d in ops:
        per_layer[d["layer"]] = per_layer.get(d["layer"], 0) + 1
    first = next(s for s in specs if "w" in s)
    strided_ok = all(s is first or s["kind"] != "conv2d" or s.get("stride", 1) == 1 for s in specs)
    acts_ok = all(s.get("act", "linear") in ("linear", "swish") for s in specs if "w" in s)
    return strided_ok and acts_ok and max(per_layer.values()) <= 4 and len(ops) + 1 <= 24


@pytest.mark.gpu
def test_random_training_graphs_match_oracle(srcfd):
    require_gpu(srcfd)
    rng = np.random.default_rng(2025)
    ratios = []
    for trial in range(14):
        specs, in_shape = random_training_graph(rng)
        assert trainer_accepts(specs, in_shape), (trial, specs)   # the generator never produces a graph the trainer refuses
        n = int(rng.integers(1, 5))
        oshape = out_shape(specs, in_shape)
        m = srcfd.SRModel.from_layers(specs, in_shape, device=0)
        assert tuple(m.output_shape) == oshape, (trial, specs)
        t = _tr().Trainer(m, max_batch=4)
        assert t.plan == {"fused_tail": 0, "fused_encoder": 0}
        x, y = batch(rng, n, in_shape, oshape)
        ref = Ref(specs, in_shape, x, y)
        desc = " ".join(f"{s['kind']}:k{s.get('k', '')}s{s.get('stride', '')}{'S' if s.get('same') else ''}:{s.get('act', '')}" for s in specs)
        loss, g = device_step(t, x, y)
        ratios.append(check(f"random {trial} n={n} in={in_shape} {desc}", ref, loss, g))
        t.close()
    print("random graphs: worst ratio", max(ratios))


# ---------------------------------------------------------------------------
# (e) refusals: an error status with a message from create, before anything runs
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_trainer_refuses_what_it_cannot_differentiate(srcfd):
    require_gpu(srcfd)
    rng = np.random.default_rng(800)
    tr = _tr()
    # a strided Conv2D after the first layer (build_dgrad has no descriptor for it)
    m = srcfd.SRModel.from_layers([conv(rng, "a", 3, 1, 4), conv(rng, "b", 3, 4, 4, stride=2), conv(rng, "out", 3, 4, 1, act="linear")], (8, 8, 1), device=0)
    with pytest.raises(ValueError, match="strided Conv2D"):
        tr.Trainer(m, max_batch=2)
    # a layer that plans into more than four GEMMs: Conv2DTranspose 2x2 stride 3 -> nine output phases (engine.hip build_plan)
    specs = [conv(rng, "a", 3, 1, 4), convt(rng, "up", 2, 3, 4, 2), conv(rng, "out", 3, 2, 1, act="linear")]
    assert len([d for d in gemm_ops(specs, (4, 4, 1)) if d["layer"] == "up"]) == 9
    m = srcfd.SRModel.from_layers(specs, (4, 4, 1), device=0)
    with pytest.raises(ValueError, match="at most four per layer"):
        tr.Trainer(m, max_batch=2)
    # an activation without a backward pass here (it would have been differentiated as the identity)
    m = srcfd.SRModel.from_layers([conv(rng, "a", 3, 1, 4, act="relu"), conv(rng, "out", 3, 4, 1, act="linear")], (8, 8, 1), device=0)
    with pytest.raises(ValueError, match="activation"):
        tr.Trainer(m, max_batch=2)


# ---------------------------------------------------------------------------
# (f) Adam over several steps, with a ragged step
# ---------------------------------------------------------------------------
def adam_m_v_f32(g, m, v, b1=0.9, b2=0.999):
    """numpy float32 restatement of adam_f32's moment expressions (csrc/train.hip)."""
    f = np.float32
    g, m, v = g.astype(f), m.astype(f), v.astype(f)
    b1, b2 = f(b1), f(b2)
    return b1 * m + (f(1) - b1) * g, b2 * v + (f(1) - b2) * g * g


def adam_steps_match_reference(srcfd, enc_weights, dec_weights, max_batch=8, batches=(8, 8, 7, 8, 8)):
    """Trainer.steps on moving batches of `batches` samples on a max_batch handle: after each, the device's own gradient through the
    float64 Adam reference with float64 m / v carried forward -> params (rtol 2e-6, atol 2e-9), Trainer.m and Trainer.v (8x the
    error of the float32 restatement of adam_f32, against float64).  Every ragged step's (fewer samples than max_batch) loss and
    gradient against the oracle on its samples (the 1 / (gb out_elems) scale)."""
    import torch
    ag = _ag()
    specs = srcfd.layers_from_weights(enc_weights, dec_weights)
    t = _tr().Trainer(srcfd.SRModel.from_layers(specs, (10, 10, 1), device=0), max_batch=max_batch)
    rng = np.random.default_rng(900)
    m64 = np.zeros(t.n_params)
    v64 = np.zeros(t.n_params)
    m32, v32 = m64.astype(np.float32), v64.astype(np.float32)
    keep = []
    assert any(n < max_batch for n in batches)
    for step, n in enumerate(batches, start=1):
        x, y = batch(rng, n, (10, 10, 1), (400, 400, 1))
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        keep.append((xd, yd))                      # later batches land at new addresses
        p0 = t.params.cpu().numpy().astype(np.float64)
        loss = t.step(xd, yd)
        torch.cuda.synchronize()
        g = t.grads.cpu().numpy().astype(np.float64)
        if n < max_batch:
            cur = [dict(s) for s in specs]
            off = 0
            for s in cur:
                if "w" in s:
                    kw, kb = s["w"].size, s["b"].size
                    s["w"] = p0[off:off + kw].reshape(s["w"].shape).astype(np.float32); off += kw
                    s["b"] = p0[off:off + kb].reshape(s["b"].shape).astype(np.float32); off += kb
            assert off == t.n_params
            check(f"adam ragged step {step} n={n}", Ref(cur, (10, 10, 1), x, y), loss, g)
        p_ref, m64, v64 = ag.adam_reference(p0, g, m64, v64, step)
        m32, v32 = adam_m_v_f32(g, m32, v32)
        np.testing.assert_allclose(t.params.cpu().numpy(), p_ref, rtol=2e-6, atol=2e-9, err_msg=f"params after step {step}")
        for name, dev, r64, r32 in (("m", t.m, m64, m32), ("v", t.v, v64, v32)):
            nr = np.linalg.norm(r64)
            e32 = np.linalg.norm(r32.astype(np.float64) - r64) / nr
            ed = np.linalg.norm(dev.cpu().numpy().astype(np.float64) - r64) / nr
            print(f"[adam step {step}] {name}: device {ed:.2e}, float32 restatement {e32:.2e}")
            assert ed <= RATIO * max(e32, TINY), (step, name, ed, e32)
    steps = t.t
    t.close()
    assert steps == len(batches)
    return steps


@pytest.mark.gpu
def test_adam_five_steps_and_ragged_step_match_reference(srcfd, enc_weights, dec_weights):
    """Five Trainer.steps on moving batches (8, 8, 7, 8, 8 samples), max_batch 8: adam_steps_match_reference."""
    require_gpu(srcfd)
    assert adam_steps_match_reference(srcfd, enc_weights, dec_weights, max_batch=8, batches=(8, 8, 7, 8, 8)) == 5
