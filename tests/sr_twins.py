"""Exact integer twins of the 10 -> 400 graph with its nine swish layers in place (test_sr_twins.py on the CPU, test_gpu_sr_twins.py).

Swish is exact where it saturates.  The 16-bit kernels evaluate swish_scaled(u) = u * rcp(1 + exp2(-u)) in float32 on u = log2(e) x
(csrc/dev16.h), the f32 kernels x * rcp(1 + exp2(-log2(e) x)) (csrc/kernels_fp32.hip):
  u = 0       0 * rcp(2) = 0
  u >= 25     exp2(-u) <= 2^-25, 1 + e rounds to 1.0f, rcp(1.0f) = 1.0f: the result is u
  u <= -130   exp2(-u) = +inf, rcp(inf) = 0: the result is -0
and between -130 and 25, other than 0, the last bits of the hardware's exp2 / rcp show.  A twin is an integer network (K, J) whose
every swish pre-activation lies in {0} | [25, 256] | (-inf, -130] on every input of `inputs`, so that swish(u) = u if u >= 25 else 0.

Two encodings hand the same integer network to SRModel.from_weights:
  "scaled"  for the 16-bit precisions.  operand_pack.cpp folds log2(e) into the weights (scale_in / scale_out / scale_w), so the
            *scaled* domain is the integer domain when the float32 weights are
              conv2d, dense_1                        K / log2e, J / log2e
              conv2d_1, dense, conv2d_transpose*     K,         J / log2e
              latent_vector, output_image_400        K log2e,   J
            The 16-bit weights the pack rounds them to are the integers K exactly (|K| <= 256; test_sr_twins.py checks every one);
            conv1's f32 weights and the scaled biases come out as k (1 + d), |d| < 1e-7, and the 16-bit store of every layer's output
            rounds that away -- except where an integer pre-activation of 0 is reached by cancellation against a scaled bias or, in
            conv1, between scaled weights: there the device would hold k d, not 0.  Condition 1 below therefore admits u = 0 only
            with J = 0 (conv1: only where every product is 0).
  "plain"   for the f32 precisions: kernel K, bias J.  Every product and sum is an integer below 2^24: float32 is exact.
            NOT for the streaming f32 tail (tail32, kernels_tail32.hip): it multiplies ConvT#2's weights and all its biases by log2(e)
            in float32 and the output convolution's by 1 / log2(e), so its products round (relative 2^-24 each) and its sum over 72
            taps depends on the order.  test_gpu_sr_twins.py compares the plain encoding exactly under SRCFD_NO_TAIL32=1 and holds
            tail32 to the integers after rounding to nearest.

Bound against the float64 oracle (test_sr_twins.py): `oracle_bound`, per element of every layer's output.  The float64 swish
differs from the saturated one by at most u (1 - sigma(25 ln 2)) <= u 2^-25 (at u <= -130 by |u| 2^-130); each float32-rounded scaled
kernel or bias of the scaled encoding adds at most 2^-24 of S = sum |K| |u| + |J|; both are carried to the output through the network of
|K|.  Nothing in it comes from a measured figure.

Pure numpy; nothing here touches the GPU or imports oracle/.
"""
from __future__ import annotations

import numpy as np

LOG2E = 1.4426950408889634
TWIN_SEEDS = (0, 1, 2)
HI, LO = 25, -130            # the saturation bands: u >= HI passes, u <= LO is killed
VMAX = 256                   # stored activations: integers of magnitude <= 256 are exact in bf16 (8 significant bits) and in f16

LAYERS = ("conv2d", "conv2d_1", "dense", "latent_vector", "dense_1", "conv2d_transpose", "conv2d_transpose_1", "conv2d_transpose_2",
          "conv2d_transpose_3", "conv2d_transpose_4", "output_image_400")
ENCODER = LAYERS[:4]
SHAPES = {"conv2d": (3, 3, 1, 64), "conv2d_1": (3, 3, 64, 128), "dense": (3200, 128), "latent_vector": (128, 50), "dense_1": (50, 36864),
          "conv2d_transpose": (3, 3, 128, 256), "conv2d_transpose_1": (2, 2, 64, 128), "conv2d_transpose_2": (2, 2, 32, 64),
          "conv2d_transpose_3": (2, 2, 16, 32), "conv2d_transpose_4": (2, 2, 8, 16), "output_image_400": (3, 3, 8, 1)}
SWISH = {name: name not in ("latent_vector", "output_image_400") for name in LAYERS}
# how the scaled encoding writes (kernel, bias): "/" = divided by log2e, "*" = multiplied, "" = as it is
SCALED = {"conv2d": ("/", "/"), "conv2d_1": ("", "/"), "dense": ("", "/"), "latent_vector": ("*", ""), "dense_1": ("/", "/"),
          "conv2d_transpose": ("", "/"), "conv2d_transpose_1": ("", "/"), "conv2d_transpose_2": ("", "/"), "conv2d_transpose_3": ("", "/"),
          "conv2d_transpose_4": ("", "/"), "output_image_400": ("*", "")}


def swish_sat(u):
    return np.where(u >= HI, u, 0.0)


# ------------------------------------------------------------------------------------------------------------------------
# the integer model: plain numpy on float64 (integers below 2^53 are exact), Keras layer semantics
# ------------------------------------------------------------------------------------------------------------------------
def conv_same(x, K, J, stride, pad_before_rows=None):
    """Conv2D 'same' (TF: out = ceil(in / s), the odd padding pixel goes after).  K (kh, kw, Cin, Cout)."""
    n, h, w, _ = x.shape
    kh, kw, _, cout = K.shape
    oh, ow = -(-h // stride), -(-w // stride)
    th, tw = max((oh - 1) * stride + kh - h, 0), max((ow - 1) * stride + kw - w, 0)
    pt, pl = th // 2, tw // 2
    if pad_before_rows is not None:
        pt = pad_before_rows
    xp = np.zeros((n, h + th, w + tw, x.shape[3]))
    xp[:, pt:pt + h, pl:pl + w] = x
    u = np.zeros((n, oh, ow, cout))
    for a in range(kh):
        for b in range(kw):
            u += xp[:, a:a + (oh - 1) * stride + 1:stride, b:b + (ow - 1) * stride + 1:stride] @ K[a, b]
    return u + J


def convt_valid(x, K, J, skip=None):
    """Conv2DTranspose stride 2 'valid': out[2 i + a, 2 j + b, co] += x[i, j, ci] K[a, b, co, ci].  skip = (a, b, i, j): that one
    contribution is left out (a planted defect)."""
    n, h, w, _ = x.shape
    k, _, cout, _ = K.shape
    u = np.zeros((n, 2 * (h - 1) + k, 2 * (w - 1) + k, cout))
    for a in range(k):
        for b in range(k):
            t = x @ K[a, b].T
            if skip is not None and skip[:2] == (a, b):
                t[:, skip[2], skip[3]] = 0
            u[:, a:a + 2 * h - 1:2, b:b + 2 * w - 1:2] += t
    return u + J


def acc_k(k):
    """operand_pack.cpp: bits 2 and 3 of k exchanged (the k order of a 32x32 accumulator used as the next B operand)."""
    return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1)


def output_conv(t, K, J, pad=None, drop_left_granule=False):
    """3x3 'same' Conv2D to one channel.  pad = 'top' / 'bottom' / 'left' / 'right': that border reads its neighbour row / column in
    place of the zero padding; drop_left_granule: at output columns 8 k (k >= 1) the taps that read column 8 k - 1 are left out."""
    n, H, W, _ = t.shape
    tp = np.pad(t, ((0, 0), (1, 1), (1, 1), (0, 0)))
    if pad == "top":
        tp[:, 0, 1:-1] = t[:, 0]
    elif pad == "bottom":
        tp[:, -1, 1:-1] = t[:, -1]
    elif pad == "left":
        tp[:, 1:-1, 0] = t[:, :, 0]
    elif pad == "right":
        tp[:, 1:-1, -1] = t[:, :, -1]
    y = np.zeros((n, H, W))
    for a in range(3):
        for b in range(3):
            c = tp[:, a:a + H, b:b + W] @ K[a, b, :, 0]
            if drop_left_granule and b == 0:
                c[:, :, 8::8] = 0
            y += c
    return (y + J[0])[..., None]


def forward(K, J, x, return_all=False, defect=None, return_pre=False):
    """The integer model.  x (n, 10, 10, 1) integers -> (n, 400, 400, 1) float64 integers [, the eleven activations][, the eleven
    pre-activations].  defect: one name of PLANTED."""
    assert defect is None or defect in PLANTED, defect
    acts, pre = [], []

    def done(name, u):
        pre.append(u)
        a = swish_sat(u) if SWISH[name] else u
        acts.append(a)
        return a

    x = np.asarray(x, np.float64)
    n = x.shape[0]
    a = done("conv2d", conv_same(x, K["conv2d"], J["conv2d"], 2, pad_before_rows=1 if defect == "conv1_rows_padded_before" else None))
    K1 = K["conv2d_1"]
    if defect == "conv2d_1_tap_transposed":
        K1 = K1.copy()
        K1[0, 1], K1[1, 0] = K["conv2d_1"][1, 0], K["conv2d_1"][0, 1]
    a = done("conv2d_1", conv_same(a, K1, J["conv2d_1"], 1))
    f = a.transpose(0, 3, 1, 2).reshape(n, -1) if defect == "flatten_channel_major" else a.reshape(n, -1)
    a = done("dense", f @ K["dense"] + J["dense"])
    z = done("latent_vector", a @ K["latent_vector"] + J["latent_vector"])
    if defect == "latent_pad_column_read":
        z = z.copy()
        z[:, PAD_COLUMN_VICTIM] = 0       # column 49's weights meet a zero-padded column (50 .. 63) instead
    h = done("dense_1", z @ K["dense_1"] + J["dense_1"])
    h = h.reshape(n, 256, 12, 12).transpose(0, 2, 3, 1) if defect == "dense_1_reshape_channel_major" else h.reshape(n, 12, 12, 256)
    u = convt_valid(h, K["conv2d_transpose"], J["conv2d_transpose"], skip=(0, 0, 0, 0) if defect == "convt0_border_tap_dropped" else None)
    if defect == "convt0_phases_exchanged":
        t = u[:, 0:24:2, 1:24:2].copy()
        u[:, 0:24:2, 1:24:2] = u[:, 1:24:2, 0:24:2]
        u[:, 1:24:2, 0:24:2] = t
    a = done("conv2d_transpose", u)
    for i in range(1, 5):
        name = f"conv2d_transpose_{i}"
        Ki = K[name]
        if defect == "convt1_acc_k_not_undone" and i == 1:      # one 32-row A tile: tap (0, 0), output channels 0 .. 31
            Ki = Ki.copy()
            Ki[0, 0, :32, :] = K[name][0, 0][:32][:, acc_k(np.arange(128))]
        if defect == "convt4_two_channels_exchanged" and i == 4:   # the first output channel whose tap (0, 0) passes: its reader and the channel 8 on
            Ki = Ki.copy()
            co = int(np.argmax(Ki[0, 0].max(1) >= 1))
            c1 = int(np.argmax(Ki[0, 0, co]))
            c2 = (c1 + 8) % 16
            Ki[0, 0, co, [c1, c2]] = Ki[0, 0, co, [c2, c1]]
        if defect == "convt3_taps_transposed" and i == 3:
            Ki = Ki.copy()
            Ki[0, 1], Ki[1, 0] = K[name][1, 0], K[name][0, 1]
        a = done(name, convt_valid(a, Ki, J[name]))
    if defect == "ring_row_one_lap_late":      # sample 0, columns 64 .. 71 of row 200 hold what the ring held a lap (18 rows) earlier
        a = a.copy()
        a[0, 200, 64:72] = a[0, 182, 64:72]
    pad = defect[len("outconv_reads_neighbour_"):] if defect is not None and defect.startswith("outconv_reads_neighbour_") else None
    y = done("output_image_400", output_conv(a, K["output_image_400"], J["output_image_400"], pad=pad,
                                             drop_left_granule=defect == "outconv_left_granule_tap_dropped"))
    if defect == "last_row_from_next_sample" and n > 1:
        y = y.copy()
        y[0, 399] = y[1, 399]
        acts[-1] = y
    out = (y,)
    if return_all:
        out += (acts,)
    if return_pre:
        out += (pre,)
    return out if len(out) > 1 else y


PAD_COLUMN_VICTIM = 49
# index-level defects of the integer model, each confined to the smallest unit it can hit (see forward)
PLANTED = ("conv1_rows_padded_before", "conv2d_1_tap_transposed", "flatten_channel_major", "latent_pad_column_read", "dense_1_reshape_channel_major",
           "convt0_border_tap_dropped", "convt0_phases_exchanged", "convt1_acc_k_not_undone", "convt4_two_channels_exchanged", "convt3_taps_transposed",
           "ring_row_one_lap_late", "outconv_reads_neighbour_top", "outconv_reads_neighbour_bottom", "outconv_reads_neighbour_left",
           "outconv_reads_neighbour_right", "outconv_left_granule_tap_dropped", "last_row_from_next_sample")


# ------------------------------------------------------------------------------------------------------------------------
# inputs and affines
# ------------------------------------------------------------------------------------------------------------------------
def _samples():
    rng = np.random.default_rng(4711)
    return rng.choice([0.0, 4.0, 5.0, 6.0, 7.0], p=[0.24, 0.19, 0.19, 0.19, 0.19], size=(8, 10, 10, 1))


def order(n):
    """Which of the 8 samples stands at place i of a batch of n: the first 8 in order, then a fixed non-periodic sequence in which
    no sample follows itself, so that both sides of every sample seam differ."""
    idx = list(range(min(n, 8)))
    rng = np.random.default_rng(815)
    while len(idx) < n:
        c = int(rng.integers(8))
        if c != idx[-1]:
            idx.append(c)
    return np.array(idx)


def inputs(n):
    """(n, 10, 10, 1) integer fields in {0} | [4, 7] (a quarter zeros, so that which elements a layer kills differs from sample to
    sample): 8 distinct samples in the order `order(n)`."""
    return _samples()[order(n)]


def in_affine(n):
    """(mean, std) rows, integer mean and power-of-two std, a different row for neighbouring samples, + the raw input that they
    standardise to inputs(n): (x - m) / s, x (1 / s) - m / s and the fused form are all exact in float32."""
    i = np.arange(n)
    mean = ((i * 5) % 7 - 3).astype(np.float32)
    std = np.array([0.5, 2.0, 0.25, 4.0, 1.0], np.float32)[i % 5]
    raw = (inputs(n) * std.reshape(-1, 1, 1, 1).astype(np.float64) + mean.reshape(-1, 1, 1, 1)).astype(np.float32)
    return np.stack([mean, std], 1), raw


def out_affine(n):
    """(mean, std) rows for y * std + mean: integer mean, std a power of two, so that the product and the sum are integers (or
    quarter-integers) below 2^24 whichever way they are fused."""
    i = np.arange(n)
    mean = ((i * 3) % 11 - 5).astype(np.float32)
    std = np.array([2.0, 0.5, 4.0, 1.0, 0.25], np.float32)[i % 5]
    return np.stack([mean, std], 1)


def apply_out_affine(y, aff):
    return y * aff[:, 1].astype(np.float64).reshape(-1, 1, 1, 1) + aff[:, 0].astype(np.float64).reshape(-1, 1, 1, 1)


def round_bf16(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def expected_output(y, kind):
    """The stated value of a float32 / bfloat16 / float16 output: the exact field, rounded to nearest even ONCE (the float32 result
    is exact, so the two roundings of a kernel that goes through float32 are one)."""
    y32 = np.asarray(y, np.float64).astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y), "the float32 result is not exact"
    if kind == "float32":
        return y32
    return round_bf16(y32) if kind == "bfloat16" else y32.astype(np.float16).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# the twin's weights: drawn per output channel, kept only where the conditions hold on every input (else redrawn, else a fallback
# that holds by construction)
# ------------------------------------------------------------------------------------------------------------------------
def _channel_ok(u, Jc, channels=None):
    """Per output (last axis): every pre-activation in {0 with J = 0} | [HI, VMAX] | (-inf, LO], and some element of its channel
    (the output itself, or output % channels) passes."""
    ok = (u >= HI) | (u <= LO) | ((u == 0) & (Jc == 0))
    red = tuple(range(u.ndim - 1))
    top = u.max(red)
    passes = top >= HI
    if channels is not None:
        passes = np.tile(top.reshape(-1, channels).max(0) >= HI, top.size // channels)
    return ok.all(red) & (top <= VMAX) & passes


def _draw(rng, layer, a_prev, propose, fallback, linear, attempts=6, extra=None):
    """K, J of one layer: `propose(rng, K, J, cos)` / `fallback(rng, K, J, cos)` fill the slices of the output channels `cos`;
    extra(u) -> a further condition per output channel."""
    shape = SHAPES[layer]
    cout = shape[2] if layer.startswith("conv2d_transpose") else shape[-1]
    K, J = np.zeros(shape), np.zeros(cout)
    todo = np.arange(cout)
    for attempt in range(attempts + 40):
        (propose if attempt < attempts else fallback)(rng, K, J, todo)
        u = linear(a_prev, K, J)
        ok = _channel_ok(u, J, channels=256 if layer == "dense_1" else None)
        if extra is not None:
            ok &= extra(u)
        todo = np.flatnonzero(~ok)
        if todo.size == 0:
            return K, J, u
    raise AssertionError(f"{layer}: the fallback does not meet the conditions for outputs {todo[:8]}")


def _pick(rng, p, size=None):
    vals, probs = zip(*p)
    return rng.choice(np.array(vals, dtype=np.float64), size=size, p=np.array(probs) / sum(probs))


def integer_twin(seed):
    """(K, J): {layer: float64 integer array} in Keras layouts, for the eleven compute layers.  Sparse: every (tap, output channel)
    has one or two readers -- weight 1 or 2 (pass), -10 or less (kill wherever that input is non-zero) -- and biases 0, [25, 30]
    (a floor where everything read is zero) or -132 / -141 (kept only where every value read is 0 or large enough to stay >= 25);
    the output convolution, which has no swish, is dense in +-{1, 2, 3}.  A draw is kept per output channel only if the conditions
    of check_conditions hold for it on all 8 samples and it passes somewhere; otherwise it is redrawn, at last from a fallback
    (one passing reader per tap, no bias) that meets them by construction."""
    if seed in _TWINS:
        return _TWINS[seed]
    assert seed in TWIN_SEEDS
    rng = np.random.default_rng(77000 + seed)
    x = _samples()
    K, J = {}, {}
    # conv2d: one passing tap (8 .. 10 on x in [4, 7]), in 40 % of the channels a killing tap in the row or column that the 'same'
    # padding reaches (-60: 70 - 240 <= -130), so that the channel passes only where that tap reads the padding
    border_taps = [(2, 0), (2, 1), (2, 2), (0, 2), (1, 2)]

    def conv1_fill(kill):
        def fill(rng, Kc, Jc, cos):
            for co in cos:
                Kc[:, :, 0, co] = 0
                Jc[co] = 0
                t = int(rng.integers(9))
                Kc[t // 3, t % 3, 0, co] = rng.integers(8, 11)
                if kill and rng.random() < 0.4:
                    a, b = border_taps[int(rng.integers(5))]
                    if (a, b) != (t // 3, t % 3):
                        Kc[a, b, 0, co] = -60
        return fill
    K["conv2d"], J["conv2d"], u = _draw(rng, "conv2d", x, conv1_fill(True), conv1_fill(False), lambda a, Kc, Jc: conv_same(a, Kc, Jc, 2))
    a = swish_sat(u)

    # conv2d_1: a reader on about a quarter of the taps
    def conv2_propose(rng, Kc, Jc, cos):
        for co in cos:
            Kc[:, :, :, co] = 0
            Jc[co] = _pick(rng, [(0, 0.8), (25, 0.1), (28, 0.1)])
            taps = np.flatnonzero(rng.random(9) < 0.25)
            if taps.size == 0:
                taps = np.array([4])
            for t in taps:
                Kc[t // 3, t % 3, int(rng.integers(64)), co] = _pick(rng, [(1, 0.8), (-10, 0.2)])

    def conv2_fallback(rng, Kc, Jc, cos):
        for co in cos:
            Kc[:, :, :, co] = 0
            Jc[co] = 0
            Kc[1, 1, int(rng.integers(64)), co] = 1
    K["conv2d_1"], J["conv2d_1"], u = _draw(rng, "conv2d_1", a, conv2_propose, conv2_fallback, lambda a, Kc, Jc: conv_same(a, Kc, Jc, 1), attempts=12)
    a = swish_sat(u).reshape(8, -1)

    # dense layers: a few readers per output
    def dense_fill(readers, biases, weights):
        def propose(rng, Kc, Jc, cos):
            live = np.flatnonzero(prev.max(0) > 0)
            for co in cos:
                Kc[:, co] = 0
                Jc[co] = _pick(rng, biases)
                r = int(rng.integers(1, readers + 1))
                Kc[rng.choice(live, size=r, replace=False), co] = _pick(rng, weights, size=r)

        def fallback(rng, Kc, Jc, cos):
            live = np.flatnonzero(prev.min(0) > 0) if (prev.min(0) > 0).any() else np.flatnonzero(prev.max(0) > 0)
            for co in cos:
                Kc[:, co] = 0
                Jc[co] = 0
                Kc[rng.choice(live), co] = 1
        return propose, fallback
    lin = lambda a, Kc, Jc: a @ Kc + Jc
    prev = a
    K["dense"], J["dense"], u = _draw(rng, "dense", a, *dense_fill(4, [(0, 0.7), (26, 0.15), (30, 0.15)], [(1, 0.7), (-10, 0.3)]), lin, attempts=12)
    prev = a = swish_sat(u)
    # latent_vector is linear, but dense_1 passes it on: it keeps to the same bands
    K["latent_vector"], J["latent_vector"], u = _draw(rng, "latent_vector", a, *dense_fill(3, [(0, 0.6), (25, 0.2), (29, 0.2)], [(1, 0.8), (2, 0.2)]), lin,
                                                      attempts=12)
    prev = a = u
    assert (a >= 0).all()

    # dense_1: one reader per output (pass, doubled, or killing under a bias that then shows only where the latent is 0) or a bias alone
    def d1_propose(rng, Kc, Jc, cos):
        m = cos.size
        Kc[:, cos] = 0
        Jc[cos] = _pick(rng, [(0, 0.6)] + [(j, 0.4 / 32) for j in range(32, 64)], size=m)
        w = _pick(rng, [(1, 0.6), (2, 0.1), (-10, 0.15), (0, 0.15)], size=m)
        w[(w == 0) & (Jc[cos] == 0)] = 1
        Kc[rng.integers(50, size=m), cos] = w

    def d1_fallback(rng, Kc, Jc, cos):
        Kc[:, cos] = 0
        Jc[cos] = 40 + cos % 16
    K["dense_1"], J["dense_1"], u = _draw(rng, "dense_1", a, d1_propose, d1_fallback, lin, attempts=4)
    a = swish_sat(u).reshape(8, 12, 12, 256)

    # ConvT#0 (3x3, stride 2): output pixels (even, even) sum up to four taps, (even, odd) and (odd, even) two, (odd, odd) one
    groups = [[(0, 0), (0, 2), (2, 0), (2, 2)], [(0, 1), (2, 1)], [(1, 0), (1, 2)], [(1, 1)]]

    def t0_propose(rng, Kc, Jc, cos):
        for co in cos:
            Kc[:, :, co, :] = 0
            Jc[co] = _pick(rng, [(0, 0.7), (25, 0.15), (27, 0.15)])
            for g in groups:
                main = int(rng.integers(len(g)))
                for i, (ta, tb) in enumerate(g):
                    if i == main:      # (the one-tap phase may be a killed one: the channel passes in the other three)
                        Kc[ta, tb, co, int(rng.integers(256))] = -10 if len(g) == 1 and rng.random() < 0.2 else 1
                    elif rng.random() < 0.35:
                        Kc[ta, tb, co, int(rng.integers(256))] = _pick(rng, [(-10, 0.7), (1, 0.3)])

    def t0_fallback(rng, Kc, Jc, cos):
        for co in cos:
            Kc[:, :, co, :] = 0
            Jc[co] = 0
            for g in groups:
                ta, tb = g[int(rng.integers(len(g)))]
                Kc[ta, tb, co, int(rng.integers(256))] = 1
    K["conv2d_transpose"], J["conv2d_transpose"], u = _draw(rng, "conv2d_transpose", a, t0_propose, t0_fallback, lambda a, Kc, Jc: convt_valid(a, Kc, Jc),
                                                            attempts=10)
    a = swish_sat(u)

    # ConvT#1 .. #4 (2x2, stride 2): one tap per output pixel
    def t_propose(rng, Kc, Jc, cos):
        cin = Kc.shape[3]
        for co in cos:
            Kc[:, :, co, :] = 0
            Jc[co] = _pick(rng, [(0, 0.6), (25, 0.1), (30, 0.1), (-132, 0.1), (-141, 0.1)])
            for ta in range(2):
                for tb in range(2):
                    # (ConvT#4's own reader always passes: a (phase, channel) of the last activation that is zero everywhere would hide the
                    # output convolution's weights for it, whose packed order is keyed by the row's parity and the column mod 8)
                    Kc[ta, tb, co, int(rng.integers(cin))] = _pick(rng, [(1, 0.7), (2, 0.1), (-10, 0.2)] if cin > 16 else [(1, 0.8), (2, 0.2)])
                    if rng.random() < 0.2:
                        Kc[ta, tb, co, int(rng.integers(cin))] = -16

    def t_fallback(rng, Kc, Jc, cos):
        cin = Kc.shape[3]
        for co in cos:
            Kc[:, :, co, :] = 0
            Jc[co] = 0
            for ta in range(2):
                for tb in range(2):
                    Kc[ta, tb, co, int(rng.integers(cin))] = 1
    for i in range(1, 5):
        name = f"conv2d_transpose_{i}"
        # what the output convolution reads passes somewhere at every (row % 2, column % 8) of every channel (see t_propose)
        cells = (lambda u: np.all([u[:, ra::2, cb::8].max((0, 1, 2)) >= HI for ra in range(2) for cb in range(8)], 0)) if i == 4 else None
        K[name], J[name], u = _draw(rng, name, a, t_propose, t_fallback, lambda a, Kc, Jc: convt_valid(a, Kc, Jc), attempts=8, extra=cells)
        a = swish_sat(u)
    K["output_image_400"] = (rng.choice([-1.0, 1.0], size=(3, 3, 8, 1)) * rng.integers(1, 4, size=(3, 3, 8, 1))).astype(np.float64)
    J["output_image_400"] = rng.integers(-50, 51, size=1).astype(np.float64)
    for d in (K, J):
        for v in d.values():
            v.setflags(write=False)
    _TWINS[seed] = (K, J)
    return K, J


_TWINS = {}


def encode(K, J, encoding):
    """-> (enc_weights, dec_weights) as SRModel.from_weights takes them, float32."""
    assert encoding in ("scaled", "plain")
    enc, dec = {}, {}
    for name in LAYERS:
        sk, sj = SCALED[name] if encoding == "scaled" else ("", "")
        f = lambda v, s: (v / LOG2E if s == "/" else v * LOG2E if s == "*" else v).astype(np.float32)
        d = enc if name in ENCODER else dec
        d[f"{name}/kernel"], d[f"{name}/bias"] = f(K[name], sk), f(J[name], sj)
    return enc, dec


# ------------------------------------------------------------------------------------------------------------------------
# the conditions the exactness argument rests on
# ------------------------------------------------------------------------------------------------------------------------
def linear(name, a, Kn, Jn):
    """The linear part of layer `name` on its input activation a (as the previous layer left it)."""
    n = a.shape[0]
    if name == "conv2d":
        return conv_same(a, Kn, Jn, 2)
    if name == "conv2d_1":
        return conv_same(a, Kn, Jn, 1)
    if name in ("dense", "latent_vector", "dense_1"):
        return a.reshape(n, -1) @ Kn + Jn
    if name == "output_image_400":
        return output_conv(a, Kn, Jn)
    return convt_valid(a.reshape(n, 12, 12, 256) if name == "conv2d_transpose" else a, Kn, Jn)


def _abs_sums(K, J, acts, x):
    """Per layer, sum |K| |u| + |J| per output element."""
    ins = [np.abs(x)] + [np.abs(a) for a in acts[:-1]]
    return [linear(name, a, np.abs(K[name]), np.abs(J[name])) for name, a in zip(LAYERS, ins)]


def oracle_bound(K, J, x, acts, pre, S, encoding):
    """Per layer, a bound per element on |float64 oracle's activation - the integer model's|, in the integer domain, propagated
    through the network of absolute values: E_pre = sum |K| E_in + r S, with r = 2^-24 for the float32-rounded kernel and bias of the
    scaled encoding (2^-50 for the float64 arithmetic alone in the plain one), and behind a swish E = 1.1 E_pre + |u| 2^-25
    (|swish'| <= 1.1; at u >= 25 the true swish is u sigma(u ln 2) >= u (1 - 2^-25), at u <= -130 it is below |u| 2^-130, at 0 it is 0).
    Doubled for the second-order terms."""
    r = 2.0 ** -24 if encoding == "scaled" else 2.0 ** -50
    E = np.zeros_like(np.asarray(x, np.float64))
    out = []
    for name, u, s in zip(LAYERS, pre, S):
        E = linear(name, E, np.abs(K[name]), np.zeros_like(J[name])) + r * s
        if SWISH[name]:
            E = 1.1 * E + np.abs(u) * 2.0 ** -25
        out.append(2 * E)
    return out


def check_conditions(K, J, x):
    """Asserts conditions 1-3 of the module docstring's argument on the inputs x, and returns (y, acts, pre, S)."""
    y, acts, pre = forward(K, J, x, return_all=True, return_pre=True)
    S = _abs_sums(K, J, acts, x)
    for name, u, a, s in zip(LAYERS, pre, acts, S):
        assert np.array_equal(u, np.rint(u)) and np.array_equal(K[name], np.rint(K[name])) and np.array_equal(J[name], np.rint(J[name])), f"{name}: not integers"
        assert np.abs(K[name]).max() <= 256, f"{name}: a weight above 256 is not exact in 16 bits"
        if SWISH[name]:
            # 1. every swish pre-activation is 0 (not by cancellation against a scaled bias / scaled conv1 weight), >= 25 or <= -130
            zero_ok = (s == 0) if name == "conv2d" else np.broadcast_to(J[name] == 0, u.shape[-1:])
            bad = ~((u >= HI) | (u <= LO) | ((u == 0) & zero_ok))
            assert not bad.any(), f"{name}: {int(bad.sum())} pre-activations in the forbidden band, first at {tuple(np.argwhere(bad)[0])}: {u[bad][0]}"
        # 2. every stored activation is exact in bf16 (the tighter kind) -- and in f16
        if name != "output_image_400":
            assert np.array_equal(round_bf16(a.astype(np.float32)).astype(np.float64), a), f"{name}: a stored activation is not exact in bf16"
            assert np.array_equal(a.astype(np.float16).astype(np.float64), a), f"{name}: a stored activation is not exact in f16"
        # 3. every partial sum is an integer below 2^24 whatever the order
        assert s.max() < 2 ** 24, f"{name}: sum |K u| + |J| reaches {s.max()}"
    return y, acts, pre, S


def check_affines(n):
    """Condition 4: the affines are exact in float32 whichever way a kernel evaluates them."""
    aff, raw = in_affine(n)
    m, s = aff[:, 0].reshape(-1, 1, 1, 1), aff[:, 1].reshape(-1, 1, 1, 1)
    want = inputs(n)
    one = np.float32(1)
    for got in ((raw - m) / s, (raw - m) * (one / s), raw * (one / s) - m / s, raw * (one / s) + (-m) * (one / s)):
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    assert len({tuple(r) for r in aff[:min(n, 5)]}) == min(n, 5) and all(tuple(aff[i]) != tuple(aff[i + 1]) for i in range(n - 1))
    out = out_affine(n)
    assert all(tuple(out[i]) != tuple(out[i + 1]) for i in range(n - 1))
    return aff, raw, out


def check_out_affine_exact(y, aff):
    """y * std + mean in float32, as two roundings and as one fma, is the exact value."""
    exact = apply_out_affine(y, aff)
    y32 = y.astype(np.float32)
    two = (y32 * aff[:, 1].reshape(-1, 1, 1, 1)) + aff[:, 0].reshape(-1, 1, 1, 1)
    assert two.dtype == np.float32 and np.array_equal(two.astype(np.float64), exact) and np.abs(exact).max() < 2 ** 24
    assert np.array_equal(exact * 4, np.rint(exact * 4))
    return exact


def richness(K, J, x, y, acts, pre):
    """-> list of the richness conditions that do NOT hold (empty = fine)."""
    miss = []
    kills = [name for name, u in zip(LAYERS, pre) if SWISH[name] and (u <= LO).any()]
    passes = [name for name, u in zip(LAYERS, pre) if SWISH[name] and (u >= HI).any()]
    if len(kills) < 9 or len(passes) < 9:
        miss.append(f"kills in {kills}, passes in {passes}: not in all nine swish layers")
    a1 = acts[0]       # conv1: stride 2 on 10 rows pads after -- a channel whose passing tap is in row 2 is zero in output row 4 only
    if not any((a1[:, 4, :, c] == 0).all() and (a1[:, :4, :, c] > 0).any() for c in range(64)):
        miss.append("no conv2d channel is zero exactly where the 'same' padding is read")
    t0 = acts[5]       # ConvT#0: a border row or column that only one tap row / column reaches
    if not any(((t0[:, 0, :, c] == 0).all() or (t0[:, 24, :, c] == 0).all() or (t0[:, :, 0, c] == 0).all() or (t0[:, :, 24, c] == 0).all()) and
               (t0[:, 1:24, 1:24, c] > 0).any() for c in range(128)):
        miss.append("no ConvT#0 channel has a zero border phase")
    f = y[..., 0]
    for r in range(400):
        if len({f[s, r].tobytes() for s in range(f.shape[0])}) != f.shape[0]:
            miss.append(f"two samples share output row {r}")
            break
    if (f[:, 1:] == f[:, :-1]).all(2).any():
        miss.append("an output row equals its neighbour")
    if (f[:, :, 1:] == f[:, :, :-1]).all(1).any():
        miss.append("an output column equals its neighbour")
    t4 = acts[9]       # what the output convolution reads: every channel at every (row % 2, column % 8), the key of its packed weights
    hidden = [(a, b, c) for a in range(2) for b in range(8) for c in range(8) if not t4[:, a::2, b::8, c].any()]
    if hidden:
        miss.append(f"ConvT#4's output is zero everywhere at (row % 2, column % 8, channel) = {hidden[:6]} ({len(hidden)} in all)")
    for name, a in zip(LAYERS, acts):
        dead = np.flatnonzero(~(a.reshape(-1, a.shape[-1]) != 0).any(0)) if name != "dense_1" else np.flatnonzero(~(a.reshape(-1, 256) != 0).any(0))
        if dead.size:
            miss.append(f"{name}: output channels {dead[:8]} are zero everywhere")
    return miss


def k_steps(K):
    """{name of an MFMA k-step: whether it carries a non-zero weight for some output}, read from operand_pack.cpp: a_frags' KS per
    layer (32x32x16: 16 k per step, 16x16x32: 32), dense's 100 steps, ConvT#0's 256-wide tap stages in steps of 16, and every
    (tap, input channel) of the output convolution."""
    out = {}
    nz = lambda a: bool((a != 0).any())
    k1 = K["conv2d_1"].reshape(576, 128)                       # k = tap 64 + ci; a_frags(32, 4, 36)
    for s in range(36):
        out[f"conv2d_1 k-step {s}"] = nz(k1[16 * s:16 * s + 16])
    for s in range(100):                                       # a_frags(16, 8, 100)
        out[f"dense k-step {s}"] = nz(K["dense"][32 * s:32 * s + 32])
    for s in range(4):                                         # a_frags(16, 4, 4)
        out[f"latent_vector k-step {s}"] = nz(K["latent_vector"][32 * s:32 * s + 32])
    for s in range(4):                                         # the latent vector zero-padded to 64: columns 48, 49 are all of step 3
        out[f"dense_1 k-step {s}"] = nz(K["dense_1"][16 * s:16 * s + 16])
    for a in range(3):                                         # ConvT#0: phase (a % 2, b % 2), tap stage (a // 2, b // 2) of 256 k
        for b in range(3):
            for s in range(16):
                out[f"conv2d_transpose tap ({a}, {b}) k-step {s}"] = nz(K["conv2d_transpose"][a, b, :, 16 * s:16 * s + 16])
    for i, cin in ((1, 128), (2, 64), (3, 32), (4, 16)):       # rows (tap, co), KS = Cin / 16
        for s in range(cin // 16):
            out[f"conv2d_transpose_{i} k-step {s}"] = nz(K[f"conv2d_transpose_{i}"][..., 16 * s:16 * s + 16])
    for a in range(3):
        for b in range(3):
            for c in range(8):
                out[f"output_image_400 tap ({a}, {b}) channel {c}"] = K["output_image_400"][a, b, c, 0] != 0
    return out


def unreached():
    """Names of the k-steps that no seed of TWIN_SEEDS reaches, in order."""
    reach = None
    for seed in TWIN_SEEDS:
        r = k_steps(integer_twin(seed)[0])
        reach = r if reach is None else {k: reach[k] or v for k, v in r.items()}
    return [k for k, v in reach.items() if not v]


# ------------------------------------------------------------------------------------------------------------------------
# where two fields differ: the message of every exact comparison
# ------------------------------------------------------------------------------------------------------------------------
def describe_mismatch(got, want, label=""):
    """None if equal as values (-0 == +0); else count, first (sample, row, column), bounding box, residues of the differing rows
    and columns mod 2, 4, 8, 16."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{label}: shape {got.shape} against {want.shape}"
    if np.array_equal(got, want):
        return None
    d = np.argwhere(got != want)
    first = tuple(int(v) for v in d[0])
    lines = [f"{label}: {len(d)} of {got.size} elements differ; first at {first}: got {got[first]!r}, want {want[first]!r}",
             "  bounding box: " + ", ".join(f"axis {ax} [{int(d[:, ax].min())}, {int(d[:, ax].max())}]" for ax in range(d.shape[1]))]
    if d.shape[1] >= 3:
        for what, ax in (("rows", 1), ("columns", 2)):
            lines.append(f"  differing {what} " + "; ".join(f"mod {m}: {sorted(set(int(v) for v in d[:, ax] % m))}" for m in (2, 4, 8, 16)))
    return "\n".join(lines)
