"""Per-position error statistics for the inference kernels (shared by test_error_maps.py and test_gpu_error_maps.py).

The whole-field relative L2 the parity modules assert dilutes a LOCAL defect (one row, one column, one lattice phase, one corner,
one channel) by sqrt(share of elements touched).  Here the error field of the device, dG = G - T (T: the float64 oracle), is
reduced per named POSITION CLASS (a boolean mask built from the kernels' geometry) and compared, class by class, with the error
dE = E - T of a CPU emulation E of the same arithmetic:

    rms_C(dG) <= margin_P * rms_C(dE)      for every class C,   and   max|dG| <= margin_P * max|dE|.

margin_P = 2 * spread_P, and spread_P is NOT read off the device: it is how far the class statistic moves between two legitimate
CPU evaluations of the same arithmetic (E and `second_emulation` below: float32 sequential accumulation in a permuted order over
taps and channels, exp2 / reciprocal a few ulp off), spread_P = max over classes of rms_C(dE') / rms_C(dE).  The factor 2 is for
the device's MFMA accumulation order, a third ordering neither emulation reproduces.  tests/test_error_maps.py recomputes
spread_P and fails if it drifts above the figures written here.

The measured figures (per precision and weight set, the batch, the date) stand next to SPREAD / MARGIN at the end of this file
and in DESIGN.md section 7.

Pure numpy; nothing here touches the GPU.
"""
from __future__ import annotations

import numpy as np

from oracle import sr_oracle as o
from oracle import sr_oracle_lowp as lp

LOG2E = lp.LOG2E
REF_N = 8            # samples of the reference batch (the oracle and the emulations need ~1 s per sample each)
KERAS_SEED = 5       # the one synth.keras_default_init seed of the second weight set (bf16 and the f32 family)
F32_FAMILY = ("fp32", "fp32_naive", "fp32x3")


def emu_kind(precision: str) -> str:
    return "f32" if precision in F32_FAMILY else precision


# ------------------------------------------------------------------------------------------------------------------------
# the fixed batch
# ------------------------------------------------------------------------------------------------------------------------
def fixed_batch(coarse_cases, lr_stats, n: int = REF_N, seed: int = 4242) -> np.ndarray:
    """(n,10,10,1) float32: real standardised coarse fields first (5 cases x u,v,p, taken with stride 4 so that every case and
    every component appears early), then standard-normal fields.  Two thirds real, one third normal; the same for every n."""
    real = []
    for case in coarse_cases.values():
        for c in ("u", "v", "p"):
            x = case[c].astype(np.float32)
            real.append(((x - lr_stats[c][0]) / lr_stats[c][1]).astype(np.float32))
    order = [(4 * i) % 15 for i in range(15)]
    n_real = min(n - n // 3, 15)
    xs = [real[i] for i in order[:n_real]]
    rng = np.random.default_rng(seed)
    xs += [rng.standard_normal((10, 10)).astype(np.float32) for _ in range(n - n_real)]
    return np.stack(xs)[..., None]


# ------------------------------------------------------------------------------------------------------------------------
# references: T (float64), E_P (the emulation the parity modules already use), and the pieces the planted defects re-run
# ------------------------------------------------------------------------------------------------------------------------
def oracle_f64(x, enc_w, dec_w):
    """T: float64 forward -> (y (N,400,400), {"t0","t1","t4"})."""
    z = o.encoder_forward(x, enc_w, np.float64)
    y, acts = o.decoder_forward(z, dec_w, np.float64, return_all=True)
    return y[..., 0], {"t0": acts[1], "t1": acts[2], "t4": acts[5]}


def emulation(x, enc_w, dec_w, kind):
    """E_P: bf16 / f16 -> oracle/sr_oracle_lowp.py; f32 -> the float32 oracle.  -> (y (N,400,400), {"t0","t1","t4"})."""
    if kind == "f32":
        z = o.encoder_forward(x, enc_w, np.float32)
        y, acts = o.decoder_forward(z, dec_w, np.float32, return_all=True)
        return y[..., 0], {"t0": acts[1], "t1": acts[2], "t4": acts[5]}
    y, acts = lp.superres_forward_lowp(x, enc_w, dec_w, kind, return_all=True)
    return y[..., 0], acts


def _quant(kind):
    """(weights of a swish consumer, weights of a linear consumer of scaled activations, stored swish output) of E_P."""
    if kind == "f32":
        f = lambda a: np.asarray(a, np.float32)
        return f, f, f
    rnd = lp.round_bf16 if kind == "bf16" else lp.round_f16
    q = lambda w: rnd(w).astype(np.float64)
    q_div = lambda w: LOG2E * rnd(np.asarray(w, np.float64) / LOG2E).astype(np.float64)
    rs = lambda a: rnd((a * LOG2E).astype(np.float32)).astype(np.float64) / LOG2E
    return q, q_div, rs


def convT_layer(h, dec_w, kind, i, kernel=None):
    """ConvT#i of E_P from the stored activation `h` of the layer before (sr_oracle_lowp.py:60-62); `kernel` overrides the weights."""
    q, _, rs = _quant(kind)
    name = o.DECODER_LAYERS[1 + i]
    w = dec_w[f"{name}/kernel"] if kernel is None else kernel
    return rs(o.conv2d_transpose(h, q(w), dec_w[f"{name}/bias"], 2, "valid", "swish"))


def tail_from_t1(t1, dec_w, kind):
    """ConvT#2..#4 of E_P from a (possibly tampered) ConvT#1 output -> t4 (N,400,400,8)."""
    h = t1
    for i in (2, 3, 4):
        h = convT_layer(h, dec_w, kind, i)
    return h


def output_conv(t4, dec_w, kind, pad_top="zero", pad_right="zero"):
    """The output 3x3 conv of E_P (sr_oracle_lowp.py:63) -> (N,400,400).  pad_* = "edge" replaces the zero padding row / column by
    a copy of the image's first row / last column (what a window that reads its neighbour instead of the zero block computes)."""
    _, q_div, _ = _quant(kind)
    w = q_div(dec_w["output_image_400/kernel"])
    b = dec_w["output_image_400/bias"]
    y = o.conv2d(t4, w, b, 1, "same", "linear")[..., 0]
    if pad_top == "edge":      # row 0 only: add the ky = 0 taps applied to row 0 itself
        xp = np.pad(t4[:, :1], ((0, 0), (0, 0), (1, 1), (0, 0)))
        y[:, 0] += sum(xp[:, 0, kx:kx + 400] @ w[0, kx].astype(t4.dtype) for kx in range(3))[..., 0]
    if pad_right == "edge":    # column 399 only: the kx = 2 taps applied to column 399 itself
        xp = np.pad(t4[:, :, -1:], ((0, 0), (1, 1), (0, 0), (0, 0)))
        y[:, :, 399] += sum(xp[:, ky:ky + 400, 0] @ w[ky, 2].astype(t4.dtype) for ky in range(3))[..., 0]
    return y


# ------------------------------------------------------------------------------------------------------------------------
# E'_P: the second emulation.  It differs from E_P only in what the device is allowed to differ in.
# ------------------------------------------------------------------------------------------------------------------------
_ULP = np.float32(2.0 ** -23)


def _perm(k):
    return np.random.default_rng(1000 + k).permutation(k)


def _mm_seq(a, w):
    """a (..., K) @ w (K, M) as a chain of float32 fused multiply-adds, ONE product at a time in a fixed permuted order of k: the
    exact product (float64 holds it) is added to the float32 accumulator and rounded once, which is what v_fma_f32 and the MFMA
    units do.  numpy's matmul, which E_P uses, runs the blocked / vectorised order of its BLAS, in float64 for the 16-bit kinds."""
    at = np.ascontiguousarray(np.moveaxis(np.asarray(a, np.float32), -1, 0)).astype(np.float64)
    w = np.asarray(w, np.float32).astype(np.float64)
    out = np.zeros(a.shape[:-1] + (w.shape[1],), np.float32)
    for k in _perm(a.shape[-1]):
        out = (out + at[k][..., None] * w[k]).astype(np.float32)
    return out


def _swish(pre, rng, scaled):
    """float32 swish as the device forms it: exp2 of the log2(e)-scaled argument, reciprocal, one product; the exp2 and the
    reciprocal each up to 2 ulp off (v_exp_f32 / v_rcp_f32 are specified to 1 ulp).  scaled: `pre` already carries the factor
    log2(e) (16-bit kinds) and so does the result; otherwise the argument is scaled here and the result is plain swish."""
    pre = np.asarray(pre, np.float32)
    arg = pre if scaled else pre * np.float32(LOG2E)
    with np.errstate(over="ignore"):
        e = np.exp2(-arg) * (np.float32(1) + 2 * _ULP * rng.uniform(-1, 1, pre.shape).astype(np.float32))
        s = (np.float32(1) / (np.float32(1) + e)) * (np.float32(1) + 2 * _ULP * rng.uniform(-1, 1, pre.shape).astype(np.float32))
    return (pre * s).astype(np.float32)


def second_emulation(x, enc_w, dec_w, kind):
    """E'_P -> (y (N,400,400), {"t0","t1"}).  Same roundings of weights and stored activations as E_P (16-bit kinds: activations
    stored as round(log2e * a), consumers of them use round(W) / round(W / log2e), dense_1 round(W * log2e)); float32 sequential
    accumulation in a permuted channel order, taps in reverse order, bias first, perturbed exp2 / reciprocal."""
    f32 = np.float32
    lowp = kind != "f32"
    rnd = (lp.round_bf16 if kind == "bf16" else lp.round_f16) if lowp else (lambda a: np.asarray(a, f32))
    L = f32(LOG2E)
    rng = np.random.default_rng(77)
    q = lambda w: rnd(np.asarray(w, f32))
    q_div = (lambda w: rnd((np.asarray(w, np.float64) / LOG2E).astype(f32))) if lowp else q
    q_mul = (lambda w: rnd((np.asarray(w, np.float64) * LOG2E).astype(f32))) if lowp else q
    # a stored swish activation s is log2e * a for the 16-bit kinds (the next layer's sum then arrives scaled for exp2) and a
    # itself for f32 (the argument of the exp2 is scaled inside _swish)
    bias = lambda b: (np.asarray(b, f32) * L) if lowp else np.asarray(b, f32)
    # the f32 family differs in the order of its sums only: its swish is the oracle's own, in float32
    act = (lambda pre: rnd(_swish(pre, rng, True))) if lowp else (lambda pre: o.silu(np.asarray(pre, f32)))

    def conv_same(a, w, b, stride):
        n, h, wd, _ = a.shape
        kh, kw, _, cout = w.shape
        oh, pt, pb = o.same_padding(h, kh, stride)
        ow, pl, pr = o.same_padding(wd, kw, stride)
        ap = np.pad(np.asarray(a, f32), ((0, 0), (pt, pb), (pl, pr), (0, 0)))
        out = np.zeros((n, oh, ow, cout), f32) + b
        for ky in reversed(range(kh)):
            for kx in reversed(range(kw)):
                out += _mm_seq(ap[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride], w[ky, kx])
        return out

    def conv_t(a, w, b):
        n, h, wd, _ = a.shape
        kh, kw, cout, _ = w.shape
        out = np.zeros((n, (h - 1) * 2 + kh, (wd - 1) * 2 + kw, cout), f32) + b
        for ky in reversed(range(kh)):
            for kx in reversed(range(kw)):
                out[:, ky:ky + (h - 1) * 2 + 1:2, kx:kx + (wd - 1) * 2 + 1:2] += _mm_seq(a, w[ky, kx].T)
        return out

    x = np.asarray(x, f32)
    # conv2d: f32 on the VALU with unrounded weights (sr_oracle_lowp.py:53)
    pre = conv_same(x, np.asarray(enc_w["conv2d/kernel"], f32), np.asarray(enc_w["conv2d/bias"], f32), 2)
    s = act(pre * L) if lowp else act(pre)
    s = act(conv_same(s, q(enc_w["conv2d_1/kernel"]), bias(enc_w["conv2d_1/bias"]), 1))
    s = act(_mm_seq(s.reshape(s.shape[0], -1), q(enc_w["dense/kernel"])) + bias(enc_w["dense/bias"]))
    z = rnd(_mm_seq(s, q_div(enc_w["latent_vector/kernel"])) + np.asarray(enc_w["latent_vector/bias"], f32))
    s = act(_mm_seq(z, q_mul(dec_w["dense_1/kernel"])) + bias(dec_w["dense_1/bias"])).reshape(-1, 12, 12, 256)
    acts = {}
    for i, name in enumerate(o.DECODER_LAYERS[1:6]):
        s = act(conv_t(s, q(dec_w[f"{name}/kernel"]), bias(dec_w[f"{name}/bias"])))
        if i < 2:
            acts[f"t{i}"] = (s.astype(np.float64) / LOG2E) if lowp else s
    y = conv_same(s, q_div(dec_w["output_image_400/kernel"]), np.asarray(dec_w["output_image_400/bias"], f32), 1)
    return y[..., 0], acts


# ------------------------------------------------------------------------------------------------------------------------
# position classes
# ------------------------------------------------------------------------------------------------------------------------
def output_classes(seg: int = 1, pool_rows: int = 1) -> dict:
    """name -> boolean mask over (400, 400) [row, col].  `seg` = the tail segmentation that ran (last_plan()["tail_seg"]);
    `pool_rows` > 1 pools the single-row / single-column catch-all classes in groups of that many."""
    H = 400
    r = np.arange(H)[:, None] * np.ones((1, H), int)
    c = np.arange(H)[None, :] * np.ones((H, 1), int)
    cl = {}
    # SAME padding of the 3x3 output conv: ring granules 0 and 51 of a plane (tail16_layout.h:3-4,16) left / right, the 16-byte
    # zero block (tail16_layout.h:22) and the `d_top` row pair (kernels_bf16.hip:558) above / below
    for name, m in (("row_0", r == 0), ("row_399", r == H - 1), ("col_0", c == 0), ("col_399", c == H - 1),
                    ("row_1", r == 1), ("row_398", r == H - 2), ("col_1", c == 1), ("col_398", c == H - 2)):
        cl["border/" + name] = m
    # the four corners as ONE class of four pixels: a single corner pixel is N values per class, and on N = 8 the ratio of two
    # correct float32 evaluations already reaches 3.0 there (margin 6); a lone wrong pixel is the worst-element check's business
    cl["corner/all_four"] = ((r == 0) | (r == H - 1)) & ((c == 0) | (c == H - 1))
    # one 50x50 pixel expands to 8x8; strips are 8 rows (kernels_bf16.hip:288); ring planes are x & 7 (tail16_layout.h:26)
    for k in range(8):
        cl[f"lattice/row%8=={k}"] = r % 8 == k
        cl[f"lattice/col%8=={k}"] = c % 8 == k
    # the 2x2 taps of ConvT#2..#4 (sr_oracle.py:61-64: kernels (2,2,..), stride 2)
    for mod in (2, 4):
        for k in range(mod):
            cl[f"lattice/row%{mod}=={k}"] = r % mod == k
            cl[f"lattice/col%{mod}=={k}"] = c % mod == k
    # D(g) covers rows 8g-1 .. 8g+6 (kernels_bf16.hip:406,535): the strip seam lies between rows 8g+6 and 8g+7
    cl["seam/strip_last_row_8g+6"] = r % 8 == 6
    cl["seam/strip_first_row_8g+7"] = r % 8 == 7
    if seg > 1:
        # segments of 50 / seg strips, each after one warm-up strip (kernels_bf16.hip:409-411); seams at multiples of 400 / seg rows
        L = H // seg
        seams = np.arange(1, seg) * L
        for d in (-2, -1, 0, 1):
            cl[f"seam/segment_row{d:+d}"] = np.isin(r, seams + d)
        first = (np.arange(seg) * L)[:, None] + np.arange(-1, 7)[None, :]          # rows 8g-1 .. 8g+6 of a segment's first strip
        cl["seam/segment_first_strip"] = np.isin(r, first[first >= 0])
    # D items are 2x8-pixel tiles read 8 apart in x, 16 tiles per item (tail16_layout.h:5-6)
    for k in range(50):
        cl[f"band8/cols_{8 * k}-{8 * k + 7}"] = c // 8 == k
    for k in range(4):
        cl[f"band128/cols_{128 * k}-{min(128 * k + 127, H - 1)}" + ("_last" if k == 3 else "")] = c // 128 == k
    # the catch-all for geometry nobody listed
    for k in range(0, H, pool_rows):
        tag = f"{k}" if pool_rows == 1 else f"{k}-{k + pool_rows - 1}"
        cl[f"single/row_{tag}"] = (r >= k) & (r < k + pool_rows)
        cl[f"single/col_{tag}"] = (c >= k) & (c < k + pool_rows)
    return cl


def grid_classes(n: int, H: int, W: int, stacked: int = 1, pool: int = 1, sample_group: int = 1) -> dict:
    """`output_classes` for any output size, with the batch as an axis: name -> boolean mask over (n, H, W) [sample, row, col], for
    the graphs of tests/any16_cases.py (`class_rms` / `class_check` then take the error field as d[None]).  No class knows a
    kernel's tiling; they follow what every stride-2 transposed convolution + 3x3 'same' output convolution has:
      border/   the two outermost rows and columns on each side (the zero padding of the output convolution, the crop);
      corner/   the four corners as one class;
      lattice/  row % 2 x col % 2, the output phases of the last transposed convolution, and % 4 where `stacked` = 2 of them;
      single/   every row and column, pooled in groups of `pool`;
      sample/   groups of `sample_group` consecutive samples: the last one rides in the GEMMs' last, partial 128-row tile."""
    r = np.arange(H)[:, None] * np.ones((1, W), int)
    c = np.arange(W)[None, :] * np.ones((H, 1), int)
    cl = {}
    for k in range(min(2, H // 2)):
        cl[f"border/row_{k}"], cl[f"border/row_{H - 1 - k}"] = r == k, r == H - 1 - k
    for k in range(min(2, W // 2)):
        cl[f"border/col_{k}"], cl[f"border/col_{W - 1 - k}"] = c == k, c == W - 1 - k
    cl["corner/all_four"] = ((r == 0) | (r == H - 1)) & ((c == 0) | (c == W - 1))
    for mod in (2, 4)[:stacked]:
        for a in range(mod):
            for b in range(mod):
                cl[f"lattice/row%{mod}=={a},col%{mod}=={b}"] = (r % mod == a) & (c % mod == b)
    for k in range(0, H, pool):
        cl[f"single/row_{k}" if pool == 1 else f"single/row_{k}-{min(k + pool, H) - 1}"] = (r >= k) & (r < k + pool)
    for k in range(0, W, pool):
        cl[f"single/col_{k}" if pool == 1 else f"single/col_{k}-{min(k + pool, W) - 1}"] = (c >= k) & (c < k + pool)
    cl = {k: np.broadcast_to(m, (n, H, W)) for k, m in cl.items()}
    s = np.arange(n)[:, None, None] * np.ones((1, H, W), int)
    starts = list(range(0, n - n % sample_group, sample_group)) or [0]      # a short remainder joins the last group
    for k, hi in zip(starts, starts[1:] + [n]):
        cl[f"sample/{k}" if hi - k == 1 else f"sample/{k}-{hi - 1}"] = (s >= k) & (s < hi)
    return cl


def activation_classes(h: int, w: int, ch: int) -> dict:
    """name -> boolean mask over (h, w, ch) for an intermediate activation (ConvT#1: 50x50x64; ConvT#0: 25x25x128)."""
    r = np.arange(h)[:, None, None] * np.ones((1, w, ch), int)
    c = np.arange(w)[None, :, None] * np.ones((h, 1, ch), int)
    k = np.arange(ch)[None, None, :] * np.ones((h, w, 1), int)
    cl = {}
    # fragment packing / the host-permuted k order hit channels (kernels_mid16.hip, kernels_enc16.hip)
    for i in range(ch):
        cl[f"channel/{i}"] = k == i
    for g in (8, 16, 32):
        for i in range(ch // g):
            cl[f"channels{g}/{g * i}-{g * i + g - 1}"] = k // g == i
    for name, m in (("row_0", r == 0), (f"row_{h - 1}", r == h - 1), ("col_0", c == 0), (f"col_{w - 1}", c == w - 1)):
        cl["border/" + name] = m
    # the output phases of a stride-2 transposed conv (ConvT#0: 4 / 2 / 2 / 1 taps, kernels_mid16.hip)
    for a in range(2):
        for b in range(2):
            cl[f"phase/row%2=={a},col%2=={b}"] = (r % 2 == a) & (c % 2 == b)
    for i in range(h):
        cl[f"single/row_{i}"] = r == i
    for i in range(w):
        cl[f"single/col_{i}"] = c == i
    return cl


# ------------------------------------------------------------------------------------------------------------------------
# the statistic
# ------------------------------------------------------------------------------------------------------------------------
def class_rms(d, classes) -> dict:
    """d (N, *S) error fields -> {class: rms over the N samples and the class's elements}."""
    d = np.asarray(d, np.float64)
    sq = (d * d).sum(0)
    n = d.shape[0]
    return {name: float(np.sqrt(sq[m].sum() / (n * int(m.sum())))) for name, m in classes.items()}


def spread(dE2, dE, classes):
    """max over classes of rms_C(dE') / rms_C(dE), the class it sits in, and the ratio of the worst single elements."""
    r2, r1 = class_rms(dE2, classes), class_rms(dE, classes)
    ratios = {k: r2[k] / max(r1[k], 1e-300) for k in classes}
    worst = max(ratios, key=ratios.get)
    return ratios[worst], worst, float(np.abs(dE2).max() / np.abs(dE).max())


def class_check(dG, dE, classes, margin, label=""):
    """-> (ok, report, names of the ten worst classes, worst ratio).  ok = every class AND the worst single element inside margin."""
    rg, re_ = class_rms(dG, classes), class_rms(dE, classes)
    ratios = {k: rg[k] / max(re_[k], 1e-300) for k in classes}
    ten = sorted(ratios, key=ratios.get, reverse=True)[:10]
    mg, me = float(np.abs(dG).max()), float(np.abs(dE).max())
    at = tuple(int(i) for i in np.unravel_index(int(np.abs(dG).argmax()), np.shape(dG)))
    failed = [k for k in classes if ratios[k] > margin]
    ok = not failed and mg <= margin * me
    lines = [f"[{label}] {len(classes)} classes, margin {margin:.2f}: {len(failed)} over; worst ratio {ratios[ten[0]]:.3f}",
             f"  worst element |dG| {mg:.3e} at (sample, ...) {at} vs emulation max |dE| {me:.3e} (ratio {mg / max(me, 1e-300):.3f})"]
    lines += [f"  {k:34s} rms dG {rg[k]:.3e}  rms dE {re_[k]:.3e}  ratio {ratios[k]:.3f}" for k in ten]
    return ok, "\n".join(lines), ten, ratios[ten[0]]


# ------------------------------------------------------------------------------------------------------------------------
# measured on the CPU, 2026-10-16, batch fixed_batch(n=8); tests/test_error_maps.py::test_margins_are_calibrated_on_two_emulations
# recomputes every figure and fails if one drifts above SPREAD.  max over classes of rms_C(dE') / rms_C(dE) | worst-element ratio:
#                 trained multiBC encoder + synthetic_decoder(1)                   keras_default_init(5)
#   bf16   output 1.0174 | 1.0000   ConvT#1 1.0012   ConvT#0 1.0038        output 1.0144 | 1.0513   ConvT#1 1.0012   ConvT#0 1.0014
#   f16    output 1.0372 | 1.0000   ConvT#1 1.0073   ConvT#0 1.0164        (not run: f16 denormals, test_gpu_parity_fp32.py:175)
#   f32    output 1.5905 | 1.3616  (single rows / columns pooled in pairs)   output 1.9434 | 1.7690
# f32: single rows / columns are pooled in pairs because unpooled the spread is 1.68 and 2.04, i.e. a margin of 4.08, and no
# margin above 4 is accepted.  The f32 figure is mostly systematic: a sequential chain over K = 3200 / 1152 products loses about
# twice what the blocked sums of the BLAS lose (whole-field 1.2e-6 against 6.0e-7), and the device's f32 kernels are chains of that
# kind; E for the f32 family stays the float32 oracle on the BLAS, the reference the f32 parity tests already use.
# SPREAD: bf16 and f16 are the largest figure of their row rounded up with about 0.02 to spare (another BLAS kernel order flips
# other 16-bit roundings); f32 is rounded up to the cap (1.9434 -> 2.0, margin 4.0).
# For the record (NOT the source of any bound): worst class ratio rms_C(dG) / rms_C(dE) the MI355X showed on 2026-10-16 --
#   bf16 1.009 (every tail kernel / batch size / segmentation), 1.014 on keras_default_init(5), ConvT#1 / ConvT#0 1.002;
#   f16 1.043, ConvT#1 / ConvT#0 1.007;  fp32 2.02, fp32_naive 1.99, fp32x3 1.72, fp32 on keras_default_init(5) 1.21.
# ------------------------------------------------------------------------------------------------------------------------
SPREAD = {"bf16": 1.07, "f16": 1.05, "f32": 2.0}
MARGIN = {k: 2.0 * v for k, v in SPREAD.items()}          # bf16 2.14, f16 2.10, f32 4.0
POOL_ROWS = {"bf16": 1, "f16": 1, "f32": 2}


def margin(precision: str) -> float:
    return MARGIN[emu_kind(precision)]
