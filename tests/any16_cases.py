"""The case table of the generic 16-bit layer path (any16: enc16 -> gemm16 / gemm16n per layer -> outconv16), shared by
test_any16_cases.py (CPU) and test_gpu_any16_layers.py.

A case is a decoder behind encoder_10: dense_1, an optional further Dense, a Reshape, one or two stride-2 transposed
convolutions and the 3x3 'same' output convolution.  Every case is the smallest graph that reaches one branch of the 16-bit
kernels which the five family decoders never take (see `reaches`).  `gemm_ops` restates, from a case alone, which kernel and
which branch of it every GEMM op takes (build_plan / plan16 / plan_chunk16 of csrc/; test_any16_cases.py holds it against the
library's own plan), and
test_any16_cases.py::test_table_reaches_every_branch_of_the_16bit_layer_kernels fails if a branch is reached by no case.

Three weight sets per case:
  random_decoder   variance-preserving seeded weights, the rule of family.synthetic_decoder_weights (error statistics)
  integer_twin     every layer linear, dense_1 with a zero kernel, sparse small-integer weights: every intermediate is an integer
                   of magnitude <= 256, exact in bf16 and f16, so the device must equal float64 bit for bit (geometry)
  twin_reference   the twin once more in plain integer numpy, with the planted geometric defects the CPU tests use to show
                   that the bit-for-bit comparison would see them

Pure numpy; nothing here touches the GPU.

Measured on the CPU, 2026-10-19, batch error_maps.fixed_batch(n = batch_size(case)), weights random_decoder(case):
spread = max over grid_classes of rms_C(E' - T) / rms_C(E - T) | ratio of the worst single elements (E: family_ref.
forward_specs_lowp, E': family_ref.forward_specs_lowp2, T: float64).  test_any16_cases.py::test_spreads_are_calibrated_on_two_
emulations recomputes every figure and fails if one drifts above SPREAD[kind] below; the GPU margin is 2 x SPREAD[kind].
  case                 n   output       bf16                f16
  narrow16_k2         67    6 x  8   1.0199 | 1.0000     1.0184 | 1.0000
  narrow16_k3same     67    6 x  8   1.0044 | 1.0000     1.0289 | 0.9999
  narrow32_k3valid    67    5 x  7   1.0167 | 1.0000     1.0318 | 0.9999
  narrow32_same_c48   67    8 x  8   1.0042 | 1.0000     1.0375 | 1.0006
  wide_1px           259    4 x  4   1.0900 | 1.0000     1.0687 | 1.0003
  bn64_k3valid        67    7 x  7   1.0402 | 1.0000     1.0254 | 1.0001
  k2_npad192          67    6 x 10   1.0195 | 1.0000     1.0404 | 1.0002
  n16_from64          67   10 x  6   1.0153 | 1.0000     1.0535 | 0.9902
  act_mix             67   12 x 16   1.0506 | 1.0000     1.0559 | 1.0000
  mid_dense_splitk    67    4 x  6   1.0252 | 1.0000     1.0269 | 1.0000
No pooling of single rows / columns was needed (POOL = 1): every figure is far below the cap of 2.0.
"""
from __future__ import annotations

import importlib
import math

import numpy as np

KINDS = ("bf16", "f16")
LATENT = 50

# id -> dense_1 activation, optional (dense_1 width, its activation is d1_act; second Dense's activation), reshape (h, w, c),
#       [(cout, k, 'same', activation)] of the stride-2 transposed convolutions, what the case is there for
CASES = {
    "narrow16_k2": dict(d1_act="swish", mid=None, reshape=(3, 4, 16), convts=[(16, 2, False, "swish")],
                        reaches="gemm16n CI=16, K=16 (one k-step), pixel-shuffle store"),
    "narrow16_k3same": dict(d1_act="swish", mid=None, reshape=(3, 4, 16), convts=[(16, 3, True, "swish")],
                            reaches="gemm16n phase ops with 1/2/2/4 taps, crop"),
    "narrow32_k3valid": dict(d1_act="swish", mid=None, reshape=(2, 3, 32), convts=[(16, 3, False, "swish")],
                             reaches="gemm16n 3x3 VALID, odd output 5x7"),
    "narrow32_same_c48": dict(d1_act="swish", mid=None, reshape=(4, 4, 32), convts=[(48, 3, True, "swish")],
                              reaches="outconv16 C=48, N=48 / Npad=64"),
    "wide_1px": dict(d1_act="swish", mid=None, reshape=(1, 1, 512), convts=[(256, 3, True, "swish"), (64, 2, False, "swish")],
                     reaches="gemm16 BN=128, one-pixel image, M < 32"),
    "bn64_k3valid": dict(d1_act="swish", mid=None, reshape=(3, 3, 128), convts=[(64, 3, False, "swish")],
                         reaches="gemm16 BN=64, outconv16 C=64, 7x7"),
    "k2_npad192": dict(d1_act="swish", mid=None, reshape=(3, 5, 64), convts=[(48, 2, False, "swish")],
                       reaches="gemm16 Npad=192, four phases of 48"),
    "n16_from64": dict(d1_act="swish", mid=None, reshape=(5, 3, 64), convts=[(16, 3, True, "swish")],
                       reaches="gemm16 N=16 < Npad=64, tall image"),
    "act_mix": dict(d1_act="linear", mid=None, reshape=(3, 4, 64), convts=[(32, 3, True, "linear"), (16, 2, False, "swish")],
                    reaches="q, q_mul, q_div weight scalings on the decoder side"),
    "mid_dense_splitk": dict(d1_act="swish", mid=(1024, "swish"), reshape=(2, 3, 64), convts=[(32, 2, False, "swish")],
                             reaches="Dense behind dense_1, split-K with its slab guard"),
}
TWIN_SEEDS = (0, 1, 2, 3)      # of the integer twin: over them every output-convolution tap and every input channel is non-zero
BATCHES = (1, 3, 130)          # the batch sizes of the bit-for-bit tests, + batch_size(case) of the statistics
# the largest spread of its kind in the table above, rounded up with about 0.02 to spare (error_maps.SPREAD's rule); the cap of
# error_maps.py holds: no spread above 2.0 (margin 4)
SPREAD = {"bf16": 1.11, "f16": 1.09}
POOL = {"bf16": 1, "f16": 1}   # single rows / columns pooled in groups of this many (error_maps.POOL_ROWS' rule)


def _family():
    return importlib.import_module("sr-for-cfd_amd.family")


def convt_out(size, k, same):
    return 2 * size if same else 2 * (size - 1) + k


def out_hw(case):
    h, w, _ = CASES[case]["reshape"]
    for _, k, same, _ in CASES[case]["convts"]:
        h, w = convt_out(h, k, same), convt_out(w, k, same)
    return h, w


def batch_size(case):
    """Samples of the statistics batch: every position class (the smallest are the four corners, a single row or column, and on
    4 x 4 a one-pixel phase of the % 4 lattice) holds at least 256 values over the batch; + 3 so that the batch is odd."""
    import error_maps as em
    cl = em.grid_classes(1, *out_hw(case), stacked=len(CASES[case]["convts"]))
    return -(-256 // min(int(m.sum()) for k, m in cl.items() if not k.startswith("sample/"))) + 3


def sample_group(case):
    """Consecutive samples per sample class: at least 256 values each."""
    h, w = out_hw(case)
    return -(-256 // (h * w))


def decoder_layers(case):
    """[(name, kind, shape, activation, extra)] of the decoder's weighted layers, in order; Conv2DTranspose kernels are
    (k, k, Cout, Cin), extra = 'same' for them."""
    c = CASES[case]
    h, w, ch = c["reshape"]
    out = []
    if c["mid"] is None:
        out.append(("dense_1", "dense", (LATENT, h * w * ch), c["d1_act"], None))
    else:
        width, act = c["mid"]
        out.append(("dense_1", "dense", (LATENT, width), c["d1_act"], None))
        out.append(("dense_2", "dense", (width, h * w * ch), act, None))
    for i, (cout, k, same, act) in enumerate(c["convts"]):
        out.append(("conv2d_transpose" if i == 0 else f"conv2d_transpose_{i}", "conv2d_transpose", (k, k, cout, ch), act, same))
        ch = cout
    out.append(("output_image", "conv2d", (3, 3, ch, 1), "linear", True))
    return out


def build_specs(case, enc_w, weights, all_linear=False):
    """`SRModel.from_layers` specs of encoder_10 + the case's decoder; weights = {name: (kernel, bias)}.  all_linear: every
    decoder layer without its activation (the integer twin)."""
    specs = _family().encoder_specs(enc_w, 10)
    for name, kind, shape, act, extra in decoder_layers(case):
        w, b = weights[name]
        act = "linear" if all_linear else act
        assert tuple(w.shape) == shape, (name, w.shape, shape)
        if kind == "dense":
            specs.append(dict(kind="dense", name=name, act=act, w=w, b=b))
        elif kind == "conv2d_transpose":
            if name == "conv2d_transpose":
                specs.append(dict(kind="reshape", name="reshape", shape=CASES[case]["reshape"]))
            specs.append(dict(kind="conv2d_transpose", name=name, k=shape[0], stride=2, same=extra, act=act, w=w, b=b))
        else:
            specs.append(dict(kind="conv2d", name=name, k=3, stride=1, same=True, act="linear", w=w, b=b))
    return specs


def random_decoder(case, seed=None, bias_scale=0.1):
    """family.synthetic_decoder_weights' rule on the case's shapes: uniform kernels of variance 2.4 / fan_eff (fan_eff counts the
    taps of a stride-2 transposed convolution that reach one output pixel: k k / 4), normal biases."""
    rng = np.random.default_rng(500 + list(CASES).index(case) if seed is None else seed)
    out = {}
    for name, kind, shape, act, extra in decoder_layers(case):
        tr = kind == "conv2d_transpose"
        fan_in = shape[0] if kind == "dense" else shape[0] * shape[1] * (shape[3] if tr else shape[2])
        fan_eff = fan_in / 4.0 if (tr and shape[0] == 2) else (fan_in / 2.25 if tr else fan_in)
        limit = math.sqrt(3.0 * 2.4 / fan_eff)
        out[name] = (rng.uniform(-limit, limit, size=shape).astype(np.float32),
                     (bias_scale * rng.standard_normal(shape[2] if tr else shape[-1])).astype(np.float32))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# which branch every GEMM op takes: the selection rules of csrc/, restated
# ------------------------------------------------------------------------------------------------------------------------
def _round_up(a, b):
    return -(-a // b) * b


def scaling(prev_act, act):
    """scale_w of operand_pack.cpp as the name of the emulation's rounding: a linear consumer of swish output holds
    round(W / log2e), a swish layer behind a linear one round(W log2e), everything else round(W)."""
    if prev_act == "swish" and act != "swish":
        return "q_div"
    if act == "swish" and prev_act != "swish":
        return "q_mul"
    return "q"


def gemm_ops(case, n):
    """The decoder's GEMM ops for a batch of n, in launch order, + the output convolution:
    [dict(layer, kernel, shape, CI, K, N, Npad, BN, taps, MH, MW, M, splitk, scaling)]."""
    c = CASES[case]
    ops = []
    prev_act = "linear"            # latent_vector
    h, w, _ = c["reshape"]
    for name, kind, shape, act, same in decoder_layers(case):
        sc = scaling(prev_act, act)
        prev_act = act
        new = []
        if kind == "dense":
            ci = 64 if name == "dense_1" else shape[0]       # dense_1 reads the latent vector zero-padded to 64 (plan16)
            assert ci % 64 == 0 and shape[1] % 64 == 0, "any16_plan: dense width"
            new.append(dict(shape="dense", CI=ci, K=ci, N=shape[1], taps=1, MH=1, MW=1))
        elif kind == "conv2d_transpose":
            k, _, cout, cin = shape
            assert cin % 16 == 0 and cout % 4 == 0, "any16_plan: channel counts"
            oh, ow = convt_out(h, k, same), convt_out(w, k, same)
            if k == 2:                                           # k == s: one pixel-shuffle op, N = s s Cout
                new.append(dict(shape="k2", CI=cin, K=cin, N=4 * cout, taps=1, MH=h, MW=w))
            else:                                                # up to four output phases, TY x TX taps each (build_plan)
                for py in range(2):
                    for px in range(2):
                        ty, tx = (k - py + 1) // 2, (k - px + 1) // 2
                        mh, mw = (oh - py + 1) // 2 if py < oh else 0, (ow - px + 1) // 2 if px < ow else 0
                        if mh and mw:
                            new.append(dict(shape="k3same" if same else "k3valid", CI=cin, K=ty * tx * cin, N=cout, taps=ty * tx, MH=mh, MW=mw))
            h, w = oh, ow
        else:
            assert shape[2] in (16, 32, 48, 64), "any16_plan: output convolution"
            ops.append(dict(layer=name, kernel="outconv16", shape="out", CI=shape[2], K=9 * shape[2], N=1, Npad=1, BN=0, taps=9, MH=h, MW=w,
                            M=n * h * w, splitk=False, scaling=sc))
        for d in new:
            narrow = d["CI"] % 64 != 0                           # any16_narrow
            d.update(layer=name, scaling=sc, kernel="gemm16n" if narrow else "gemm16", M=n * d["MH"] * d["MW"])
            d["Npad"] = _round_up(d["N"], 32 if narrow else 64)  # plan16
            d["BN"] = 32 if narrow else (128 if d["Npad"] % 128 == 0 else 64)   # gemm16: wide
            assert d["N"] % 4 == 0 and (narrow or d["K"] % 64 == 0), "any16_plan: GEMM shape"
            # plan_chunk16: layers with a 1x1 output (Dense) and a long K split it over up to 16 slabs, if the slabs the handle reserves
            # for a chunk of this size (16 x chunk x 128 f32) hold them.  One row per sample is not enough: wide_1px's phase ops have MH = MW = 1 and K = 2048 / 1024 too, and until
            # 2026-10-19 they took this branch, whose finish kernel stores row m at Y + m OC (found by test_gpu_any16_layers.py)
            splits = max(1, min(16, d["K"] // 256)) if (d["shape"] == "dense" and not narrow and d["K"] >= 1024) else 1
            d["splitk"] = splits > 1 and splits * d["M"] * d["Npad"] <= 16 * n * 128
            ops.append(d)
    return ops


# ------------------------------------------------------------------------------------------------------------------------
# the integer twin
# ------------------------------------------------------------------------------------------------------------------------
def _tap_shift(t):
    return 5 * t + 1       # 5 t mod 16 is different for t = 0 .. 8: the channel map differs for every tap at every Cin >= 16


def integer_twin(case, seed):
    """{name: (kernel, bias)} in float32, all integers: dense_1 = (0, seeded integers in [-7, 7]); a further Dense and the
    transposed convolutions one non-zero per output channel and tap, W[a, b, co, ci] = g[a, b] [ci == (co + 5 (3 a + b) + 1) % Cin],
    g in +-{1, 2, 3}, biases in [-1, 1]; the output convolution: channel c is read by seed c % 4 alone, at tap (c + 2 seed) % 9,
    with a weight in +-{1, 2}.  With at most 4 taps per output pixel in the first and one in the second transposed convolution:
    |activations| <= 7, 4 x 3 x 7 + 1 = 85, 3 x 85 + 1 = 256."""
    rng = np.random.default_rng(9000 + 10 * list(CASES).index(case) + seed)
    sign = lambda size: rng.choice([-1, 1], size=size)
    out = {}
    for name, kind, shape, act, extra in decoder_layers(case):
        if name == "dense_1":
            out[name] = (np.zeros(shape, np.float32), rng.integers(-7, 8, shape[1]).astype(np.float32))
        elif kind == "dense":
            w = np.zeros(shape, np.float32)
            co = np.arange(shape[1])
            w[(3 * co + 7) % shape[0], co] = sign(shape[1]) * rng.integers(1, 4, shape[1])
            out[name] = (w, rng.integers(-1, 2, shape[1]).astype(np.float32))
        elif kind == "conv2d_transpose":
            k, _, cout, cin = shape
            w = np.zeros(shape, np.float32)
            co = np.arange(cout)
            for a in range(k):
                for b in range(k):
                    w[a, b, co, (co + _tap_shift(3 * a + b)) % cin] = int(sign(None)) * int(rng.integers(1, 4))
            out[name] = (w, rng.integers(-1, 2, cout).astype(np.float32))
        else:
            C = shape[2]
            w = np.zeros(shape, np.float32)
            for c in range(seed % 4, C, 4):
                t = (c + 2 * seed) % 9
                w[t // 3, t % 3, c, 0] = int(sign(None)) * int(rng.integers(1, 3))
            out[name] = (w, rng.integers(-3, 4, 1).astype(np.float32))
    return out


TWIN_DEFECTS = ("crop_off_by_one", "border_tap_dropped", "phases_swapped", "taps_transposed", "channel_quad_shifted", "outconv_reads_edge")


def defect_applies(case, defect, layer):
    """layer: index of the transposed convolution the defect is planted in (ignored by the output convolution's)."""
    cout, k, same, _ = CASES[case]["convts"][layer]
    if defect == "crop_off_by_one":
        return k == 3 and same          # only a cropped layer has a crop offset
    if defect == "outconv_reads_edge":
        return layer == len(CASES[case]["convts"]) - 1
    return True


def twin_reference(case, weights, defect=None, layer=0):
    """The twin's decoder in integer numpy -> ((H, W) int64, the same for every sample: dense_1's kernel is zero; the largest
    |activation| handed from one layer to the next).  `defect`
    plants one geometric mistake of the kind a kernel can make in transposed convolution `layer` (or in the output convolution):
      crop_off_by_one       the 'same' crop starts one row and column late
      border_tap_dropped    tap (0, 0) does not reach output pixel (0, 0): a bounds test that is off by one at the border
      phases_swapped        output phases (0, 1) and (1, 0) land in each other's place
      taps_transposed       tap (a, b) uses the weights of tap (b, a)
      channel_quad_shifted  output channels 0 .. 3 hold what channels 4 .. 7 should (a quad store one slot off)
      outconv_reads_edge    the output convolution reads row 0 in place of the zero padding above it
                            (error_maps.output_conv(pad_top="edge"))"""
    c = CASES[case]
    x = weights["dense_1"][1].astype(np.int64)
    if c["mid"] is not None:
        w, b = weights["dense_2"]
        x = x @ w.astype(np.int64) + b.astype(np.int64)
    x = x.reshape(c["reshape"])
    peak = int(np.abs(x).max())
    for i, (cout, k, same, _) in enumerate(c["convts"]):
        w, b = (t.astype(np.int64) for t in weights["conv2d_transpose" if i == 0 else f"conv2d_transpose_{i}"])
        d = defect if i == layer else None
        h, wd, _ = x.shape
        full = np.zeros((2 * (h - 1) + k, 2 * (wd - 1) + k, cout), np.int64)
        for a in range(k):
            for bb in range(k):
                tap = w[bb, a] if d == "taps_transposed" else w[a, bb]
                t = x @ tap.T
                if d == "border_tap_dropped" and (a, bb) == (0, 0):
                    t[0, 0] = 0
                full[a:a + 2 * h - 1:2, bb:bb + 2 * wd - 1:2] += t
        if same:
            o = 1 if (d == "crop_off_by_one" and k == 3) else 0
            full = full[o:o + 2 * h, o:o + 2 * wd]
        y = full + b
        if d == "phases_swapped":
            hh, ww = y.shape[0] // 2 * 2, y.shape[1] // 2 * 2
            t = y[0:hh:2, 1:ww:2].copy()
            y[0:hh:2, 1:ww:2] = y[1:hh:2, 0:ww:2]
            y[1:hh:2, 0:ww:2] = t
        if d == "channel_quad_shifted":
            y[..., 0:4] = y[..., 4:8].copy()
        x = y
        peak = max(peak, int(np.abs(x).max()))
    w, b = (t.astype(np.int64) for t in weights["output_image"])
    H, W, _ = x.shape
    xp = np.pad(x, ((1, 1), (1, 1), (0, 0)))
    if defect == "outconv_reads_edge":
        xp[0, 1:-1] = x[0]
    y = sum(xp[ty:ty + H, tx:tx + W] @ w[ty, tx, :, 0] for ty in range(3) for tx in range(3)) + b[0]
    return y, peak


# ------------------------------------------------------------------------------------------------------------------------
# the references of the statistics tests, computed once per case and process
# ------------------------------------------------------------------------------------------------------------------------
_REF = {}


def references(case, enc_w, coarse_cases, lr_stats):
    """-> dict(specs, x (n, 10, 10, 1), T (n, H, W) float64, "bf16" / "f16": the emulation E of that kind, classes): the random-
    weight graph of the case on error_maps.fixed_batch(n = batch_size(case)).  Shared, never modified."""
    if case not in _REF:
        import error_maps as em
        import family_ref as fr
        n = batch_size(case)
        x = em.fixed_batch(coarse_cases, lr_stats, n)
        specs = build_specs(case, enc_w, random_decoder(case))
        ref = dict(specs=specs, x=x, T=fr.forward_specs64(specs, x)[..., 0])
        for kind in KINDS:
            ref[kind] = fr.forward_specs_lowp(specs, x, kind)[..., 0]
        ref["classes"] = {kind: em.grid_classes(n, *out_hw(case), stacked=len(CASES[case]["convts"]), pool=POOL[kind], sample_group=sample_group(case))
                          for kind in KINDS}
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[case] = ref
    return _REF[case]
