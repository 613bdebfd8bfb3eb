"""SRCFD_FLAG_NAN_GUARD on partly bad fields: the numpy reference, the recipe that makes such fields, and planted defects
(shared by test_guard_cases.py, which needs no GPU, and test_gpu_nonfinite_guard.py).

The contract (include/srcfd.h): a guarded call zero-fills every element that is non-finite IN y's OWN TYPE and adds their
number to the counter; every other element keeps the bits of the unguarded call.  `guard_ref` states it in numpy, which is the
reference's `np.nan_to_num(..., 0, 0, 0)` and its warning count applied to the array the caller receives.

The recipe.  Every older guard test poisons an input, so all H W values of that sample are bad.  Here the network runs
untouched and the OUTPUT AFFINE overflows part of the field: for a sample whose un-affined output is `acc`, the row
(mean, std) = (0, T / q) with T the overflow threshold of the output type and q the Q-quantile of |acc| turns the share
1 - Q of the field into +-Inf, both signs, scattered over rows, tiles, lanes' groups of four and waves.  A second kind of row
carries a non-zero mean (+-T / 8), which moves the two signs' shares apart.  float32 cannot scale by more than FLT_MAX: where
T / q is not finite in float32 (q < 1) std is FLT_MAX, and the bad set is |acc| > 1 or so.  The choices, stated once:

    inputs   error_maps.fixed_batch(coarse_cases, lr_stats, 3), trained multiBC encoder + synthetic_decoder(1)
    rows     sample i takes ROWS[i % 3]: (Q, mean / T) = (0.90, 0), (0.80, +1/8), (0.97, -1/8)

They were the first tried; test_guard_cases.py shows that they deliver every coverage condition of `coverage` for all three
output types, and the GPU module asserts the same conditions on the device's own pattern.

Arrays: a float32 output is np.float32, a float16 output np.float16, a bfloat16 output its uint16 bit pattern (numpy has no
bfloat16).  `bits` gives the unsigned view all comparisons are made on.  Pure numpy; nothing here touches the GPU.
"""
from __future__ import annotations

import numpy as np

OUT_DTYPES = ("float32", "bfloat16", "float16")
SIXTEEN_BIT = ("bf16", "f16")                       # precisions that de-standardise with one fma (srcfd.h)
FLT_MAX = np.float32(3.4028234663852886e38)
# the smallest magnitude that the round-to-nearest-even cast turns into Inf: the largest finite value plus half an ulp (the tie
# goes to the even neighbour, and the largest finite value's mantissa is odd).  float32: the value itself must already be Inf.
OVERFLOW = {
    "float32": np.float32(np.inf),
    "bfloat16": np.array(0x7F7F8000, np.uint32).view(np.float32)[()],    # 3.3961775e38
    "float16": np.float32(65520.0),
}
# T of the recipe: what a value has to reach to be bad.  For float32 a product must pass FLT_MAX (plus half an ulp).
TRIGGER_T = {"float32": FLT_MAX, "bfloat16": OVERFLOW["bfloat16"], "float16": OVERFLOW["float16"]}
ROWS = ((0.90, 0.0), (0.80, 0.125), (0.97, -0.125))   # (Q, mean / T) of sample i % 3
SHARE = (0.01, 0.25)                                  # the bad share a triggered sample must show
START = 7                                             # the counter's value before a guarded call
H = W = 400


# ------------------------------------------------------------------------------------------------------------------------
# casts and views
# ------------------------------------------------------------------------------------------------------------------------
def cast(v32, out_dtype):
    """float32 -> the output type, round to nearest even, overflow to +-Inf, NaN stays NaN."""
    v32 = np.ascontiguousarray(v32, np.float32)
    if out_dtype == "float32":
        return v32
    if out_dtype == "float16":
        with np.errstate(over="ignore", invalid="ignore"):
            return v32.astype(np.float16)
    assert out_dtype == "bfloat16"
    u = v32.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(v32), ((u >> 16) | 0x40).astype(np.uint16), r)


def bits(y):
    y = np.ascontiguousarray(y)
    return y.view({4: np.uint32, 2: np.uint16}[y.dtype.itemsize])


def to_f32(y, out_dtype):
    if out_dtype == "bfloat16":
        return (np.ascontiguousarray(y).view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    return np.asarray(y).astype(np.float32)


def finite(y, out_dtype):
    return np.isfinite(to_f32(y, out_dtype))


def same_bits(got, want, out_dtype):
    """Element-wise: the same bit pattern, or NaN on both sides (a NaN's payload is not part of any contract)."""
    g, w = bits(got), bits(want)
    return (g == w) | (np.isnan(to_f32(got, out_dtype)) & np.isnan(to_f32(want, out_dtype)))


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def guard_ref(v32, out_dtype):
    """(y, count): v32 cast to out_dtype; every element that is not finite THERE becomes +0 and is counted."""
    y = cast(v32, out_dtype).copy()
    bad = ~finite(y, out_dtype)
    y[bad] = 0
    return y, int(bad.sum())


def fma32(a, b, c):
    """round_f32(a * b + c) with ONE rounding, a, b, c float32: the product is exact in float64, the sum is rounded to odd there
    (TwoSum gives its error), and a round-to-odd 53-bit value rounds to 24 bits like the exact one.  Overflows to +-Inf."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.broadcast_to(np.asarray(c, np.float64), p.shape)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def affine_ref(acc32, aout, precision):
    """y * std + mean as srcfd.h states it: one fma in the 16-bit precisions, two float32 roundings (numpy's own float32
    arithmetic, as in test_gpu_parity_fp32.py) in fp32 / fp32_naive / fp32x3.  acc32 (n, ...), aout (n, 2) = (mean, std)."""
    acc32 = np.asarray(acc32, np.float32)
    aout = np.asarray(aout, np.float32)
    shape = (-1,) + (1,) * (acc32.ndim - 1)
    mean, std = aout[:, 0].reshape(shape), aout[:, 1].reshape(shape)
    if precision in SIXTEEN_BIT:
        return fma32(acc32, std, mean)
    assert precision in ("fp32", "fp32_naive", "fp32x3"), precision
    with np.errstate(over="ignore", invalid="ignore"):
        v = acc32 * std + mean
    assert v.dtype == np.float32
    return v


# ------------------------------------------------------------------------------------------------------------------------
# the recipe
# ------------------------------------------------------------------------------------------------------------------------
def trigger_rows(acc32, out_dtype, first=0):
    """(n, 2) float32 (mean, std): sample i takes ROWS[(first + i) % 3] on the quantile of its own |acc|."""
    acc32 = np.asarray(acc32, np.float32)
    T = float(TRIGGER_T[out_dtype])
    rows = []
    for i in range(acc32.shape[0]):
        Q, m = ROWS[(first + i) % 3]
        q = float(np.quantile(np.abs(acc32[i]), Q))
        rows.append((m * T, min(T / q, float(FLT_MAX)) if q > 0 else float(FLT_MAX)))
    return np.asarray(rows, np.float32)


def strip_seam_rows(seg):
    """Output rows on the two sides of the seams between the segments of SRCFD_TAIL_SEG=seg: a segment's first strip starts at
    row k L - 1 (strips are rows 8 g - 1 .. 8 g + 6, kernels_bf16.hip), L = 400 / seg."""
    L = H // seg
    k = np.arange(1, seg) * L
    return k - 2, k - 1


def coverage(bad, pos_inf=None, neg_inf=None):
    """What a pattern must show to be able to reveal the planted defects: name -> bool.  bad (n, 400, 400) of TRIGGERED samples
    in batch order; pos_inf / neg_inf: the same shape, where the unguarded value is +Inf / -Inf."""
    bad = np.asarray(bad, bool)
    n = bad.shape[0]
    share = bad.reshape(n, -1).mean(1)
    c = {"share": bool(np.all((share >= SHARE[0]) & (share <= SHARE[1]))),
         "row_0": bool(bad[:, 0].any()), "row_399": bool(bad[:, H - 1].any()),
         "cols_384_399": bool(bad[:, :, 384:392].any() and bad[:, :, 392:].any())}
    if pos_inf is not None:
        c["both_signs"] = bool(np.any(pos_inf) and np.any(neg_inf))
    if n > 1:
        c["sample_seam"] = bool(any(bad[i, H - 1].any() and bad[i + 1, 0].any() for i in range(n - 1)))
    for seg in (5, 25):
        above, below = strip_seam_rows(seg)
        c[f"strip_seam_{seg}"] = bool(bad[:, above].any() and bad[:, below].any())
    g = bad.reshape(n, H, W // 4, 4)
    k = g.sum(-1)
    c["group_none"] = bool((k == 0).any())
    c["group_all"] = bool((k == 4).any())
    for j in range(4):
        c[f"group_only_{j}"] = bool(((k == 1) & g[..., j]).any())
    return c, share


# ------------------------------------------------------------------------------------------------------------------------
# planted defects: a numpy restatement of the guard epilogue of the two 16-bit tails, with one thing wrong at a time
# ------------------------------------------------------------------------------------------------------------------------
DEFECTS = {
    "a_test_before_cast": "the test is made on the float32 value, the cast comes after (the order before this module)",
    "b_idle_lanes_counted": "lanes that hold no pixel are counted: the clamped duplicate of tile 49 once more",
    "c_wave_count_by_every_lane": "the per-wave count of the fast path is added by all 64 lanes",
    "d_group_zeroed": "a whole group of four is zeroed when one of its values is bad",
    "e_seam_count_dropped": "the per-lane count of the seam rows is never added",
    "f_neg_inf_passes": "-Inf passes",
    "g_nan_passes": "NaN passes, as in a `v > FLT_MAX` form of the test",
    "h_counter_overwritten": "the counter is stored, not added to",
}


def seam_row_mask(n, seg=1):
    """(n, 400) bool: the rows the seam epilogue writes (do_d): rows 0 and 399 of every sample, and the first row pair of every
    segment's first strip, rows k L - 1 and k L.  Every other row goes through the fast path."""
    m = np.zeros((n, H), bool)
    m[:, 0] = m[:, H - 1] = True
    if seg > 1:
        k = np.arange(1, seg) * (H // seg)
        m[:, k - 1] = m[:, k] = True
    return m


def guard_epilogue(v32, out_dtype, start=START, seg=1, defect=None):
    """(y, counter after the call) of a guarded call on the float32 values v32 (n, 400, 400), as the kernels are built: the
    per-value test, the zero-fill, a per-wave count on the fast rows and a per-lane count on the seam rows, both added to
    the counter.  defect: None, or a key of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    v32 = np.asarray(v32, np.float32)
    n = v32.shape[0]
    y = cast(v32, out_dtype).copy()
    f = to_f32(y, out_dtype)
    if defect == "a_test_before_cast":
        bad = ~np.isfinite(v32)
    elif defect == "f_neg_inf_passes":
        bad = np.isnan(f) | (f == np.inf)
    elif defect == "g_nan_passes":
        with np.errstate(invalid="ignore"):
            bad = np.abs(f) == np.inf
    else:
        bad = ~np.isfinite(f)
    zero = bad
    if defect == "d_group_zeroed":
        zero = np.repeat(bad.reshape(n, H, W // 4, 4).any(-1), 4, axis=-1).reshape(n, H, W)
    y[zero] = 0
    seam = seam_row_mask(n, seg)[:, :, None] & bad
    fast = bad & ~seam
    n_fast, n_seam = int(fast.sum()), int(seam.sum())
    if defect == "b_idle_lanes_counted":
        n_fast += int(fast[:, :, 392:].sum())
    if defect == "c_wave_count_by_every_lane":
        n_fast *= 64
    if defect == "e_seam_count_dropped":
        n_seam = 0
    count = n_fast + n_seam
    return y, (count if defect == "h_counter_overwritten" else start + count)


# ------------------------------------------------------------------------------------------------------------------------
# a NaN that is local: one unit of dense_1's bias
# ------------------------------------------------------------------------------------------------------------------------
DECODER_GEOMETRY = ((3, 2), (2, 2), (2, 2), (2, 2), (2, 2))   # (kernel, stride) of the five VALID transposed convolutions, 12 -> 400
LATENT_GRID, LATENT_CH = 12, 256                              # dense_1's output as (12, 12, 256), sr_oracle.decoder_forward


def nan_unit(r, c, ch=0):
    """Index into dense_1/bias of channel ch of latent pixel (r, c)."""
    return (r * LATENT_GRID + c) * LATENT_CH + ch


def nan_footprint(r, c):
    """(400, 400) bool: the output pixels that latent pixel (r, c) reaches.  A VALID transposed convolution (k, s) sends input
    index i to outputs s i .. s i + k - 1; the 3x3 SAME output convolution adds one pixel on each side; clipped to the field."""
    def axis(i):
        lo = hi = i
        for k, s in DECODER_GEOMETRY:
            lo, hi = s * lo, s * hi + k - 1
        return max(lo - 1, 0), min(hi + 1, H - 1)
    (r0, r1), (c0, c1) = axis(r), axis(c)
    m = np.zeros((H, W), bool)
    m[r0:r1 + 1, c0:c1 + 1] = True
    return m


# ------------------------------------------------------------------------------------------------------------------------
# the recipe's data on the CPU (computed once, shared, never written to)
# ------------------------------------------------------------------------------------------------------------------------
_REF = {}


def recipe_reference(enc_w, dec_w, coarse_cases, lr_stats):
    """{"x": fixed_batch(3), "acc": the float64 oracle's output rounded to float32, (3, 400, 400)}."""
    if "acc" not in _REF:
        import error_maps as em
        from oracle import sr_oracle as o
        x = em.fixed_batch(coarse_cases, lr_stats, 3)
        acc = o.superres_forward(x, enc_w, dec_w, np.float64)[..., 0].astype(np.float32)
        x.setflags(write=False)
        acc.setflags(write=False)
        _REF.update(x=x, acc=acc)
    return _REF
