"""What the device scorer (csrc/score.hip) must reproduce, stated with numpy: the notebook's metric expressions, numpy's float32
summation order restated in Python, and an evaluator of the plan tables `srcfd_score_plan` prints.  Shared by
tests/test_score_plan.py (CPU) and tests/test_gpu_score.py."""
import numpy as np

CHUNK = 8192     # np.getbufsize(): elements numpy reduces per buffer
LEAF = 128       # PW_BLOCKSIZE of numpy/_core/src/umath/loops_utils.h.src
NAMES = ("mae", "mse", "max_abs", "truth_min", "truth_max", "pred_min", "pred_max", "nonfinite")
# every path of pairwise_sum (serial, one leaf, split, unbalanced split), the chunk edge, two and three chunks, the family's field sizes
LENGTHS = (1, 7, 8, 9, 127, 128, 129, 257, 1000, 4352, 8191, 8192, 8193, 16385, 100, 400, 2500, 6400, 10_000, 160_000)

f32 = np.float32


def leaf_sum(a):
    """pairwise_sum for n <= 128, every add in float32."""
    n = len(a)
    if n < 8:
        res = f32(0.0)
        for v in a:
            res = f32(res + v)
        return res
    r = [f32(a[j]) for j in range(8)]
    body = n - n % 8
    for i in range(8, body, 8):
        for j in range(8):
            r[j] = f32(r[j] + a[i + j])
    res = f32(f32(f32(r[0] + r[1]) + f32(r[2] + r[3])) + f32(f32(r[4] + r[5]) + f32(r[6] + r[7])))
    for i in range(body, n):
        res = f32(res + a[i])
    return res


def pairwise(a):
    n = len(a)
    if n <= LEAF:
        return leaf_sum(a)
    n2 = n // 2
    n2 -= n2 % 8
    return f32(pairwise(a[:n2]) + pairwise(a[n2:]))


def numpy_sum_restated(a):
    """np.sum of a contiguous float32 array: chunks of 8192, pairwise_sum of each, chained from 0.f in order."""
    a = np.ascontiguousarray(a, f32).reshape(-1)
    res = f32(0.0)
    with np.errstate(all="ignore"):
        for lo in range(0, len(a), CHUNK):
            res = f32(res + pairwise(a[lo:lo + CHUNK]))
    return res


def plan_sum(plan, a):
    """The same sum from a plan's tables (srcfd_score_plan JSON), the way the kernel walks them: leaf sums, then the inner nodes in
    table order, then the chain over the chunks."""
    a = np.ascontiguousarray(a, f32).reshape(-1)
    assert plan["elems"] == len(a) and plan["chunk"] == CHUNK
    res = f32(0.0)
    with np.errstate(all="ignore"):
        for c in range(plan["n_chunks"]):
            part = a[c * CHUNK:(c + 1) * CHUNK]
            table = plan["full"] if len(part) == CHUNK else plan["last"]
            vals = [leaf_sum(part[off:off + ln]) for off, ln in table["leaves"]]
            assert sum(ln for _, ln in table["leaves"]) == len(part)
            for left, right, _ in table["nodes"]:
                vals.append(f32(vals[left] + vals[right]))
            res = f32(res + vals[-1])
    return res


def notebook_metrics(pred, truth, pa=None, ta=None):
    """Per sample, the literal numpy expressions of include/srcfd.h's table on p = pred * std + mean, t = truth * std + mean
    (`inverse_standardize`, sr-ae-conv.ipynb:c113); pa / ta: (n, 2) float32 (mean, std) or None.  -> {name: float32 (n,)}."""
    pred = np.ascontiguousarray(pred, f32)
    truth = np.ascontiguousarray(truth, f32)
    n = pred.shape[0]
    out = {k: np.empty(n, f32) for k in NAMES}
    with np.errstate(all="ignore"):
        for i in range(n):
            p = pred[i] * f32(pa[i][1]) + f32(pa[i][0]) if pa is not None else pred[i]
            t = truth[i] * f32(ta[i][1]) + f32(ta[i][0]) if ta is not None else truth[i]
            assert p.dtype == f32 and t.dtype == f32
            out["mae"][i] = np.mean(np.abs(t - p))
            out["mse"][i] = np.mean((t - p)**2)
            out["max_abs"][i] = np.max(np.abs(t - p))
            out["truth_min"][i] = np.min(t)
            out["truth_max"][i] = np.max(t)
            out["pred_min"][i] = np.min(p)
            out["pred_max"][i] = np.max(p)
            out["nonfinite"][i] = np.count_nonzero(~np.isfinite(t - p))
    return out


def assert_same_bits(got, want, what=""):
    """Equality of the float32 bit patterns, NaNs in the same places (any NaN equals any NaN)."""
    for k in want:
        g, w = np.asarray(got[k], f32), np.asarray(want[k], f32)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        same = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
        assert same.all(), f"{what} {k}: rows {np.where(~same)[0][:8].tolist()} differ: got {g[~same][:4]!r}, numpy {w[~same][:4]!r}"
