"""Guard bands and sentinels around the buffers a test hands to the library (tests/test_gpu_buffer_bounds.py; the helper's own
test with planted defects is tests/test_guard_bands.py).

One flat allocation [guard | payload | guard], every word pre-filled with a NaN payload that no finite input can turn into.  After
the call under test:
  * assert_guards_intact: a changed guard word is a store outside the caller's extent;
  * assert_fully_written: a sentinel word left in the payload is an output element the call never wrote;
  * poisoned(): the same layout for INPUTS, quiet NaNs in both guards -- a read outside the extent that reaches the result makes
    it NaN, which the bit comparison with the plain call's result then reports.
All comparisons run where the buffer lives (torch tensor on its device, or numpy) through integer views; only short index lists
reach the host.  `xp` is the `torch` module or the `numpy` module: the numpy twin serves host destinations.

Every guard lies inside the one allocation the test owns, so a defect shows as a changed word, never as a fault.  A larger overrun
than the guard is not seen (and is no more dangerous than with an exact-size tensor)."""
import numpy as np

ALIGN = 256          # bytes: the payload starts at a multiple of this inside its allocation, like a fresh device allocation,
                     # or `skew` elements behind one (guarded / poisoned, skew=): what a contiguous view into a larger tensor gives
SENTINEL32 = 0x7FA5A5A5            # float32 NaN payload
SENTINEL16 = 0x7FA5                # a NaN in bfloat16 and in float16
SENTINEL64 = 0x7FF5A5A5A5A5A5A5    # float64 NaN payload
SENTINEL_I64 = 0x5A5A5A5A5A5A5A5B  # a fixed odd pattern for the neighbours of an int64 counter
FLAT_GUARD = 4096    # elements on each side of a flat parameter array
SHOW = 8             # indices quoted in a failure message


def _is_np(xp):
    return xp is np


def _kind(xp, dtype):
    """(word dtype, sentinel word, element bytes) of a payload dtype."""
    if _is_np(xp):
        dt = np.dtype(dtype)
        table = {np.dtype(np.float32): (np.int32, SENTINEL32), np.dtype(np.float16): (np.int16, SENTINEL16),
                 np.dtype(np.uint16): (np.int16, SENTINEL16), np.dtype(np.float64): (np.int64, SENTINEL64),
                 np.dtype(np.int64): (np.int64, SENTINEL_I64)}
        word, fill = table[dt]
        return word, fill, dt.itemsize
    table = {xp.float32: (xp.int32, SENTINEL32), xp.bfloat16: (xp.int16, SENTINEL16), xp.float16: (xp.int16, SENTINEL16),
             xp.float64: (xp.int64, SENTINEL64), xp.int64: (xp.int64, SENTINEL_I64)}
    word, fill = table[dtype]
    return word, fill, {xp.int16: 2, xp.int32: 4, xp.int64: 8}[word]


def round_guard(guard_elems, itemsize):
    """guard_elems rounded up so that the guard is a whole number of ALIGN-byte blocks (and never empty)."""
    per = ALIGN // itemsize
    return max(1, -(-int(guard_elems) // per)) * per


def affine_guard():
    """Guard of an (n, 2) float32 affine table: one row pair, rounded up to 256 bytes."""
    return round_guard(2, 4)


def guarded(xp, shape, dtype, guard_elems, fill=None, device="cuda", skew=0):
    """(big, view): `big` is the flat integer-word allocation [guard | payload | guard], every word = `fill` (default: the dtype's
    sentinel); `view` is the contiguous payload as `dtype` and `shape`.  torch: on `device`.
    skew (elements, 0 <= skew < ALIGN / itemsize): the payload starts skew * itemsize bytes behind a multiple of ALIGN -- aligned to
    its element and to nothing wider when skew is odd; the front guard grows by `skew` words, the rear guard keeps its size."""
    word, sentinel, itemsize = _kind(xp, dtype)
    fill = sentinel if fill is None else fill
    g = round_guard(guard_elems, itemsize)
    skew = int(skew)
    assert 0 <= skew < ALIGN // itemsize, skew
    size = int(np.prod(shape, dtype=np.int64)) if len(tuple(shape)) else 1
    total = 2 * g + skew + size
    if _is_np(xp):
        # over-allocate so that the payload itself starts at a multiple of ALIGN bytes (+ the skew)
        raw = np.empty(total * itemsize + ALIGN, np.uint8)
        skip = (-raw.ctypes.data) % ALIGN
        big = raw[skip:skip + total * itemsize].view(word)
        big[:] = fill
        return big, big[g + skew:g + skew + size].view(dtype).reshape(shape)
    big = xp.full((total,), fill, dtype=word, device=device)
    return big, big[g + skew:g + skew + size].view(dtype).view(tuple(shape))


def refill(big, fill=None):
    """Every word of `big` back to the sentinel, in place (a repeated call into the same addresses)."""
    itemsize = big.itemsize if isinstance(big, np.ndarray) else big.element_size()
    fill = {2: SENTINEL16, 4: SENTINEL32, 8: SENTINEL64}[itemsize] if fill is None else fill
    if isinstance(big, np.ndarray):
        big[:] = fill
    else:
        big.fill_(fill)


def guarded_in(xp, buf, shape, dtype, guard_elems, fill=None):
    """numpy only: the same layout inside a caller-supplied uint8 buffer (page-locked memory, say) of at least
    guarded_nbytes(shape, dtype, guard_elems) bytes."""
    assert _is_np(xp)
    word, sentinel, itemsize = _kind(xp, dtype)
    fill = sentinel if fill is None else fill
    g = round_guard(guard_elems, itemsize)
    size = int(np.prod(shape, dtype=np.int64))
    skip = (-buf.ctypes.data) % ALIGN
    big = buf[skip:skip + (2 * g + size) * itemsize].view(word)
    big[:] = fill
    return big, big[g:g + size].view(dtype).reshape(shape)


def guarded_nbytes(shape, dtype, guard_elems):
    itemsize = np.dtype(dtype).itemsize
    return (2 * round_guard(guard_elems, itemsize) + int(np.prod(shape, dtype=np.int64))) * itemsize + ALIGN


def poisoned(xp, array, guard_elems, device="cuda", skew=0):
    """(big, view) for an INPUT: `array` (numpy, float32 or float64) sits in the payload, quiet NaNs fill both guards.
    skew: as in `guarded`."""
    array = np.ascontiguousarray(array)
    assert array.dtype in (np.float32, np.float64), array.dtype
    itemsize = array.dtype.itemsize
    g = round_guard(guard_elems, itemsize)
    skew = int(skew)
    assert 0 <= skew < ALIGN // itemsize, skew
    lo = g + skew
    flat = np.full(2 * g + skew + array.size, np.nan, array.dtype)
    flat[lo:lo + array.size] = array.ravel()
    if _is_np(xp):
        raw = np.empty(flat.nbytes + ALIGN, np.uint8)
        skip = (-raw.ctypes.data) % ALIGN
        big = raw[skip:skip + flat.nbytes].view(array.dtype)
        big[:] = flat
        return big, big[lo:lo + array.size].reshape(array.shape)
    big = xp.from_numpy(flat).to(device)
    return big, big[lo:lo + array.size].view(array.shape)


def _ptr(t):
    return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def _first(mask):
    """(count, the first SHOW indices) of a boolean mask; only those reach the host."""
    if isinstance(mask, np.ndarray):
        idx = np.flatnonzero(mask)
        return int(idx.size), [int(i) for i in idx[:SHOW]]
    idx = mask.nonzero().reshape(-1)
    return int(idx.numel()), [int(i) for i in idx[:SHOW].cpu()]


def _where(indices, shape):
    return [tuple(int(v) for v in np.unravel_index(i, shape)) for i in indices] if len(tuple(shape)) > 1 else indices


def assert_guards_intact(big, view, fill=None, what=""):
    """No word of `big` outside `view`'s extent differs from the sentinel.  Indices in the message count payload elements: negative
    in front of the payload, from the payload's size on behind it."""
    itemsize = big.itemsize if isinstance(big, np.ndarray) else big.element_size()
    off = (_ptr(view) - _ptr(big)) // itemsize
    size = int(np.prod(tuple(view.shape), dtype=np.int64)) if len(tuple(view.shape)) else 1
    total = big.size if isinstance(big, np.ndarray) else big.numel()
    assert 0 < off and off + size < total, (off, size, total)
    if fill is None:
        fill = {2: SENTINEL16, 4: SENTINEL32, 8: SENTINEL64}[itemsize]
    n_front, i_front = _first(big[:off] != fill)
    n_back, i_back = _first(big[off + size:] != fill)
    if n_front or n_back:
        raise AssertionError(f"{what}: the call wrote outside its output extent: {n_front} word(s) in front of it at element(s) "
                             f"{[i - off for i in i_front]}, {n_back} behind it at element(s) {[size + i for i in i_back]} "
                             f"(payload: {size} elements, shape {tuple(view.shape)})")


def assert_fully_written(view, fill=None, what=""):
    """No element of the payload still holds the sentinel it was pre-filled with."""
    itemsize = view.itemsize if isinstance(view, np.ndarray) else view.element_size()
    if isinstance(view, np.ndarray):
        words = view.reshape(-1).view({2: np.int16, 4: np.int32, 8: np.int64}[itemsize])
    else:
        import torch
        words = view.reshape(-1).view({2: torch.int16, 4: torch.int32, 8: torch.int64}[itemsize])
    if fill is None:
        fill = {2: SENTINEL16, 4: SENTINEL32, 8: SENTINEL64}[itemsize]
    n, idx = _first(words == fill)
    if n:
        raise AssertionError(f"{what}: {n} output element(s) were never written, the first at {_where(idx, tuple(view.shape))} "
                             f"(flat {idx}; shape {tuple(view.shape)})")


def assert_same_bits(got, want, what=""):
    """got and want (both torch tensors or both numpy arrays, same dtype and shape) hold the same bits; NaNs compare by payload."""
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, tuple(got.shape), tuple(want.shape), got.dtype, want.dtype)
    itemsize = got.itemsize if isinstance(got, np.ndarray) else got.element_size()
    if isinstance(got, np.ndarray):
        word = {2: np.int16, 4: np.int32, 8: np.int64}[itemsize]
        a, b = np.ascontiguousarray(got).reshape(-1).view(word), np.ascontiguousarray(want).reshape(-1).view(word)
    else:
        import torch
        word = {2: torch.int16, 4: torch.int32, 8: torch.int64}[itemsize]
        a, b = got.contiguous().reshape(-1).view(word), want.contiguous().reshape(-1).view(word)
        if torch.equal(a, b):
            return
    n, idx = _first(a != b)
    if n:
        raise AssertionError(f"{what}: {n} element(s) differ from the plain call's bits, the first at {_where(idx, tuple(got.shape))} "
                             f"(flat {idx}; shape {tuple(got.shape)})")


def guarded_counter(xp, start=5, device="cuda"):
    """(three int64 words, the middle one as a 1-element view): the `nonfinite` counter starts at `start` between two sentinels."""
    if _is_np(xp):
        three = np.array([SENTINEL_I64, start, SENTINEL_I64], np.int64)
    else:
        three = xp.tensor([SENTINEL_I64, start, SENTINEL_I64], dtype=xp.int64, device=device)
    return three, three[1:2]


def assert_counter(three, expect, what=""):
    got = [int(v) for v in (three if isinstance(three, np.ndarray) else three.cpu())]
    assert got[0] == SENTINEL_I64 and got[2] == SENTINEL_I64, f"{what}: a neighbour of the nonfinite counter was written: {[hex(v) for v in got]}"
    assert got[1] == expect, f"{what}: nonfinite counter {got[1]}, expected {expect}"
