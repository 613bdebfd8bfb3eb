"""tests/guard_bands.py on CPU tensors and numpy arrays with planted defects: every defect the GPU tests rely on it to report is
reported, and a clean fill passes.  No kernel runs here."""
import numpy as np
import pytest

import guard_bands as gb


def _torch():
    import torch
    return torch


BACKENDS = ["numpy", "torch"]


def _xp(name):
    return np if name == "numpy" else _torch()


def _dtypes(xp):
    if xp is np:
        return [np.float32, np.float16, np.float64]
    return [xp.float32, xp.bfloat16, xp.float16, xp.float64]


def _make(xp, shape, dtype, guard):
    return gb.guarded(xp, shape, dtype, guard, device="cpu") if xp is not np else gb.guarded(xp, shape, dtype, guard)


def _fill_clean(xp, view):
    """What a correct kernel does: every payload element gets a finite value."""
    if xp is np:
        view[...] = np.arange(view.size, dtype=np.float64).reshape(view.shape).astype(view.dtype)
    else:
        view.copy_(xp.arange(view.numel(), dtype=xp.float64).reshape(view.shape).to(view.dtype))


@pytest.mark.parametrize("backend", BACKENDS)
def test_layout_and_sentinels(backend):
    xp = _xp(backend)
    for dtype in _dtypes(xp):
        big, view = _make(xp, (3, 5, 7), dtype, 35)
        itemsize = big.itemsize if xp is np else big.element_size()
        g = gb.round_guard(35, itemsize)
        assert g * itemsize % gb.ALIGN == 0 and g >= 35
        ptr = (lambda t: t.ctypes.data) if xp is np else (lambda t: t.data_ptr())
        assert ptr(view) - ptr(big) == g * itemsize
        if xp is np:
            assert ptr(view) % gb.ALIGN == 0
            assert big.size == 2 * g + 105 and view.flags.c_contiguous
            assert np.isnan(view).all()
        else:
            assert big.numel() == 2 * g + 105 and view.is_contiguous()
            assert bool(xp.isnan(view.double()).all())     # the sentinel is a NaN in every format, bfloat16 and float16 alike
        assert tuple(view.shape) == (3, 5, 7)
        # untouched: the guards are intact and every payload element counts as unwritten
        gb.assert_guards_intact(big, view)
        with pytest.raises(AssertionError, match="105 output element"):
            gb.assert_fully_written(view)


def _ptr(xp, t):
    return t.ctypes.data if xp is np else t.data_ptr()


@pytest.mark.parametrize("skew", [1, 2, 3])
@pytest.mark.parametrize("backend", BACKENDS)
def test_skewed_layout_keeps_its_guards(backend, skew):
    """skew elements behind a multiple of ALIGN: element-aligned, both guards whole (the front one `skew` words longer), and every
    planted defect is still reported at its payload-relative index."""
    xp = _xp(backend)
    for dtype in _dtypes(xp):
        big, view = _make_skewed(xp, (3, 5, 7), dtype, 35, skew)
        itemsize = big.itemsize if xp is np else big.element_size()
        g = gb.round_guard(35, itemsize)
        lo = g + skew
        assert _ptr(xp, view) - _ptr(xp, big) == lo * itemsize
        if xp is np or _ptr(xp, big) % gb.ALIGN == 0:           # numpy: by construction; torch on the CPU: when the allocator gives it
            assert _ptr(xp, view) % gb.ALIGN == skew * itemsize
        assert _ptr(xp, view) % itemsize == 0
        assert (big.size if xp is np else big.numel()) == 2 * g + skew + 105
        assert (view.flags.c_contiguous if xp is np else view.is_contiguous()) and tuple(view.shape) == (3, 5, 7)
        gb.assert_guards_intact(big, view)
        with pytest.raises(AssertionError, match="105 output element"):
            gb.assert_fully_written(view)
        _fill_clean(xp, view)
        gb.assert_guards_intact(big, view, what="clean")
        gb.assert_fully_written(view, what="clean")
        # the words next to the payload on both sides, and the far ends of both guards
        for pos, rel, front in ((lo - 1, -1, True), (0, -lo, True), (lo + 105, 105, False), (2 * g + skew + 104, 105 + g - 1, False)):
            old = int(big[pos])
            big[pos] = 0
            with pytest.raises(AssertionError, match=r"wrote outside its output extent") as e:
                gb.assert_guards_intact(big, view, what="planted")
            msg = str(e.value)
            assert f"[{rel}]" in msg and (("1 word(s) in front" in msg and "0 behind" in msg) if front else ("0 word(s) in front" in msg and "1 behind" in msg)), msg
            big[pos] = old
        gb.assert_guards_intact(big, view)
        # the first and the last payload element left unwritten
        fill = {2: gb.SENTINEL16, 4: gb.SENTINEL32, 8: gb.SENTINEL64}[itemsize]
        for pos, where in ((lo, r"\(0, 0, 0\)"), (lo + 104, r"\(2, 4, 6\)")):
            old = int(big[pos])
            big[pos] = fill
            with pytest.raises(AssertionError, match=r"1 output element\(s\) were never written, the first at \[" + where):
                gb.assert_fully_written(view, what="planted")
            big[pos] = old


def _make_skewed(xp, shape, dtype, guard, skew):
    return gb.guarded(xp, shape, dtype, guard, skew=skew) if xp is np else gb.guarded(xp, shape, dtype, guard, device="cpu", skew=skew)


@pytest.mark.parametrize("backend", BACKENDS)
def test_skew_zero_is_the_old_layout_and_a_skew_of_a_whole_block_is_refused(backend):
    xp = _xp(backend)
    big0, view0 = _make(xp, (4, 9), xp.float32, 36)
    big1, view1 = _make_skewed(xp, (4, 9), xp.float32, 36, 0)
    assert (big0.size if xp is np else big0.numel()) == (big1.size if xp is np else big1.numel())
    assert _ptr(xp, view0) - _ptr(xp, big0) == _ptr(xp, view1) - _ptr(xp, big1)
    with pytest.raises(AssertionError):
        _make_skewed(xp, (4, 9), xp.float32, 36, gb.ALIGN // 4)
    with pytest.raises(AssertionError):
        _make_skewed(xp, (4, 9), xp.float32, 36, -1)


@pytest.mark.parametrize("skew", [1, 2, 3])
@pytest.mark.parametrize("backend", BACKENDS)
def test_skewed_poisoned_inputs(backend, skew):
    xp = _xp(backend)
    rng = np.random.default_rng(skew)
    for dt in (np.float32, np.float64):
        a = rng.standard_normal((3, 5, 2)).astype(dt)
        big, view = gb.poisoned(xp, a, 10, skew=skew) if xp is np else gb.poisoned(xp, a, 10, device="cpu", skew=skew)
        g = gb.round_guard(10, a.itemsize)
        got = view if xp is np else view.numpy()
        flat = big if xp is np else big.numpy()
        assert got.dtype == dt and np.array_equal(got, a)
        assert flat.size == 2 * g + skew + a.size and np.isnan(flat[:g + skew]).all() and np.isnan(flat[g + skew + a.size:]).all()
        assert flat[g + skew + a.size:].size == g
        assert _ptr(xp, view) - _ptr(xp, big) == (g + skew) * a.itemsize
        if xp is np:
            assert view.ctypes.data % gb.ALIGN == skew * a.itemsize


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_clean_fill_passes(backend):
    xp = _xp(backend)
    for dtype in _dtypes(xp):
        for shape in [(1,), (21,), (2, 3, 5), (3, 400)]:
            big, view = _make(xp, shape, dtype, 7)
            _fill_clean(xp, view)
            gb.assert_guards_intact(big, view, what="clean")
            gb.assert_fully_written(view, what="clean")


@pytest.mark.parametrize("where", ["front", "back"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_one_word_in_a_guard_is_reported(backend, where):
    xp = _xp(backend)
    for dtype in _dtypes(xp):
        big, view = _make(xp, (4, 9), dtype, 36)
        _fill_clean(xp, view)
        itemsize = big.itemsize if xp is np else big.element_size()
        g = gb.round_guard(36, itemsize)
        # the element just outside the payload, and the farthest guard word
        for pos, rel in ((g - 1, -1), (0, -g)) if where == "front" else ((g + 36, 36), (2 * g + 35, 36 + g - 1)):
            old = int(big[pos])
            big[pos] = 0
            with pytest.raises(AssertionError, match=r"wrote outside its output extent") as e:
                gb.assert_guards_intact(big, view, what="planted")
            msg = str(e.value)
            assert f"[{rel}]" in msg, msg
            assert ("1 word(s) in front" in msg and "0 behind" in msg) if where == "front" else ("0 word(s) in front" in msg and "1 behind" in msg), msg
            big[pos] = old
            gb.assert_guards_intact(big, view)
        gb.assert_fully_written(view)


@pytest.mark.parametrize("backend", BACKENDS)
def test_one_unwritten_payload_element_is_reported(backend):
    xp = _xp(backend)
    for dtype in _dtypes(xp):
        big, view = _make(xp, (4, 9), dtype, 36)
        _fill_clean(xp, view)
        itemsize = big.itemsize if xp is np else big.element_size()
        g = gb.round_guard(36, itemsize)
        fill = {2: gb.SENTINEL16, 4: gb.SENTINEL32, 8: gb.SENTINEL64}[itemsize]
        big[g + 2 * 9 + 4] = fill               # element (2, 4) skipped
        with pytest.raises(AssertionError, match=r"1 output element\(s\) were never written, the first at \[\(2, 4\)\]"):
            gb.assert_fully_written(view, what="planted")
        gb.assert_guards_intact(big, view)       # the guards are a separate question


@pytest.mark.parametrize("backend", BACKENDS)
def test_odd_16_bit_payload_whose_last_element_is_stored_as_a_32_bit_word(backend):
    """21 sixteen-bit elements: a kernel that stores pairs writes elements 20 and 21 as one 32-bit word; element 21 is the first
    guard word."""
    xp = _xp(backend)
    dtypes = [np.float16] if xp is np else [xp.bfloat16, xp.float16]
    for dtype in dtypes:
        big, view = _make(xp, (3, 7), dtype, 21)
        _fill_clean(xp, view)
        g = gb.round_guard(21, 2)
        assert (g + 20) % 2 == 0                 # the pair is 4-byte aligned, as the device store would need
        pair = big[g + 20:g + 22].view(np.int32 if xp is np else xp.int32)
        pair[0] = 0x3C003C00                     # (1.0, 1.0) in float16
        with pytest.raises(AssertionError, match=r"0 word\(s\) in front of it at element\(s\) \[\], 1 behind it at element\(s\) \[21\]"):
            gb.assert_guards_intact(big, view, what="planted")
        gb.assert_fully_written(view)


@pytest.mark.parametrize("backend", BACKENDS)
def test_poisoned_inputs(backend):
    xp = _xp(backend)
    rng = np.random.default_rng(0)
    for dt in (np.float32, np.float64):
        a = rng.standard_normal((3, 5, 2)).astype(dt)
        big, view = gb.poisoned(xp, a, 10) if xp is np else gb.poisoned(xp, a, 10, device="cpu")
        g = gb.round_guard(10, a.itemsize)
        got = view if xp is np else view.numpy()
        flat = big if xp is np else big.numpy()
        assert got.dtype == dt and np.array_equal(got, a)
        assert flat.size == 2 * g + a.size and np.isnan(flat[:g]).all() and np.isnan(flat[g + a.size:]).all()
        if xp is np:
            assert view.ctypes.data % gb.ALIGN == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_counter_between_sentinels(backend):
    xp = _xp(backend)
    three, cnt = gb.guarded_counter(xp, 5) if xp is np else gb.guarded_counter(xp, 5, device="cpu")
    assert gb.SENTINEL_I64 % 2 == 1
    cnt += 7                                     # "added to"
    gb.assert_counter(three, 12)
    with pytest.raises(AssertionError, match="expected 13"):
        gb.assert_counter(three, 13)
    three[2] = 0
    with pytest.raises(AssertionError, match="neighbour"):
        gb.assert_counter(three, 12)


@pytest.mark.parametrize("backend", BACKENDS)
def test_same_bits_tells_nan_payloads_apart(backend):
    xp = _xp(backend)
    a = np.array([1.0, np.nan, -0.0, 3.0], np.float32)
    b = a.copy()
    if xp is not np:
        a, b = xp.from_numpy(a), xp.from_numpy(b)
    gb.assert_same_bits(a, b)                    # NaN equals the same NaN
    b[2] = 0.0                                   # +0 is not -0
    with pytest.raises(AssertionError, match=r"1 element\(s\) differ.*\[2\]"):
        gb.assert_same_bits(a, b, what="planted")


def test_guarded_in_a_supplied_buffer():
    buf = np.empty(gb.guarded_nbytes((5, 3), np.float32, 15), np.uint8)
    big, view = gb.guarded_in(np, buf, (5, 3), np.float32, 15)
    assert view.ctypes.data % gb.ALIGN == 0 and view.shape == (5, 3)
    assert buf.ctypes.data <= big.ctypes.data and big.ctypes.data + big.nbytes <= buf.ctypes.data + buf.nbytes
    view[...] = 1.0
    gb.assert_guards_intact(big, view)
    gb.assert_fully_written(view)
