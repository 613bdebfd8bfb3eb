"""Overlapped tiling on the host (pipeline.tiled_super_resolution(..., overlap=)) and its plan (csrc/tile_plan.cpp through
srcfd_tiled_plan_overlap).  The host function IS the specification of the device path; here it is held, bit for bit, to
tests/tiled_overlap_ref.py, a per-pixel scalar restatement of the definition in include/srcfd.h written independently of it.
No device is needed."""
import ctypes as C
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tiled_overlap_ref as ref

# (TY, TX, C, lr, overlap, scale)
CASES = [(2, 3, 2, 4, 1, 1), (3, 2, 3, 10, 2, 2), (1, 4, 1, 10, 5, 1), (4, 1, 5, 6, 3, 3), (2, 2, 2, 8, (2, 0), 1), (2, 2, 1, 8, (0, 3), 2),
         (1, 1, 3, 5, 2, 1)]
IDS = ["x".join(str(v) for v in c[:4]) + f"_o{c[4]}_s{c[5]}".replace(" ", "") for c in CASES]


def _pl():
    return importlib.import_module("sr-for-cfd_amd.pipeline")


def _lib():
    return importlib.import_module("sr-for-cfd_amd._lib")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Up:
    """Duck-typed model: nearest up-scaling by `scale` plus an offset per call position, so that neighbouring tiles disagree in
    their overlaps.  `const`: every sample becomes that constant instead."""

    def __init__(self, scale, const=None, base=0):
        self.scale, self.const, self.base = scale, const, base

    def predict(self, x, in_affine=None, out_affine=None):
        x = np.asarray(x, np.float32)
        y = np.repeat(np.repeat(x, self.scale, axis=1), self.scale, axis=2)
        if self.const is not None:
            return np.full_like(y, self.const)
        off = (np.arange(x.shape[0], dtype=np.float32) + self.base) * np.float32(0.37)
        return (y + off.reshape(-1, 1, 1, 1)).astype(np.float32)


def _field(ty, tx, c, lr, overlap, seed=0):
    oy, ox = ref.pair(overlap)
    return np.random.default_rng(seed).standard_normal((ty * (lr - oy) + oy, tx * (lr - ox) + ox, c)).astype(np.float32)


_CACHE = {}


def _case(i):
    """field, samples, the host function's result and the reference's, once per case and left unchanged"""
    if i not in _CACHE:
        ty, tx, c, lr, o, s = CASES[i]
        field = _field(ty, tx, c, lr, o, seed=i)
        got = _pl().tiled_super_resolution(field, Up(s), lr, overlap=o)
        y = Up(s).predict(ref.cut(field, lr, o))
        want = ref.stitch(y, ty, tx, c, lr, lr, o)
        for a in (field, got, y, want):
            a.setflags(write=False)
        _CACHE[i] = (field, y, got, want)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_host_function_equals_the_per_pixel_reference(i):
    ty, tx, c, lr, o, s = CASES[i]
    oy, ox = ref.pair(o)
    field, y, got, want = _case(i)
    assert got.dtype == np.float32 and got.shape == want.shape == (field.shape[0] * s, field.shape[1] * s, c)
    np.testing.assert_array_equal(bits(got), bits(want))
    # the host function cuts what the reference cuts: the same samples reach the model
    seen = []

    class Spy(Up):
        def predict(self, x, **kw):
            seen.append(np.array(x))
            return super().predict(x, **kw)
    _pl().tiled_super_resolution(field, Spy(s), lr, overlap=o)
    np.testing.assert_array_equal(bits(seen[0]), bits(ref.cut(field, lr, o)))
    assert (oy, ox) != (0, 0)


def test_overlap_0_is_todays_result():
    pl = _pl()
    field = np.random.default_rng(3).standard_normal((20, 30, 3)).astype(np.float32)
    y = Up(2).predict(np.ascontiguousarray(field.reshape(2, 10, 3, 10, 3).transpose(0, 2, 4, 1, 3).reshape(18, 10, 10, 1)))
    want = y.reshape(2, 3, 3, 20, 20).transpose(0, 3, 1, 4, 2).reshape(40, 60, 3)
    for o in (0, (0, 0)):
        np.testing.assert_array_equal(bits(pl.tiled_super_resolution(field, Up(2), 10, overlap=o)), bits(want))
    np.testing.assert_array_equal(bits(pl.tiled_super_resolution(field, Up(2), 10)), bits(want))
    with pytest.raises(ValueError, match="multiple of the tile size"):
        pl.tiled_super_resolution(field[:19], Up(2), 10)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_constant_tiles_give_the_exact_constant(i):
    ty, tx, c, lr, o, s = CASES[i]
    for const in (np.float32(0.1), np.float32(-3.0000002), np.float32(1e-40), np.float32(3e38)):
        got = _pl().tiled_super_resolution(_field(ty, tx, c, lr, o), Up(s, const=const), lr, overlap=o)
        assert (bits(got) == bits(np.float32(const))).all(), const


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_outside_the_zones_a_pixel_has_its_tiles_bits_and_inside_it_lies_between(i):
    ty, tx, c, lr, o, s = CASES[i]
    oy, ox = ref.pair(o)
    field, y, got, _ = _case(i)
    hh = lr * s
    Sy, Sx = (lr - oy) * s, (lr - ox) * s
    zy, zx = ref.zones(ty, tx, lr, lr, hh, hh, o)
    t = y.reshape(ty, tx, c, hh, hh)
    H, W = got.shape[:2]
    n_out = n_one = 0
    for R in range(H):
        t1 = min(R // Sy, ty - 1)
        for X in range(W):
            u1 = min(X // Sx, tx - 1)
            own = t[t1, u1, :, R - t1 * Sy, X - u1 * Sx]
            if not zy[R, X] and not zx[R, X]:
                assert (bits(got[R, X]) == bits(own)).all(), (R, X)
                n_out += 1
            elif zy[R, X] != zx[R, X]:       # one axis: between the two contributions
                other = t[t1 - 1, u1, :, R - (t1 - 1) * Sy, X - u1 * Sx] if zy[R, X] else t[t1, u1 - 1, :, R - t1 * Sy, X - (u1 - 1) * Sx]
                lo, hi = np.minimum(own, other), np.maximum(own, other)
                assert ((lo <= got[R, X]) & (got[R, X] <= hi)).all(), (R, X, lo, got[R, X], hi)
                n_one += 1
    assert n_out > 0 and (n_one > 0 or ty * tx == 1)


@pytest.mark.parametrize("i", [1, 3, 4], ids=[IDS[1], IDS[3], IDS[4]])
def test_the_data_pins_order_direction_and_position(i):
    """The same samples stitched y before x, with w exchanged with 1 - w, and with the zone one row late each differ from the
    specification: a pass of the comparison above cannot come from inputs that do not tell them apart."""
    ty, tx, c, lr, o, s = CASES[i]
    _, y, got, want = _case(i)
    assert max(ref.pair(o)) * s >= 2      # a ramp of one entry is 0.5 both ways
    for variant in ("y_first", "flipped", "shifted"):
        if variant == "y_first" and (ty == 1 or tx == 1 or 0 in ref.pair(o)):
            continue        # no corner: the two orders are the same computation
        wrong = ref.stitch(y, ty, tx, c, lr, lr, o, variant=variant)
        assert (bits(wrong) != bits(got)).any(), variant
    assert (bits(want) == bits(got)).all()


def test_the_ramp_is_increasing_and_inside_0_1():
    for O in (1, 2, 3, 7, 40, 200, 800):
        w = np.array(ref.ramp(O), np.float32)
        assert (w > 0).all() and (w < 1).all() and (np.diff(w) > 0).all()


# ------------------------------------------------------------------------------------------------ Python-side refusals
def test_python_side_value_errors():
    pl = _pl()
    up = Up(2)
    with pytest.raises(ValueError, match=r"height 21 .*nearest sizes that fit are 18 and 26"):
        pl.tiled_super_resolution(np.zeros((21, 18, 1), np.float32), up, 10, overlap=2)
    with pytest.raises(ValueError, match=r"width 9 .*nearest sizes that fit are 10 and 17"):
        pl.tiled_super_resolution(np.zeros((10, 9, 1), np.float32), up, 10, overlap=(0, 3))
    with pytest.raises(ValueError, match=r"width 30 .*nearest sizes that fit are 26 and 34"):
        pl.tiled_super_resolution(np.zeros((18, 30, 1), np.float32), up, 10, overlap=2)
    with pytest.raises(ValueError, match="at most half a tile"):
        pl.tiled_super_resolution(np.zeros((10, 10, 1), np.float32), up, 10, overlap=6)
    with pytest.raises(ValueError, match="at least 0"):
        pl.tiled_super_resolution(np.zeros((10, 10, 1), np.float32), up, 10, overlap=(0, -1))
    with pytest.raises(ValueError, match="int or"):
        pl.tiled_super_resolution(np.zeros((10, 10, 1), np.float32), up, 10, overlap=(1, 2, 3))

    class Odd:
        def predict(self, x, **kw):
            return np.zeros((x.shape[0], 15, 15, 1), np.float32)
    with pytest.raises(ValueError, match="whole multiple of the input"):
        pl.tiled_super_resolution(np.zeros((18, 18, 1), np.float32), Odd(), 10, overlap=2)
    # the same model is fine without an overlap
    assert pl.tiled_super_resolution(np.zeros((20, 20, 1), np.float32), Odd(), 10).shape == (30, 30, 1)


def test_the_distributed_branch_only_changes_who_predicts():
    """distributed=True in a one-rank gloo group: the same bits."""
    import torch.distributed as dist
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        ty, tx, c, lr, o, s_ = CASES[1]
        field, _, got, _ = _case(1)
        np.testing.assert_array_equal(bits(_pl().tiled_super_resolution(field, Up(s_), lr, distributed=True, overlap=o)), bits(got))
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ the plan
def _raw(fn, *args, buf_len=1 << 16):
    L = _lib()
    buf = C.create_string_buffer(buf_len)
    rc = getattr(L.lib, fn)(*args, buf, len(buf))
    return rc, (buf.value.decode() if rc == 0 else L.last_error())


def _plan_py(lh, lw, hh, hw, ty, tx, c, oy, ox, max_chunk, model_chunk, align):
    """The overlapped plan, restated."""
    n = ty * tx * c
    bound = max_chunk if max_chunk > 0 else model_chunk
    chunk = min(n, max(bound // c, 1) * c)
    n_chunks = -(-n // chunk)
    a = min(max(align, 1), 16)
    v = next((k for k in (4, 2) if hw % k == 0 and a % (4 * k) == 0), 1)
    items = hh * (hw // v)
    bpt = -(-items // 256)
    chunks = [[i * chunk, min(chunk, n - i * chunk)] for i in range(n_chunks)]
    blended = oy > 0 or ox > 0
    p = {"n": n, "chunk": chunk, "n_chunks": n_chunks, "chunks": chunks, "v": v, "cut": {"grid": min(-(-n * lh * lw // 256), 1 << 20), "block": 256},
         "stitch": None if blended else {"block": 256, "items_per_tile": items, "blocks_per_tile": bpt, "grid": [k // c * bpt for _, k in chunks]},
         "intermediate_bytes": (n if blended else chunk) * hh * hw * 4, "overlap": [oy, ox], "stride": [lh - oy, lw - ox]}
    sy, sx = (hh // lh, hw // lw) if blended else (None, None)
    H, W = ty * (lh - oy) + oy, tx * (lw - ox) + ox
    p["field"] = [H, W]
    p["out"] = [H * sy, W * sx] if blended else [ty * hh, tx * hw]
    p["blend"] = {"grid": p["out"][0] * -(-p["out"][1] // 256), "block": 256, "blocks_per_row": -(-p["out"][1] // 256), "ramp": [oy * sy, ox * sx]} if blended else None
    return p


PLANS = [  # lh, lw, hh, hw, ty, tx, c, oy, ox, max_chunk, model_chunk, align
    (10, 10, 400, 400, 4, 4, 3, 2, 2, 0, 48, 16),       # config-5 scale: 34 x 34 x 3
    (10, 10, 400, 400, 4, 4, 3, 2, 2, 6, 48, 16),
    (10, 10, 400, 400, 4, 4, 3, 0, 0, 0, 48, 16),
    (5, 5, 10, 10, 3, 2, 3, 2, 1, 3, 1024, 4),
    (10, 10, 10, 10, 1, 4, 1, 5, 5, 0, 1024, 16),
    (8, 8, 8, 8, 2, 2, 2, 2, 0, 0, 3, 8),
    (8, 8, 16, 16, 2, 2, 1, 0, 3, 0, 1024, 16),
    (3, 400, 3, 400, 3, 1, 5, 1, 8, 0, 1024, 16),
    (6, 4, 18, 8, 2, 5, 8, 3, 2, 7, 1024, 16),
]


@pytest.mark.parametrize("case", PLANS, ids=[str(i) for i in range(len(PLANS))])
def test_plan_json_against_a_python_restatement(srcfd, case):
    lh, lw, hh, hw, ty, tx, c, oy, ox, max_chunk, model_chunk, align = case
    rc, text = _raw("srcfd_tiled_plan_overlap", lh, lw, 1, hh, hw, 1, ty, tx, c, oy, ox, max_chunk, model_chunk, align)
    assert rc == 0, text
    assert json.loads(text) == _plan_py(*case)
    got = srcfd.tiled_plan((lh, lw, 1), (hh, hw, 1), ty, tx, c, max_chunk or None, model_chunk, align, overlap=(oy, ox))
    want = _plan_py(*case)
    if (oy, ox) == (0, 0):      # the Python wrapper takes today's function for overlap 0
        want = {k: v for k, v in want.items() if k not in ("overlap", "stride", "field", "out", "blend")}
    assert got == want


def test_config_5_scale_intermediate():
    rc, text = _raw("srcfd_tiled_plan_overlap", 10, 10, 1, 400, 400, 1, 4, 4, 3, 2, 2, 0, 48, 16)
    p = json.loads(text)
    assert p["intermediate_bytes"] == 30720000 and p["field"] == [34, 34] and p["out"] == [1360, 1360] and p["blend"]["ramp"] == [80, 80]
    rc, text = _raw("srcfd_tiled_plan_overlap", 10, 10, 1, 400, 400, 1, 4, 4, 3, 2, 2, 3, 48, 16)
    p = json.loads(text)
    assert p["n_chunks"] == 16 and p["intermediate_bytes"] == 30720000      # all n samples, whatever the chunk


OLD_CASES = [dict(), dict(hh=20, hw=20, ty=2, tx=3), dict(hh=7, hw=7, align=4), dict(hh=20, hw=50, ty=3, tx=4, c=5, max_chunk=10, model_chunk=36),
             dict(hh=10, hw=10, ty=2, tx=2, max_chunk=2), dict(model_chunk=48), dict(align=8)]


@pytest.mark.parametrize("kw", OLD_CASES, ids=[str(i) for i in range(len(OLD_CASES))])
def test_the_old_plan_function_is_unchanged(kw):
    """srcfd_tiled_plan's JSON, byte for byte: the key order and the values of the format it documents, and nothing of the new keys."""
    a = dict(lh=10, lw=10, hh=400, hw=400, ty=4, tx=4, c=3, max_chunk=0, model_chunk=1024, align=16)
    a.update(kw)
    rc, text = _raw("srcfd_tiled_plan", a["lh"], a["lw"], 1, a["hh"], a["hw"], 1, a["ty"], a["tx"], a["c"], a["max_chunk"], a["model_chunk"], a["align"])
    assert rc == 0, text
    p = _plan_py(a["lh"], a["lw"], a["hh"], a["hw"], a["ty"], a["tx"], a["c"], 0, 0, a["max_chunk"], a["model_chunk"], a["align"])
    chunks = ",".join(f"[{f},{k}]" for f, k in p["chunks"])
    grids = ",".join(str(g) for g in p["stitch"]["grid"])
    want = (f'{{"n":{p["n"]},"chunk":{p["chunk"]},"n_chunks":{p["n_chunks"]},"chunks":[{chunks}],"v":{p["v"]},"cut":{{"grid":{p["cut"]["grid"]},"block":256}},'
            f'"stitch":{{"block":256,"items_per_tile":{p["stitch"]["items_per_tile"]},"blocks_per_tile":{p["stitch"]["blocks_per_tile"]},"grid":[{grids}]}},'
            f'"intermediate_bytes":{p["intermediate_bytes"]}}}')
    assert text == want
    # and overlap 0 through the new function: the same text, then the new keys
    rc, text0 = _raw("srcfd_tiled_plan_overlap", a["lh"], a["lw"], 1, a["hh"], a["hw"], 1, a["ty"], a["tx"], a["c"], 0, 0, a["max_chunk"], a["model_chunk"], a["align"])
    assert rc == 0 and text0.startswith(want[:-1] + ',"overlap":[0,0],') and text0.endswith(',"blend":null}')


@pytest.mark.parametrize("kw,words", [
    (dict(oy=-1), ["overlap of (-1, 2)", "0 or more"]),
    (dict(ox=-3), ["overlap of (2, -3)", "0 or more"]),
    (dict(oy=6), ["overlap of (6, 2)", "10 x 10", "at most half a tile"]),
    (dict(ox=2147483647), ["at most half a tile"]),
    (dict(hh=405), ["whole multiple of the input", "10 x 10 -> 405 x 400"]),
    (dict(hw=15, hh=20), ["whole multiple of the input", "20 x 15"]),
    (dict(ty=40000, tx=1, c=1, lh=32768, lw=4, hh=32768 * 2, hw=8, oy=1, ox=1), ["overlapped output of", "2147483647"]),
    (dict(ty=30000, tx=30000, c=1, lh=4, lw=4, hh=400, hw=400, oy=1, ox=1), ["blending stitch of 9000100 x 9000100", "workgroups"]),
    # everything the plan refuses today
    (dict(c=0), ["0 channels", "1 .. 8"]),
    (dict(c=9), ["9 channels"]),
    (dict(ty=0), ["0 x 4 tiles"]),
    (dict(ty=46341, tx=46341, c=1), ["2147488281 tile samples"]),
    (dict(ic=3), ["3 -> 1 channels"]),
    (dict(oc=2), ["1 -> 2 channels"]),
    (dict(model_chunk=0), ["no unchunked call size"]),
])
def test_plan_refusals_come_back_with_the_reason(kw, words):
    L = _lib()
    a = dict(lh=10, lw=10, ic=1, hh=400, hw=400, oc=1, ty=4, tx=4, c=3, oy=2, ox=2, max_chunk=0, model_chunk=1024, align=16)
    a.update(kw)
    rc, msg = _raw("srcfd_tiled_plan_overlap", *(a[k] for k in ("lh", "lw", "ic", "hh", "hw", "oc", "ty", "tx", "c", "oy", "ox", "max_chunk", "model_chunk", "align")))
    assert rc == L.EINVAL, (rc, msg)
    assert msg.startswith("srcfd_tiled_plan_overlap: tiles: "), msg
    for w in words:
        assert w in msg, (w, msg)


def test_entry_points_and_a_short_buffer():
    L = _lib()
    for name in ("srcfd_tiled_plan_overlap", "srcfd_tiler_create_overlap"):
        assert name in L.EXPORTED and getattr(L.lib, name).argtypes is not None, name
    rc, msg = _raw("srcfd_tiled_plan_overlap", 10, 10, 1, 400, 400, 1, 4, 4, 3, 2, 2, 0, 48, 16, buf_len=16)
    assert rc == L.EINVAL and "buffer too small" in msg
    h = C.c_void_p()
    assert L.lib.srcfd_tiler_create_overlap(None, 2, 2, 3, 1, 1, 0, C.byref(h)) == L.EINVAL and not h.value


def test_plan_checker_sweeps_the_source_map_under_the_sanitizers():
    """tools/tile_plan_check.cpp under AddressSanitizer + UBSan, on the CPU: beside the plans it walked before, the per-axis source
    map of tile_map.h (the statement the kernel runs) for every lh <= 12, overlap <= lh / 2, scale <= 4, T <= 4, and the ramps."""
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "sr-for-cfd_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "tile_plan_check"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "sr-for-cfd_amd", "lib", "tile_plan_check_asan")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    plans, axes = (int(v) for v in out.stdout.split()[:2])
    assert plans >= 8 * 6 * 8 * 5 * 8
    assert axes == sum((lh // 2 + 1) * 4 * 4 for lh in range(1, 13))
