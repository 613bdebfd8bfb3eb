"""The host-only plan of tiled super-resolution on the device (csrc/tile_plan.cpp through srcfd_tiled_plan), the sharded
path's row map (pipeline.tile_source_index) and the tiler's refusals that need no device.  What the plan says is what
csrc/tiles.hip launches; tests/test_gpu_tiled_device.py holds the result to numpy's reshape / transpose on the device."""
import ctypes as C
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ENCODER_H5, ROOT

IN10 = (10, 10, 1)


def _lib():
    return importlib.import_module("sr-for-cfd_amd._lib")


def _raw_plan(lh=10, lw=10, ic=1, hh=400, hw=400, oc=1, ty=4, tx=4, c=3, max_chunk=0, model_chunk=1024, align=16, buf_len=1 << 16):
    L = _lib()
    buf = C.create_string_buffer(buf_len)
    rc = L.lib.srcfd_tiled_plan(lh, lw, ic, hh, hw, oc, ty, tx, c, max_chunk, model_chunk, align, buf, len(buf))
    return rc, (json.loads(buf.value.decode()) if rc == 0 else L.last_error())


def test_entry_points_are_declared_and_bound():
    L = _lib()
    for name in ("srcfd_tiled_plan", "srcfd_tiler_create", "srcfd_tiler_destroy", "srcfd_tiler_set_stream", "srcfd_tiler_run",
                 "srcfd_tiles_cut_device", "srcfd_tiles_stitch_device"):
        assert name in L.EXPORTED and getattr(L.lib, name).argtypes is not None, name


@pytest.mark.parametrize("hw,v", [(400, 4), (20, 4), (10, 2), (50, 2), (7, 1)])
def test_vector_width_follows_the_row_length(srcfd, hw, v):
    p = srcfd.tiled_plan(IN10, (hw, hw, 1), 2, 3, 3)
    assert p["v"] == v
    assert p["stitch"]["items_per_tile"] == hw * (hw // v)
    assert p["stitch"]["blocks_per_tile"] == -(-hw * (hw // v) // 256) and p["stitch"]["block"] == 256


@pytest.mark.parametrize("align,v400,v10", [(16, 4, 2), (32, 4, 2), (256, 4, 2), (8, 2, 2), (4, 1, 1)])
def test_vector_width_follows_the_stated_alignment(srcfd, align, v400, v10):
    assert srcfd.tiled_plan(IN10, (400, 400, 1), 4, 4, 3, align_bytes=align)["v"] == v400
    assert srcfd.tiled_plan(IN10, (10, 10, 1), 4, 4, 3, align_bytes=align)["v"] == v10
    assert srcfd.tiled_plan(IN10, (7, 7, 1), 4, 4, 3, align_bytes=align)["v"] == 1


@pytest.mark.parametrize("c", [1, 2, 3, 5])
def test_chunks_are_whole_tiles_and_cover_the_samples_once(srcfd, c):
    ty, tx, hh, hw, model_chunk = 3, 4, 20, 50, 7 * c + 1
    n = ty * tx * c
    for max_chunk in (None, c, 2 * c, n - 1, n + 5):
        p = srcfd.tiled_plan(IN10, (hh, hw, 1), ty, tx, c, max_chunk, model_chunk)
        bound = max_chunk if max_chunk else model_chunk
        want = min(n, bound // c * c)
        assert p["n"] == n and p["chunk"] == want and p["chunk"] % c == 0, (max_chunk, p)
        at = 0
        for first, count in p["chunks"]:
            assert first == at and count % c == 0 and 0 < count <= p["chunk"], (max_chunk, p["chunks"])
            at += count
        assert at == n and len(p["chunks"]) == p["n_chunks"]
        assert all(count == p["chunk"] for _, count in p["chunks"][:-1])
        assert p["intermediate_bytes"] == p["chunk"] * hh * hw * 4
        # one stitch grid per chunk: blocks_per_tile workgroups for each of the chunk's tiles
        assert p["stitch"]["grid"] == [count // c * p["stitch"]["blocks_per_tile"] for _, count in p["chunks"]]
        assert p["cut"]["block"] == 256 and p["cut"]["grid"] == -(-n * 100 // 256)


def test_a_bound_below_one_tile_still_takes_a_whole_tile(srcfd):
    p = srcfd.tiled_plan(IN10, (10, 10, 1), 2, 2, 3, max_chunk=2)
    assert p["chunk"] == 3 and p["n_chunks"] == 4


def test_config_5(srcfd):
    p = srcfd.tiled_plan(IN10, (400, 400, 1), 4, 4, 3, None, 48)
    assert p["n"] == 48 and p["chunks"] == [[0, 48]] and p["v"] == 4 and p["intermediate_bytes"] == 30720000
    assert p["stitch"]["grid"] == [16 * 157]


@pytest.mark.parametrize("kw,words", [
    (dict(c=0), ["0 channels", "1 .. 8"]),
    (dict(c=9), ["9 channels", "1 .. 8"]),
    (dict(ty=0), ["0 x 4 tiles"]),
    (dict(tx=-1), ["4 x -1 tiles"]),
    (dict(ty=46341, tx=46341, c=1), ["2147488281 tile samples", "2147483647"]),
    (dict(ty=1 << 15, tx=1 << 15, c=2), ["2147483648 tile samples"]),
    (dict(ic=3), ["3 -> 1 channels", "one-channel"]),
    (dict(oc=2), ["1 -> 2 channels", "one-channel"]),
])
def test_refusals_come_back_as_a_status_with_the_reason(kw, words):
    L = _lib()
    rc, msg = _raw_plan(**kw)
    assert rc == L.EINVAL, (rc, msg)
    assert msg.startswith("srcfd_tiled_plan: tiles: "), msg
    for w in words:
        assert w in msg, (w, msg)


def test_a_short_buffer_is_refused_with_the_size_needed():
    L = _lib()
    rc, msg = _raw_plan(buf_len=16)
    assert rc == L.EINVAL and "buffer too small" in msg
    L.lib.srcfd_tiled_plan.argtypes  # bound
    assert L.lib.srcfd_tiled_plan(10, 10, 1, 400, 400, 1, 4, 4, 3, 0, 48, 16, None, 0) == L.EINVAL


def test_many_chunks_are_not_listed(srcfd):
    p = srcfd.tiled_plan(IN10, (10, 10, 1), 300, 300, 1, max_chunk=1)
    assert p["n"] == 90000 and p["n_chunks"] == 90000 and p["chunks"] is None and p["stitch"]["grid"] is None


@pytest.mark.parametrize("n", [9, 12, 48])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_tile_source_index_agrees_with_shard_range(n, world):
    pl = importlib.import_module("sr-for-cfd_amd.pipeline")
    shard = importlib.import_module("sr-for-cfd_amd.shard")
    idx = pl.tile_source_index(n, world)
    assert idx.dtype == np.int32 and idx.shape == (n,)
    per = -(-n // world)
    rows = []
    for r in range(world):
        lo, hi = shard.shard_range(n, r, world)
        assert hi - lo <= per
        np.testing.assert_array_equal(idx[lo:hi], r * per + np.arange(hi - lo))     # rank r's block starts at row r * per
        rows.append(set(idx[lo:hi].tolist()))
        assert rows[-1] <= set(range(r * per, (r + 1) * per))
    assert sum(len(s) for s in rows) == n == len(set().union(*rows)), "two ranks' rows overlap"
    assert 0 <= idx.min() and idx.max() < world * per


def test_tile_source_index_is_not_always_the_identity():
    """shard_range gives the longer blocks to the LOWER ranks, so two ranks always map to the identity (9 samples: rows 0-4 and
    5-8); from three ranks on a shorter block can precede another one and the map skips the padding rows."""
    pl = importlib.import_module("sr-for-cfd_amd.pipeline")
    np.testing.assert_array_equal(pl.tile_source_index(9, 2), np.arange(9))
    np.testing.assert_array_equal(pl.tile_source_index(9, 4), [0, 1, 2, 3, 4, 6, 7, 9, 10])
    np.testing.assert_array_equal(pl.tile_source_index(12, 8), [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14])


def test_a_tiler_on_a_host_only_model_is_enodev(srcfd):
    L = _lib()
    m = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1)
    h = C.c_void_p()
    rc = L.lib.srcfd_tiler_create(m._h, 2, 2, 3, 0, C.byref(h))
    assert rc == L.ENODEV and not h.value
    assert "srcfd_tiler_create" in L.last_error() and "host-only" in L.last_error()
    with pytest.raises(srcfd.NoDeviceError):
        srcfd.Tiler(m, 2, 2, 3)
    assert L.lib.srcfd_tiler_create(None, 2, 2, 3, 0, C.byref(h)) == L.EINVAL
    assert L.lib.srcfd_tiler_set_stream(None, None) == L.EINVAL
    L.lib.srcfd_tiler_destroy(None)   # a no-op


def test_device_path_refuses_a_duck_typed_model():
    pl = importlib.import_module("sr-for-cfd_amd.pipeline")

    class Up:
        def predict(self, x, in_affine=None, out_affine=None):
            return x
    with pytest.raises(TypeError, match="tiled_super_resolution"):
        pl.tiled_super_resolution_device(np.zeros((10, 10, 1), np.float32), Up())


def test_plan_checker_builds_and_passes_under_the_sanitizers():
    """tools/tile_plan_check.cpp + tile_plan.cpp under AddressSanitizer + UBSan, on the CPU: tile sizes, grids, channel counts, chunk
    bounds and alignments, up to the largest sample counts the plan accepts, and every refusal."""
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "sr-for-cfd_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "tile_plan_check"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "sr-for-cfd_amd", "lib", "tile_plan_check_asan")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert int(out.stdout.split()[0]) >= 8 * 6 * 8 * 5 * 8
