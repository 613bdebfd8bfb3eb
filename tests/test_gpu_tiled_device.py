"""Tiled super-resolution on the device (csrc/tiles.hip, srcfd_tiler_*, pipeline.tiled_super_resolution_device) on an MI355X.

Every comparison is BIT FOR BIT: the two kernels only move float32 values, so a cut equals numpy's reshape / transpose of the
field, a stitch equals numpy's reshape / transpose of the samples, and the whole device path equals
pipeline.tiled_super_resolution (the host path, unchanged) on the same model handle.  No tolerance anywhere.

The side-stream tests are what tests/test_gpu_stream_order.py asks of every stream-ordered entry point, for the three that
bind their stream to the handle instead of taking it per call (srcfd_tiler_run, srcfd_tiles_cut_device,
srcfd_tiles_stitch_device; include/srcfd.h says why its table does not list them).
"""
import importlib
import os
import signal
import socket

import numpy as np
import pytest

from conftest import ENCODER_H5, ROOT, STATS_TXT, require_gpu

import stream_order as so

pytestmark = pytest.mark.gpu
FILL = 0x7FA5A5A5        # a NaN payload no finite input can turn into: "never written"
GUARD = 64               # floats in front of and behind `out` inside its allocation


@pytest.fixture(autouse=True)
def _time_limit(request):
    """Every test here runs under its own time limit (each takes a few seconds)."""
    def _alarm(*_):
        raise TimeoutError(f"{request.node.name} exceeded its time limit")
    old = signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _pl():
    return importlib.import_module("sr-for-cfd_amd.pipeline")


def np_cut(field, ty, tx, c, lh, lw):
    """The tiles of pipeline.tiled_super_resolution: sample s = (ty_i * TX + tx_i) * C + c."""
    return np.ascontiguousarray(field.reshape(ty, lh, tx, lw, c).transpose(0, 2, 4, 1, 3).reshape(ty * tx * c, lh, lw, 1))


def np_stitch(y, ty, tx, c, hh, hw):
    return np.ascontiguousarray(y.reshape(ty, tx, c, hh, hw).transpose(0, 3, 1, 4, 2).reshape(ty * hh, tx * hw, c))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


_SHAPE_MODELS = {}


def shape_model(srcfd, h, w):
    """A one-layer h x w x 1 -> h x w x 1 model: the single-kernel calls take their sizes from the tiler's model and run no network."""
    if (h, w) not in _SHAPE_MODELS:
        spec = [dict(kind="conv2d", name="one", k=1, stride=1, same=True, act="linear", w=np.ones((1, 1, 1, 1), np.float32), b=np.zeros(1, np.float32))]
        _SHAPE_MODELS[(h, w)] = srcfd.SRModel.from_layers(spec, (h, w, 1), device=0)
    return _SHAPE_MODELS[(h, w)]


@pytest.fixture(scope="module")
def torch_(srcfd):
    require_gpu(srcfd)
    import torch
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. cut
@pytest.mark.parametrize("ty,tx,c,lh,lw", [(1, 1, 1, 10, 10), (2, 3, 3, 10, 10), (3, 2, 2, 10, 10), (1, 4, 5, 20, 20)])
def test_cut(srcfd, torch_, ty, tx, c, lh, lw):
    torch = torch_
    rng = np.random.default_rng(100 * ty + 10 * tx + c)
    t = srcfd.Tiler(shape_model(srcfd, lh, lw), ty, tx, c)
    field = rng.standard_normal((ty * lh, tx * lw, c)).astype(np.float32)
    ain, aout = (rng.standard_normal((c, 2)).astype(np.float32) for _ in range(2))
    x, a_in, a_out = t.cut(dev(torch, field), dev(torch, ain), dev(torch, aout))
    torch.cuda.synchronize()
    assert_same_bits(x.cpu().numpy(), np_cut(field, ty, tx, c, lh, lw), "x")
    assert_same_bits(a_in.cpu().numpy(), np.tile(ain, (ty * tx, 1)), "in_affine")
    assert_same_bits(a_out.cpu().numpy(), np.tile(aout, (ty * tx, 1)), "out_affine")
    # one affine only, and none
    x2, no_in, only_out = t.cut(dev(torch, field), None, dev(torch, aout))
    assert no_in is None
    assert_same_bits(only_out.cpu().numpy(), np.tile(aout, (ty * tx, 1)), "out_affine alone")
    x3, n1, n2 = t.cut(dev(torch, field))
    assert n1 is None and n2 is None
    assert_same_bits(x2.cpu().numpy(), x.cpu().numpy())
    assert_same_bits(x3.cpu().numpy(), x.cpu().numpy())
    t.close()


# ------------------------------------------------------------------------------------------------ 2. stitch alone
def _guarded_out(torch, shape, offset=GUARD):
    """`out` of `shape` inside a larger allocation, everything pre-filled with FILL; `offset` floats in front of it (64: 256-byte
    aligned like a fresh allocation; 65, 66: 4- and 8-byte aligned, which narrows the stitch's vector width)."""
    size = int(np.prod(shape))
    big = torch.full((offset + size + GUARD,), FILL, dtype=torch.int32, device="cuda")
    return big, big[offset:offset + size].view(torch.float32).view(shape)


@pytest.mark.parametrize("c", [1, 2, 3, 5])
@pytest.mark.parametrize("hh,hw", [(7, 5), (10, 10), (6, 50), (20, 20), (3, 400)])
def test_stitch_alone(srcfd, torch_, hh, hw, c):
    torch = torch_
    ty, tx = 2, 3
    n = ty * tx * c
    rng = np.random.default_rng(1000 * hh + 10 * hw + c)
    t = srcfd.Tiler(shape_model(srcfd, hh, hw), ty, tx, c)
    assert t.plan()["v"] == (4 if hw % 4 == 0 else 2 if hw % 2 == 0 else 1)
    y = rng.standard_normal((n, hh, hw)).astype(np.float32)
    want = np_stitch(y, ty, tx, c, hh, hw)
    # a permuted index into a y with more rows than samples
    rows = n + 3
    perm = rng.permutation(rows)[:n].astype(np.int32)
    y_big = rng.standard_normal((rows, hh, hw)).astype(np.float32)
    y_big[perm] = y
    y_d, y_big_d, perm_d = dev(torch, y), dev(torch, y_big), dev(torch, perm)
    size = want.size
    fill = np.full(size, FILL, np.uint32)

    def check(big, offset, expect_bits, what):
        got = big.cpu().numpy().view(np.uint32)
        assert (got[:offset] == FILL).all() and (got[offset + size:] == FILL).all(), f"{what}: the guard area was written"
        np.testing.assert_array_equal(got[offset:offset + size], expect_bits, err_msg=what)

    # the whole range at the three alignments of `out` (the plan narrows V for the last two)
    for offset in (GUARD, GUARD + 1, GUARD + 2):
        for mode in ("identity", "index"):
            big, out = _guarded_out(torch, want.shape, offset)
            if mode == "identity":
                t.stitch(y_d, out)
            else:
                t.stitch(y_big_d, out, src_index=perm_d)
            check(big, offset, bits(want).ravel(), f"{mode}, out at +{offset} floats")

    # every sub-range [s0, s1) at multiples of C, each into a fresh pre-filled `out`: only its tiles are written
    tile_of = np_stitch(np.repeat(np.arange(n) // c, hh * hw).reshape(n, hh, hw).astype(np.float32), ty, tx, c, hh, hw).astype(np.int64).ravel()
    for mode in ("identity", "index"):
        for a in range(0, ty * tx):
            for b in range(a + 1, ty * tx + 1):
                big, out = _guarded_out(torch, want.shape)
                if mode == "identity":
                    t.stitch(y_d[a * c:b * c], out, a * c, b * c)
                else:
                    t.stitch(y_big_d, out, a * c, b * c, src_index=perm_d)
                inside = (tile_of >= a) & (tile_of < b)
                check(big, GUARD, np.where(inside, bits(want).ravel(), fill), f"{mode}, tiles [{a}, {b})")
    # an empty range writes nothing; a range that splits a tile, runs past n or has too few rows is refused
    big, out = _guarded_out(torch, want.shape)
    t.stitch(y_d, out, c, c)
    check(big, GUARD, fill, "empty range")
    if c > 1:
        with pytest.raises(ValueError, match="whole tiles"):
            t.stitch(y_d, out, 1, c)
    with pytest.raises(ValueError):
        t.stitch(y_d, out, 0, n + c)
    with pytest.raises(ValueError, match="rows"):
        t.stitch(y_d[:c], out, 0, 2 * c)
    # an index that points outside y leaves its tile as it was
    bad = perm.copy()
    bad[c] = rows + 7                       # first sample of tile 1
    t.stitch(y_big_d, out, src_index=dev(torch, bad))
    check(big, GUARD, np.where(tile_of == 1, fill, bits(want).ravel()), "index outside y")
    t.close()


# ------------------------------------------------------------------------------------------------ 3. end to end
_MODELS = {}


def _model(srcfd, enc_weights, dec_weights, name):
    """'d10' / 'd20': encoder_10 + a seeded decoder_10 / decoder_20 (layer by layer); 'd400': the fused encoder_10 + decoder_400."""
    if name not in _MODELS:
        fam = importlib.import_module("sr-for-cfd_amd.family")
        dec = dec_weights if name == "d400" else fam.synthetic_decoder_weights(int(name[1:]), seed=20 + int(name[1:]))
        _MODELS[name] = srcfd.SRModel.from_weights(enc_weights, dec, device=0)
    return _MODELS[name]


def _golden_affines(srcfd):
    lr, hr = srcfd.load_stats(STATS_TXT, 10, 400)
    return (np.array([lr[c] for c in "uvp"], np.float32), np.array([hr[c] for c in "uvp"], np.float32))


def _field(ty, tx, c, seed):
    return np.random.default_rng(seed).standard_normal((ty * 10, tx * 10, c)).astype(np.float32)


E2E = [("d10", "fp32", 3, 2, 3, False), ("d10", "bf16", 3, 2, 3, False), ("d20", "f16", 2, 2, 2, False), ("d400", "f16", 2, 2, 3, True)]
_HOST = {}


@pytest.mark.parametrize("chunks", [None, 1, 2], ids=["unchunked", "chunk_C", "chunk_2C"])
@pytest.mark.parametrize("name,precision,ty,tx,c,affines", E2E, ids=[f"{e[0]}_{e[1]}" for e in E2E])
def test_end_to_end_equals_the_host_path(srcfd, torch_, enc_weights, dec_weights, name, precision, ty, tx, c, affines, chunks):
    torch = torch_
    pl = _pl()
    m = _model(srcfd, enc_weights, dec_weights, name)
    m.precision = precision
    field = _field(ty, tx, c, 7 * c + ty)
    ain, aout = _golden_affines(srcfd) if affines else (None, None)
    key = (name, precision)
    if key not in _HOST:       # the host path, once per model and precision, left unchanged
        _HOST[key] = pl.tiled_super_resolution(field, m, 10, in_affine=ain, out_affine=aout).copy()
        _HOST[key].setflags(write=False)
    want = _HOST[key]
    max_chunk = None if chunks is None else chunks * c
    # tensor in / tensor out
    got = pl.tiled_super_resolution_device(dev(torch, field), m, 10, in_affine=ain, out_affine=aout, max_chunk=max_chunk)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    assert_same_bits(got.cpu().numpy(), want, "tensor in / tensor out")
    tiler = m._tilers[(ty, tx, c, max_chunk)]
    plan = tiler.plan()
    assert plan["chunk"] == (ty * tx * c if chunks is None else chunks * c) and plan["n_chunks"] == (1 if chunks is None else ty * tx // chunks)
    # numpy in / numpy out, and `out=`
    got_np = pl.tiled_super_resolution_device(field, m, 10, in_affine=ain, out_affine=aout, max_chunk=max_chunk)
    assert isinstance(got_np, np.ndarray)
    assert_same_bits(got_np, want, "numpy in / numpy out")
    out = torch.zeros(want.shape, dtype=torch.float32, device="cuda")
    ret = pl.tiled_super_resolution_device(dev(torch, field), m, 10, in_affine=None if ain is None else dev(torch, ain),
                                           out_affine=None if aout is None else dev(torch, aout), out=out, max_chunk=max_chunk)
    assert ret is out
    assert_same_bits(out.cpu().numpy(), want, "out=")
    assert m._tilers[(ty, tx, c, max_chunk)] is tiler      # one tiler per (model, TY, TX, C, max_chunk), reused by the calls above


@pytest.mark.parametrize("chunks", [None, 1, 2], ids=["unchunked", "chunk_C", "chunk_2C"])
def test_nan_guard_and_counter_pass_through(srcfd, torch_, enc_weights, dec_weights, chunks):
    """The fused 400x400 model, 2x2 tiles, C = 3, f16, the golden affines, SRCFD_FLAG_NAN_GUARD and the counter: one poisoned
    component of one tile.  The reference is srcfd_predict of the same tiles with the guard, stitched by numpy."""
    torch = torch_
    m = _model(srcfd, enc_weights, dec_weights, "d400")
    m.precision = "f16"
    ty, tx, c = 2, 2, 3
    field = _field(ty, tx, c, 99)
    field[13, 4, 1] = np.nan                 # tile (1, 0), component 1: sample 7
    ain, aout = _golden_affines(srcfd)
    y, bad = m.predict(np_cut(field, ty, tx, c, 10, 10), in_affine=np.tile(ain, (ty * tx, 1)), out_affine=np.tile(aout, (ty * tx, 1)),
                       nan_guard=True, return_nonfinite=True)
    assert bad > 0 and np.isfinite(y).all() and (y[7] == 0).all()
    want = np_stitch(y, ty, tx, c, 400, 400)
    t = srcfd.Tiler(m, ty, tx, c, None if chunks is None else chunks * c)
    out = torch.empty(want.shape, dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    t.run(dev(torch, field), out, dev(torch, ain), dev(torch, aout), nan_guard=True, nonfinite=cnt)
    assert_same_bits(out.cpu().numpy(), want)
    assert int(cnt.item()) == 5 + bad       # added to
    t.close()


def test_config_5_at_full_size(srcfd, torch_, enc_weights, dec_weights):
    """40 x 40 x 3 -> 1600 x 1600 x 3 through 4 x 4 tiles, f16: 48 samples, one chunk."""
    torch = torch_
    pl = _pl()
    m = _model(srcfd, enc_weights, dec_weights, "d400")
    m.precision = "f16"
    field = _field(4, 4, 3, 5)
    want = pl.tiled_super_resolution(field, m, 10)
    got = pl.tiled_super_resolution_device(dev(torch, field), m, 10)
    assert tuple(got.shape) == (1600, 1600, 3)
    assert_same_bits(got.cpu().numpy(), want)
    assert m._tilers[(4, 4, 3, None)].plan()["chunks"] == [[0, 48]]


def test_bad_arguments(srcfd, torch_, enc_weights, dec_weights):
    pl = _pl()
    m = _model(srcfd, enc_weights, dec_weights, "d10")
    with pytest.raises(ValueError, match="multiple of the tile size"):
        pl.tiled_super_resolution_device(np.zeros((15, 10, 1), np.float32), m, 10)
    with pytest.raises(ValueError, match="lr_dim"):
        pl.tiled_super_resolution_device(np.zeros((20, 20, 1), np.float32), m, 20)
    with pytest.raises(ValueError, match="channels"):
        pl.tiled_super_resolution_device(np.zeros((10, 10, 9), np.float32), m, 10)


# ------------------------------------------------------------------------------------------------ 4. side stream
@pytest.fixture(scope="module")
def ctx(torch_):
    class Ctx:
        pass
    c = Ctx()
    c.torch = torch_
    c.delay = so.Delay(torch_)
    c.S = torch_.cuda.Stream()
    return c


@pytest.mark.parametrize("max_chunk", [None, 3], ids=["one_chunk_graph", "chunks_of_C"])
def test_side_stream_tiler_run(srcfd, ctx, enc_weights, dec_weights, max_chunk):
    """srcfd_tiler_run on a non-default stream, field and affines arriving behind the delay: the cut, every chunk's forward (one
    chunk: plain launches, the hipGraph capture, a replay) and every stitch follow the bound stream."""
    torch = ctx.torch
    m = _model(srcfd, enc_weights, dec_weights, "d10")
    m.precision = "bf16"
    ty, tx, c = 3, 2, 3
    t = srcfd.Tiler(m, ty, tx, c, max_chunk)
    rng = np.random.default_rng(31)
    f_real, f_decoy = dev(torch, _field(ty, tx, c, 1)), dev(torch, _field(ty, tx, c, 2))

    def affine():
        return dev(torch, np.stack([rng.standard_normal(c) * 0.1, rng.uniform(0.5, 1.5, c)], 1).astype(np.float32))
    ai_r, ao_r, ai_d, ao_d = affine(), affine(), affine(), affine()
    ref_real = t.run(f_real, torch.empty(t.out_shape, device="cuda"), ai_r, ao_r)
    torch.cuda.synchronize()
    want = _pl().tiled_super_resolution(f_real.cpu().numpy(), m, 10, in_affine=ai_r.cpu().numpy(), out_affine=ao_r.cpu().numpy())
    assert_same_bits(ref_real.cpu().numpy(), want, "default stream vs the host path")
    ref_decoy = t.run(f_decoy, torch.empty(t.out_shape, device="cuda"), ai_d, ao_d)     # last: the buffers now derive from the decoy
    torch.cuda.synchronize()
    assert not torch.equal(ref_real, ref_decoy)
    f, ai, ao, out = torch.empty_like(f_real), torch.empty_like(ai_r), torch.empty_like(ao_r), torch.empty_like(ref_real)
    arrivals = [so.Arrival(f, f_decoy, f_real), so.Arrival(ai, ai_d, ai_r), so.Arrival(ao, ao_d, ao_r)]
    for i in range(3):
        what = f"tiler_run max_chunk={max_chunk} call {i + 1}"
        o = so.delayed_call(torch, ctx.delay, ctx.S, arrivals, lambda: t.run(f, out, ai, ao, stream=ctx.S), [out], stale=[(out, ref_decoy)], label=what)
        print(f"[tiled side stream] {what}: enqueue {o.enqueue_s * 1e3:.2f} ms, stream busy at return: {o.pending}, plan {m.last_plan()}")
        so.assert_pending(o, what)
        so.assert_bit_equal(o.clones[0], ref_real, what)
    t.set_stream(torch.cuda.default_stream())
    t.close()


def test_side_stream_cut_and_stitch(srcfd, ctx):
    """The two single-kernel calls on a non-default stream."""
    torch = ctx.torch
    ty, tx, c, h, w = 2, 3, 3, 20, 20
    t = srcfd.Tiler(shape_model(srcfd, h, w), ty, tx, c)
    rng = np.random.default_rng(8)
    f_real, f_decoy = (dev(torch, rng.standard_normal((ty * h, tx * w, c)).astype(np.float32)) for _ in range(2))
    a_real, a_decoy = (dev(torch, rng.standard_normal((c, 2)).astype(np.float32)) for _ in range(2))
    f, a = torch.empty_like(f_real), torch.empty_like(a_real)
    got = []
    o = so.delayed_call(torch, ctx.delay, ctx.S, [so.Arrival(f, f_decoy, f_real), so.Arrival(a, a_decoy, a_real)],
                        lambda: got.extend(t.cut(f, a, a, stream=ctx.S)), [], label="tiles_cut")
    so.assert_pending(o, "tiles_cut")
    ctx.S.synchronize()
    assert_same_bits(got[0].cpu().numpy(), np_cut(f_real.cpu().numpy(), ty, tx, c, h, w), "cut on a side stream")
    assert_same_bits(got[1].cpu().numpy(), np.tile(a_real.cpu().numpy(), (ty * tx, 1)), "affines on a side stream")
    assert_same_bits(got[2].cpu().numpy(), np.tile(a_real.cpu().numpy(), (ty * tx, 1)))

    n = ty * tx * c
    y_real, y_decoy = (dev(torch, rng.standard_normal((n, h, w)).astype(np.float32)) for _ in range(2))
    i_real = dev(torch, rng.permutation(n).astype(np.int32))
    i_decoy = dev(torch, np.arange(n, dtype=np.int32))
    y, idx = torch.empty_like(y_real), torch.empty_like(i_real)
    out = torch.empty(t.out_shape, device="cuda")
    ref_decoy = dev(torch, np_stitch(y_decoy.cpu().numpy(), ty, tx, c, h, w))
    o = so.delayed_call(torch, ctx.delay, ctx.S, [so.Arrival(y, y_decoy, y_real), so.Arrival(idx, i_decoy, i_real)],
                        lambda: t.stitch(y, out, src_index=idx, stream=ctx.S), [out], stale=[(out, ref_decoy)], label="tiles_stitch")
    so.assert_pending(o, "tiles_stitch")
    assert_same_bits(o.clones[0].cpu().numpy(), np_stitch(y_real.cpu().numpy()[i_real.cpu().numpy()], ty, tx, c, h, w), "stitch on a side stream")
    t.set_stream(torch.cuda.default_stream())
    t.close()


# ------------------------------------------------------------------------------------------------ 5. ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, backend, q):
    import sys
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    device = rank if backend == "nccl" else 0
    torch.cuda.set_device(device)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        srcfd = importlib.import_module("srcfd_amd")
        fam = importlib.import_module("sr-for-cfd_amd.family")
        pl = _pl()
        enc = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
        m = srcfd.SRModel.from_weights(enc, fam.synthetic_decoder_weights(10, seed=30), device=device)
        ty, tx, c = 1, 3, 3
        field = _field(ty, tx, c, 77)
        rng = np.random.default_rng(3)
        ain, aout = (np.stack([rng.standard_normal(c) * 0.1, rng.uniform(0.5, 1.5, c)], 1).astype(np.float32) for _ in range(2))
        single = pl.tiled_super_resolution_device(field, m, 10, in_affine=ain, out_affine=aout)
        host = pl.tiled_super_resolution(field, m, 10, in_affine=ain, out_affine=aout)
        got = pl.tiled_super_resolution_device(torch.from_numpy(field).cuda(), m, 10, in_affine=ain, out_affine=aout, distributed=True)
        got_np = pl.tiled_super_resolution_device(field, m, 10, in_affine=ain, out_affine=aout, distributed=True)
        shard = importlib.import_module("sr-for-cfd_amd.shard").shard_range(ty * tx * c, rank, world)
        q.put((rank, shard, bool(np.array_equal(bits(single), bits(host))), bool(np.array_equal(bits(got.cpu().numpy()), bits(single))),
               bool(np.array_equal(bits(got_np), bits(single))), pl.tile_source_index(ty * tx * c, world).tolist()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _run_ranks(world, backend):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")            # fresh child processes: none inherits an initialised GPU
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = sorted(q.get(timeout=100) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=15)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return got


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_on_one_gpu_gloo(srcfd, torch_, world):
    """A 1 x 3 grid with C = 3 (n = 9) over ranks that share one GPU, backend gloo: every rank's stitched field equals the
    single-process one, which equals the host path.  Two ranks: blocks of 5 and 4 samples; shard_range gives the longer block to
    the lower rank, so their row map IS the identity (rows 0-4 and 5-8).  Four ranks: blocks of 3, 2, 2, 2 in rows 0-2, 3-4,
    6-7, 9-10 of the gathered buffer -- the map that is not."""
    got = _run_ranks(world, "gloo")
    sizes = [hi - lo for _, (lo, hi), *_ in got]
    assert sizes == ([5, 4] if world == 2 else [3, 2, 2, 2])
    for rank, _, single_is_host, dist_is_single, dist_np_is_single, index in got:
        assert single_is_host and dist_is_single and dist_np_is_single, (rank, single_is_host, dist_is_single, dist_np_is_single)
        assert (index == list(range(9))) == (world == 2)


def test_two_ranks_nccl(srcfd, torch_):
    """The same over the real `nccl` (= RCCL) backend, one all_gather_into_tensor of device tensors.  Needs two visible devices."""
    if torch_.cuda.device_count() < 2:
        pytest.skip(f"needs 2 GPUs for the RCCL backend, {torch_.cuda.device_count()} visible: the nccl branch of "
                    "tiled_super_resolution_device(distributed=True) is not executed on this machine")
    for rank, _, single_is_host, dist_is_single, dist_np_is_single, _ in _run_ranks(2, "nccl"):
        assert single_is_host and dist_is_single and dist_np_is_single, rank
