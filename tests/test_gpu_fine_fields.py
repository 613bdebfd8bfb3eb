"""Device fields in and out of the fine solver, on an MI355X: srcfd_fine_batch_init_from_fields_device (handoff_kernel fed from a
caller's tensor, through the float64 resampler or not), srcfd_fine_batch_get_fields_device (fields_kernel, its mirror image),
srcfd_resample_device_f64, and the sweeps built on them (fine.compare_warm_starts, fine.run_nested_simulations).

The bit reference is never the new code: a state written from device fields is compared with `FineSolverBatch.init(Var)` of a host
array built from the same values with numpy, fields read on the device with `fields(i)` from `get_state`, the float64 resampler
with the float32 one on float-valued input and with numpy's float64 products at the 1e-12 bar of tests/test_resample.py.

Meshes: 37 x 29 and 29 x 37 (no multiple of the 32-wide tile, nx != ny), 33 x 32 and 64 x 65 (one past a tile), 3 x 3 (the
smallest legal mesh); batches of five cases of which cases 3 and 0, in that order, take the two fields."""
import ctypes as C
import importlib
import os
import signal

import numpy as np
import pytest

from conftest import ENCODER_H5, GOLDEN, STATS_TXT, require_gpu

import guard_bands as gb
import stream_order as so

pytestmark = pytest.mark.gpu

RUNNING = 0
MESHES = [(37, 29), (29, 37), (33, 32), (64, 65), (3, 3)]
KINDS = ["ldc_quick", "bfs_upwind"]
CASES = [3, 0]
REL = 1e-12                   # the bar of tests/test_resample.py: |out - numpy|_max <= 1e-12 |numpy|_max
_BFS = {"step_height": 1.0, "h": 2.0, "Ub": 1.0}


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


@pytest.fixture(scope="module")
def fine(srcfd):
    require_gpu(srcfd)
    return importlib.import_module("sr-for-cfd_amd.fine")


@pytest.fixture(scope="module")
def coarse():
    return importlib.import_module("sr-for-cfd_amd.coarse")


@pytest.fixture(scope="module")
def rs():
    return importlib.import_module("sr-for-cfd_amd.resample")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("sr-for-cfd_amd._lib")


@pytest.fixture(scope="module")
def torch(fine):
    return __import__("torch")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def _same(a, b):
    assert np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).shape == np.asarray(b).shape
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _extent(kind):
    return (1.0, 1.0) if kind == "ldc_quick" else (10.0, 3.0)


def _problems(fine, coarse, kind, nx, ny):
    """Five cases that differ in Reynolds number and, for the cavity, in their boundary values."""
    if kind == "ldc_quick":
        bcs = (coarse.LDC_SINGLE_LID, coarse.LDC_DOUBLE_LID, coarse.LDC_SINGLE_LID, coarse.LDC_DOUBLE_LID, coarse.LDC_SINGLE_LID)
        return [fine.problem(Re, nx, ny, 1.0, 1.0, 0.001, "QUICK", None, bc) for Re, bc in zip((100.0, 400.0, 250.0, 700.0, 1000.0), bcs)]
    return [fine.problem(Re, nx, ny, 10.0, 3.0, 0.002, "UPWIND", None, None, bfs=_BFS) for Re in (100.0, 400.0, 250.0, 300.0, 200.0)]


def _fields(nx, ny, n_fields=2, seed=0, h=None, w=None):
    """(3 * n_fields, h, w) float64, O(0.1), every value different and none of them a float."""
    h, w = ny if h is None else h, nx if w is None else w
    return np.random.default_rng(1000 * nx + ny + seed).normal(0.0, 0.1, (3 * n_fields, h, w))


def _host_var(fields, n_cases, cases, nx, ny):
    """The host recipe: zeros (n_cases, 3, nx+2, ny+2) with Var[cases[w], k, 1+i, 1+j] = fields[3 w + k][j, i] in float64."""
    var = np.zeros((n_cases, 3, nx + 2, ny + 2))
    for w, c in enumerate(cases):
        for k in range(3):
            var[c, k, 1:-1, 1:-1] = np.asarray(fields[3 * w + k], dtype=np.float64).T
    return var


def _state(b):
    return b.Var, b.iterations.tolist(), b.status.tolist(), _bits(b.rms).tolist(), b.counters()["last_sweeps"]


def _check_against_host_init(fine, pbs, b, var_host, iterations=3):
    """`b` has just been started from device fields: the state, ghosts and corners included, and the run that follows are those of
    a batch given `var_host` through init."""
    ref = fine.FineSolverBatch(pbs)
    ref.init(var_host)
    got = b.Var
    _same(got, ref.Var)
    nx, ny = pbs[0].nx, pbs[0].ny
    assert (_bits(got[:, :, [0, 0, nx + 1, nx + 1], [0, ny + 1, 0, ny + 1]]) == 0).all()
    assert b.iterations.tolist() == [0] * len(pbs) and b.status.tolist() == [RUNNING] * len(pbs)
    if iterations:
        b.run(iterations)
        ref.run(iterations)
        sb, sr = _state(b), _state(ref)
        _same(sb[0], sr[0])
        assert sb[1:] == sr[1:]
    ref.close()
    return got


# ---------------------------------------------------------------------------------------------- 1: fields as they are
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nx,ny", MESHES)
def test_init_from_fields_equals_host_init(fine, coarse, torch, nx, ny, kind):
    pbs = _problems(fine, coarse, kind, nx, ny)
    zero = fine.FineSolverBatch(pbs)
    zero_var = zero.Var
    zero.close()
    F = _fields(nx, ny)
    b = fine.FineSolverBatch(pbs)
    for dtype in (np.float64, np.float32):
        Fd = F.astype(dtype)
        b.run(1)                                  # a state that is not the initial one: the call has to clear it
        b.init_from_fields(torch.from_numpy(Fd).cuda(), cases=CASES)
        got = _check_against_host_init(fine, pbs, b, _host_var(Fd, 5, CASES, nx, ny))      # float32: the widened values
        _same(got[[1, 2, 4]], zero_var[[1, 2, 4]])
        assert not np.array_equal(got[3], got[0]) and np.abs(got[[3, 0], :, 1:-1, 1:-1]).max() > 1e-2
    # cases=None: field i into case i, the cases behind them from zero; and a numpy array, uploaded by the call
    b.init_from_fields(F)
    got = _check_against_host_init(fine, pbs, b, _host_var(F, 5, [0, 1], nx, ny), iterations=0)
    _same(got[2:], zero_var[2:])
    b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_single_case_solver_forms(fine, coarse, torch, kind):
    nx, ny = 37, 29
    pb = _problems(fine, coarse, kind, nx, ny)[1]
    F = _fields(nx, ny, 1)
    s = fine.FineSolver(pb)
    s.init_from_fields(torch.from_numpy(F).cuda())
    ref = fine.FineSolver(pb)
    ref.init(_host_var(F, 1, [0], nx, ny)[0])
    _same(s.Var, ref.Var)
    assert s.run(3) == ref.run(3) == 3
    _same(s.Var, ref.Var)
    _same(s.rms, ref.rms)
    for dtype, np_dtype in ((torch.float64, np.float64), (torch.float32, np.float32)):
        got = s.fields_device(dtype=dtype).cpu().numpy()
        _same(got, np.stack([ref.fields()[c] for c in "uvp"]).astype(np_dtype))
    s.close()
    ref.close()


# ---------------------------------------------------------------------------------------------- 2: through the resampler
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nx,ny", MESHES)
def test_init_from_fields_through_the_resampler(fine, coarse, torch, nx, ny, kind):
    lx, ly = _extent(kind)
    pbs = _problems(fine, coarse, kind, nx, ny)
    R = fine.interpolation_resampler(10, 10, nx, ny, lx, ly)
    Ry, Rx = fine.interpolation_matrices(10, 10, nx, ny, lx, ly)
    F64 = _fields(nx, ny, h=10, w=10)
    b = fine.FineSolverBatch(pbs)
    # float32 input: srcfd_resample_device's own output, taken to the host and through init
    F32 = F64.astype(np.float32)
    t32 = torch.from_numpy(F32).cuda()
    resampled = R.apply_device(t32).cpu().numpy()
    b.init_from_fields(t32, cases=CASES, resampler=R)
    got = _check_against_host_init(fine, pbs, b, _host_var(resampled, 5, CASES, nx, ny))
    # float64 input, not float-representable: numpy's float64 products, per field
    b.init_from_fields(torch.from_numpy(F64).cuda(), cases=CASES, resampler=R)
    got = b.Var
    for F, var in ((F32.astype(np.float64), _host_var(resampled, 5, CASES, nx, ny)), (F64, got)):
        for w, c in enumerate(CASES):
            for k in range(3):
                want = Ry @ F[3 * w + k] @ Rx.T
                err = np.abs(var[c, k, 1:-1, 1:-1].T - want).max() / np.abs(want).max()
                print(f"{nx} x {ny} {kind} case {c} plane {k}: rel max error vs numpy {err:.3e}")
                assert err <= REL, (c, k, err)
    _check_against_host_init(fine, pbs, b, _host_var(R.apply_device_f64(torch.from_numpy(F64).cuda()).cpu().numpy(), 5, CASES, nx, ny))
    b.close()
    R.close()


# ---------------------------------------------------------------------------------------------- 3: the float64 resampler
def _resamplers(rs):
    """(name, Ry, Rx): the general two-product path on one tile and on ragged tiles with a ragged 16-deep k loop, and the three paths
    that skip an identity factor."""
    im = rs.interp_matrix
    return [("10x10->37x29", im(10, 3.0, 37, 3.0), im(10, 10.0, 29, 10.0)),
            ("40x50->70x37", im(40, 1.0, 70, 1.0), im(50, 1.0, 37, 1.0)),
            ("rx identity", im(10, 1.0, 37, 1.0), np.eye(10)),
            ("ry identity", np.eye(10), im(10, 1.0, 29, 1.0)),
            ("both identity", np.eye(10), np.eye(10))]


def test_resample_device_f64(fine, rs, torch):
    rng = np.random.default_rng(5)
    for name, Ry, Rx in _resamplers(rs):
        R = rs.Resampler(Ry, Rx)
        F = rng.normal(0.0, 0.1, (6, R.in_h, R.in_w))
        F32 = F.astype(np.float32)
        want32 = R.apply_device(torch.from_numpy(F32).cuda())
        got32 = R.apply_device_f64(torch.from_numpy(F32.astype(np.float64)).cuda())
        assert got32.dtype == torch.float64 and tuple(got32.shape) == (6, R.out_h, R.out_w)
        _same(got32.cpu().numpy(), want32.cpu().numpy())                       # float-valued input: the float32 entry's bits
        got = R.apply_device_f64(torch.from_numpy(F).cuda()).cpu().numpy()
        want = np.einsum("ah,zhw,bw->zab", np.asarray(Ry), F, np.asarray(Rx))
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name}: float64 input, rel max error vs numpy {err:.3e}")
        assert err <= REL, (name, err)
        assert not np.array_equal(got, got32.cpu().numpy())                     # the float64 digits were read
        R.close()


# ---------------------------------------------------------------------------------------------- 4: fields out
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nx,ny", MESHES)
def test_fields_device_and_round_trip(fine, coarse, torch, nx, ny, kind):
    pbs = _problems(fine, coarse, kind, nx, ny)
    a = fine.FineSolverBatch(pbs)
    a.init_from_fields(_fields(nx, ny, 5, seed=3))          # five different fields, so that a case in the wrong place shows
    a.run(5)
    var_a = a.Var
    host = np.stack([a.fields(i)[c] for i in range(5) for c in "uvp"])
    assert host.shape == (15, ny, nx)
    all64 = a.fields_device()
    assert all64.dtype == torch.float64 and tuple(all64.shape) == (15, ny, nx) and all64.is_cuda
    _same(all64.cpu().numpy(), host)
    _same(a.fields_device(dtype=torch.float32).cpu().numpy(), host.astype(np.float32))
    pick = [3 * c + k for c in CASES for k in range(3)]
    sub = a.fields_device(cases=CASES)
    _same(sub.cpu().numpy(), host[pick])
    _same(a.fields_device(cases=CASES, dtype=torch.float32).cpu().numpy(), host[pick].astype(np.float32))
    _same(a.Var, var_a)                                     # reading changes nothing
    # round trip: B from A's device fields is A', the batch given A's host Var through init
    bb = fine.FineSolverBatch(pbs)
    bb.init_from_fields(all64)
    _check_against_host_init(fine, pbs, bb, var_a, iterations=2)
    bb.close()
    a.close()


# ---------------------------------------------------------------------------------------------- 5: buffers and streams
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_guard_bands_and_offset_views(fine, coarse, torch, dtype):
    nx, ny = 37, 29
    tdtype, ndtype = getattr(torch, dtype), np.dtype(dtype)
    pbs = _problems(fine, coarse, "ldc_quick", nx, ny)
    F = _fields(nx, ny).astype(ndtype)
    b = fine.FineSolverBatch(pbs)
    b.init_from_fields(torch.from_numpy(F).cuda(), cases=CASES)
    plain_var = b.Var
    plain_out = b.fields_device(cases=CASES, dtype=tdtype)
    R = fine.interpolation_resampler(10, 10, nx, ny)
    F10 = _fields(nx, ny, h=10, w=10).astype(ndtype)
    b.init_from_fields(torch.from_numpy(F10).cuda(), cases=CASES, resampler=R)
    plain_var10 = b.Var
    guard = 2 * nx * ny
    for skew in (0, 1, 3):
        what = f"{dtype} skew {skew}"
        # input: quiet NaNs on both sides of the fields; a read outside them that reaches the state makes it differ
        for src, resampler, want in ((F, None, plain_var), (F10, R, plain_var10)):
            big, view = gb.poisoned(torch, src, guard, skew=skew)
            before = big.clone()
            b.init_from_fields(view, cases=CASES, resampler=resampler)
            gb.assert_same_bits(b.Var, want, what + " init_from_fields")
            gb.assert_same_bits(big.view(torch.int64 if dtype == "float64" else torch.int32),
                                before.view(torch.int64 if dtype == "float64" else torch.int32), what + " input buffer")
        # output: sentinels in the payload and in both guards
        b.init_from_fields(torch.from_numpy(F).cuda(), cases=CASES)
        big, view = gb.guarded(torch, (6, ny, nx), tdtype, guard, skew=skew)
        assert b.fields_device(cases=CASES, dtype=tdtype, out=view) is view
        gb.assert_guards_intact(big, view, what=what + " fields_device")
        gb.assert_fully_written(view, what=what + " fields_device")
        gb.assert_same_bits(view, plain_out, what + " fields_device")
    R.close()
    b.close()


@pytest.fixture(scope="module")
def ctx(fine, torch):
    class Ctx:
        pass
    c = Ctx()
    c.delay = so.Delay(torch)
    c.S = torch.cuda.Stream()
    return c


def test_side_stream_input_and_output(fine, coarse, torch, rs, ctx):
    """The inputs reach their addresses behind a delay on a non-blocking side stream (tests/stream_order.py) and the calls are
    made at once, without a synchronise: a call that did not order itself behind the stream reads the decoy that sits there.
    These calls block until their work is done, so -- unlike the entries of tests/test_gpu_stream_order.py -- the stream has
    drained when they return; that they waited for it shows in their duration: a quarter of the delay is asked for, where the
    call on an idle stream takes well under a millisecond."""
    nx, ny = 37, 29
    pbs = _problems(fine, coarse, "ldc_quick", nx, ny)
    real, decoy = (torch.from_numpy(_fields(nx, ny, seed=s)).cuda() for s in (1, 2))
    real10, decoy10 = (torch.from_numpy(_fields(nx, ny, seed=s, h=10, w=10)).cuda() for s in (3, 4))
    R = fine.interpolation_resampler(10, 10, nx, ny)
    b = fine.FineSolverBatch(pbs)
    waited = 0.25 * so.DELAY_MS * 1e-3
    for x, x_real, x_decoy, resampler in ((torch.empty_like(real), real, decoy, None), (torch.empty_like(real10), real10, decoy10, R)):
        what = "init_from_fields" + (" through the resampler" if resampler is not None else "")
        b.init_from_fields(x_real, cases=CASES, resampler=resampler)
        want = b.Var
        b.init_from_fields(x_decoy, cases=CASES, resampler=resampler)
        assert not np.array_equal(b.Var, want)
        o = so.delayed_call(torch, ctx.delay, ctx.S, [so.Arrival(x, x_decoy, x_real)],
                            lambda: b.init_from_fields(x, cases=CASES, resampler=resampler, stream=ctx.S), [], label=what)
        print(f"[stream order] {what}: call took {o.enqueue_s * 1e3:.1f} ms of a {so.DELAY_MS:g} ms delay")
        assert o.enqueue_s >= waited, (what, o.enqueue_s)
        _same(b.Var, want)
    # fields out: `out` is still being written on the side stream (its stale contents arrive behind the delay) when the call is
    # made; the copy must land after that write, and the stream's own clone of `out` after the copy
    want = b.fields_device(cases=CASES)
    out = torch.empty_like(want)
    stale = torch.full_like(want, 7.0)
    o = so.delayed_call(torch, ctx.delay, ctx.S, [so.Arrival(out, torch.zeros_like(want), stale)],
                        lambda: b.fields_device(cases=CASES, out=out, stream=ctx.S), [out], label="fields_device")
    print(f"[stream order] fields_device: call took {o.enqueue_s * 1e3:.1f} ms of a {so.DELAY_MS:g} ms delay")
    assert o.enqueue_s >= waited, o.enqueue_s
    so.assert_bit_equal(o.clones[0], want, "fields_device on a side stream")
    # the float64 resampler enqueues on the stream it is given and does not synchronise
    x = torch.empty_like(real10)
    y = torch.empty((6, ny, nx), dtype=torch.float64, device="cuda")
    want = R.apply_device_f64(real10)
    o = so.delayed_call(torch, ctx.delay, ctx.S, [so.Arrival(x, decoy10, real10)], lambda: R.apply_device_f64(x, out=y, stream=ctx.S), [y],
                        stale=[(y, R.apply_device_f64(decoy10))], label="srcfd_resample_device_f64")
    so.assert_pending(o, "srcfd_resample_device_f64")
    so.assert_bit_equal(o.clones[0], want, "srcfd_resample_device_f64 on a side stream")
    R.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_leave_the_batch_usable(fine, coarse, torch, rs, L):
    nx, ny = 37, 29
    pbs = _problems(fine, coarse, "ldc_quick", nx, ny)
    b = fine.FineSolverBatch(pbs)
    F = torch.from_numpy(_fields(nx, ny)).cuda()
    b.init_from_fields(F, cases=CASES)
    b.run(1)
    before = b.Var
    out = torch.empty((6, ny, nx), dtype=torch.float64, device="cuda")
    p = lambda t: L.device_ptr(t, "t")
    R = fine.interpolation_resampler(10, 10, nx, ny)
    other = fine.interpolation_resampler(10, 10, ny, nx)          # ends at the transposed mesh
    init, get = "srcfd_fine_batch_init_from_fields_device", "srcfd_fine_batch_get_fields_device"

    def raw_init(batch=b._h, r=None, fields=p(F), dtype=L.F64, n_warm=2, cases=CASES):
        idx = None if cases is None else (C.c_int * len(cases))(*cases)
        L.check(getattr(L.lib, init)(batch, r, fields, dtype, n_warm, idx, None))

    def raw_get(batch=b._h, n=2, cases=CASES, dst=p(out), dtype=L.F64):
        idx = None if cases is None else (C.c_int * len(cases))(*cases)
        L.check(getattr(L.lib, get)(batch, n, idx, dst, dtype, None))

    for raw, entry, count in ((raw_init, init, "n_warm"), (raw_get, get, "n")):
        key = count
        for kw in (dict(batch=None), dict(fields=None) if raw is raw_init else dict(dst=None)):
            with pytest.raises(ValueError, match=entry + ": bad arguments"):
                raw(**kw)
        for dtype in (L.I32, L.BF16, -1):
            with pytest.raises(ValueError, match=entry + f": dtype {dtype} is neither SRCFD_F32 nor SRCFD_F64"):
                raw(dtype=dtype)
        for n, cases in ((0, [0]), (6, [0, 1, 2, 3, 4, 4]), (-1, [0])):
            with pytest.raises(ValueError, match=entry + f": {count} {n} is outside 1..5"):
                raw(**{key: n, "cases": cases})
        with pytest.raises(ValueError, match=entry + r": cases\[1\] = 5 is outside 0..4"):
            raw(cases=[0, 5])
        with pytest.raises(ValueError, match=entry + r": cases\[0\] = -1 is outside 0..4"):
            raw(**{key: 1, "cases": [-1]})
        with pytest.raises(ValueError, match=entry + ": case 3 is listed twice"):
            raw(cases=[3, 3])
    with pytest.raises(ValueError, match=get + ": n 2 without a case list is not the batch's 5"):
        raw_get(cases=None)
    with pytest.raises(ValueError, match=init + r": the resampler's output mesh \(29 x 37\) is not the batch's \(37 x 29\)"):
        raw_init(r=other._h)
    # a resampler on another device needs a second device to exist: the C check is the one line next to the mesh check, and the
    # Python side refuses it first (tests/test_fine_fields.py)
    # the same through the class, which names the argument before the library is reached
    for kw, text in ((dict(fields=F, cases=[0, 5]), init + r": cases\[1\] = 5 is outside 0..4"),
                     (dict(fields=F, cases=[3, 3]), "cases must not repeat a case"),
                     (dict(fields=F[:3], cases=CASES), r"first dimension must be 3 \* n_warm = 6"),
                     (dict(fields=F, cases=CASES, resampler=R), r"fields has shape \(6, 29, 37\), expected \(6, 10, 10\)"),
                     (dict(fields=F, cases=CASES, resampler=other), r"resampler ends at \(37, 29\), the mesh takes fields of \(29, 37\)"),
                     (dict(fields=F.cpu(), cases=CASES), "fields must be a CUDA tensor"),
                     (dict(fields=F.half(), cases=CASES), "fields has dtype torch.float16")):
        with pytest.raises(ValueError, match=text):
            b.init_from_fields(**kw)
    with pytest.raises(ValueError, match=get + r": cases\[0\] = 7 is outside 0..4"):
        b.fields_device(cases=[7])
    # a batch that was never initialised has no fields to give
    h = C.c_void_p()
    arr = (L.CoarseProblem * 5)(*pbs)
    L.check(L.lib.srcfd_fine_batch_create(arr, 5, 0, C.byref(h)))
    with pytest.raises(ValueError, match=get + ": call srcfd_fine_batch_init first"):
        raw_get(batch=h)
    L.lib.srcfd_fine_batch_destroy(h)
    # nothing was touched, and the batch goes on
    _same(b.Var, before)
    assert b.iterations.tolist() == [1] * 5
    assert b.run(1).tolist() == [2] * 5
    for r in (R, other):
        r.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 7: the three arms
def test_compare_warm_starts(srcfd, fine, coarse, enc_weights, tmp_path):
    """20 x 20, encoder_10 + decoder_20 (the trained encoder, the family's synthetic decoder), the multiBC statistics re-keyed for a
    20 x 20 output, 20 iterations per case: every arm has the bits of its own sweep function."""
    fam = importlib.import_module("sr-for-cfd_amd.family")
    dec = str(tmp_path / "vanilla_decoder20_from_10_synthetic.h5")
    srcfd.SRModel.from_weights(None, fam.synthetic_decoder_weights(20), device=-1).save_h5(None, dec)
    stats = str(tmp_path / "standardization_stats_10to20.txt")
    srcfd.save_stats(stats, 10, 20, *srcfd.load_stats(STATS_TXT, 10, 400))
    files = dict(stats_file=stats, encoder_file=ENCODER_H5, decoder_file=dec)
    cfs = [srcfd.read_coarse_fields(os.path.join(GOLDEN, n)) for n in ("coarse_ldc_Re800_double_lid.h5", "coarse_ldc_Re1000_single_lid.h5")]
    res, bcs = [800.0, 1000.0], [coarse.LDC_DOUBLE_LID, coarse.LDC_SINGLE_LID]
    kw = dict(max_iterations_fine=20, bc=bcs)
    got = fine.compare_warm_starts(cfs, res, 20, 20, output_name=str(tmp_path / "arms"), **kw, **files)
    want = {"zero": fine.run_normal_simulations(res, 20, 20, max_iterations=20, bc=bcs),
            "interp": fine.run_interpolated_fine_simulations(cfs, res, 20, 20, **kw),
            "ml": fine.run_ml_accelerated_fine_simulations(cfs, res, 20, 20, **kw, **files)}      # two warm fields, as in the batch above
    assert [r["Re"] for r in got] == res
    for i, r in enumerate(got):
        assert set(r) == {"Re", "ml", "interp", "zero", "iterations_saved"}
        for arm in ("ml", "interp", "zero"):
            fields, it, st = want[arm][i]
            print(f"Re {res[i]:g} {arm}: {it} iterations, status {st}")
            assert (r[arm]["iterations"], r[arm]["status"]) == (it, st), (i, arm)
            for c in "uvp":
                assert r[arm]["fields"][c].shape == (20, 20)
                _same(r[arm]["fields"][c], fields[c])
        assert r["zero"]["iterations"] == 20 and r["zero"]["status"] == RUNNING
        assert r["iterations_saved"] == {arm: 20 - want[arm][i][1] for arm in ("ml", "interp")}
        assert not np.array_equal(r["ml"]["fields"]["u"], r["interp"]["fields"]["u"])
        assert not np.array_equal(r["interp"]["fields"]["u"], r["zero"]["fields"]["u"])
    back = srcfd.read_coarse_fields(str(tmp_path / "arms_Re1000_interp.h5"))
    np.testing.assert_array_equal(back["v"], got[1]["interp"]["fields"]["v"])
    # without model files the "ml" arm is left out; the arms that remain keep their bits, in the order asked for
    two = fine.compare_warm_starts(cfs, res, 20, 20, arms=("zero", "interp"), **kw)
    dflt = fine.compare_warm_starts(cfs, res, 20, 20, **kw)
    for i in range(2):
        assert set(two[i]) == set(dflt[i]) == {"Re", "interp", "zero", "iterations_saved"}
        for arm in ("interp", "zero"):
            for c in "uvp":
                _same(two[i][arm]["fields"][c], got[i][arm]["fields"][c])
                _same(dflt[i][arm]["fields"][c], got[i][arm]["fields"][c])
    # max_batch is rounded down to a multiple of the number of arms: 3 -> one Reynolds number per batch, the interp arm unchanged
    one = fine.compare_warm_starts(cfs, res, 20, 20, arms=("interp", "zero"), max_batch=3, **kw)
    for i in range(2):
        _same(one[i]["interp"]["fields"]["p"], got[i]["interp"]["fields"]["p"])
    # the two-arm function is what it was: its halves are the ML sweep and the normal sweep
    pair = fine.compare_ml_and_normal_simulations(cfs, res, 20, 20, **kw, **files)
    for i, r in enumerate(pair):
        assert (r["ml_iterations"], r["ml_status"]) == want["ml"][i][1:] and (r["normal_iterations"], r["normal_status"]) == want["zero"][i][1:]
        for c in "uvp":
            _same(r["ml_fields"][c], want["ml"][i][0][c])
            _same(r["normal_fields"][c], want["zero"][i][0][c])


def test_compare_bfs_warm_starts_without_a_model(srcfd, fine, coarse_cases):
    cfs, res = [coarse_cases["bfs_Re400"]] * 2, [400.0, 300.0]
    got = fine.compare_bfs_warm_starts(cfs, res, 20, 20, arms=("interp", "zero"), max_iterations_fine=10)
    interp = fine.run_bfs_interpolated_fine_simulations(cfs, res, 20, 20, max_iterations_fine=10)
    zero = fine.run_bfs_normal_simulations(res, 20, 20, max_iterations=10)
    for i, r in enumerate(got):
        for arm, want in (("interp", interp), ("zero", zero)):
            assert (r[arm]["iterations"], r[arm]["status"]) == (want[i][1], want[i][2]) == (10, RUNNING)
            for c in "uvp":
                _same(r[arm]["fields"][c], want[i][0][c])


# ---------------------------------------------------------------------------------------------- 8: grid sequencing
def test_nested_simulations(fine, coarse, torch, L, monkeypatch):
    meshes, res, cap = [(12, 12), (24, 20)], [100.0, 400.0, 1000.0], 15
    bcs = [coarse.LDC_SINGLE_LID, coarse.LDC_DOUBLE_LID, coarse.LDC_SINGLE_LID]
    # the same chain by hand, with the host synchronisations of each step counted (counters()["host_syncs"])
    lo = fine.FineSolverBatch([fine.problem(Re, 12, 12, bc=bc) for Re, bc in zip(res, bcs)], cap)
    lo.solve()
    s0 = lo.counters()["host_syncs"]
    f_lo = lo.fields_device()
    assert lo.counters()["host_syncs"] == s0 + 1             # the wait for the copy on the device; get_state was not called
    hi = fine.FineSolverBatch([fine.problem(Re, 24, 20, bc=bc) for Re, bc in zip(res, bcs)], cap)
    cold = fine.FineSolverBatch([fine.problem(Re, 24, 20, bc=bc) for Re, bc in zip(res, bcs)], cap)
    s_hi, s_cold = hi.counters()["host_syncs"], cold.counters()["host_syncs"]
    cold.init()
    up = fine.interpolation_resampler(12, 12, 24, 20)
    hi.init_from_fields(f_lo, resampler=up)
    assert hi.counters()["host_syncs"] - s_hi == cold.counters()["host_syncs"] - s_cold == 1     # what a start from zero costs
    hi.solve()
    want = [hi.fields(i) for i in range(3)]
    want_it = [[int(a), int(b)] for a, b in zip(lo.iterations, hi.iterations)]
    want_st = [[int(a), int(b)] for a, b in zip(lo.status, hi.status)]
    cold.solve()
    assert not np.array_equal(hi.Var, cold.Var)              # the coarse level reached the fine one
    for h in (lo, hi, cold, up):
        h.close()
    # the function: the same bits, and the only states copied to the host are the last level's results
    calls = []
    real = L.lib.srcfd_fine_batch_get_state

    def counted(handle, case, dst):
        calls.append(case)
        return real(handle, case, dst)
    monkeypatch.setattr(L.lib, "srcfd_fine_batch_get_state", counted)
    got = fine.run_nested_simulations(res, meshes, max_iterations=cap, bc=bcs)
    monkeypatch.undo()
    assert calls == [0, 1, 2]
    for i, r in enumerate(got):
        assert r["Re"] == res[i] and r["iterations"] == want_it[i] == [cap, cap] and r["status"] == want_st[i]
        for c in "uvp":
            assert r["fields"][c].shape == (20, 24)
            _same(r["fields"][c], want[i][c])
    # one Reynolds number per batch, and a cap per level: a case's bits do not depend on its batch
    one = fine.run_nested_simulations(res, meshes, max_iterations=[cap, cap], bc=bcs, max_batch=1, resident="auto")
    for i in range(3):
        assert one[i]["iterations"] == [cap, cap]
        _same(one[i]["fields"]["u"], want[i]["u"])
