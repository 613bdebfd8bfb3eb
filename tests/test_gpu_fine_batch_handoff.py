"""The batched SR hand-off on an MI355X: srcfd_fine_batch_init_from_prediction (csrc/fine_solver.hip, handoff_kernel) writes the
super-resolved fields of any subset of a batch's cases straight into their device state.

The bit reference is never the new kernel: it is the host recipe on `model.predict` (with a resampler `model.predict_resampled`)
of the same 3 * n_warm-sample batch -- float64, transposed into the interior -- handed to `FineSolverBatch.init(Var)`, which
stages interiors and applies the same priming.  For one case the single-case `FineSolver.init_from_prediction` is a reference
too."""
import ctypes as C
import importlib
import os
import signal

import numpy as np
import pytest

from conftest import ENCODER_H5, GOLDEN, STATS_TXT, require_gpu

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, DIVERGED = 0, 1, 2
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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _neumann_side(coarse):
    """The single lid with an outflow-like right side: u and v Neumann there."""
    bc = {c: dict(coarse.LDC_SINGLE_LID[c]) for c in "uvp"}
    bc["u"]["right"] = ("neumann", 0.0)
    bc["v"]["right"] = ("neumann", 0.0)
    return bc


def _tiny_model(srcfd, in_shape, seed=5, out_channels=1, device=0):
    """ConvT 2x2 stride 2 swish to 4 channels, then a 3x3 same conv: (h, w, 1) -> (2h, 2w, out_channels), O(0.1) outputs."""
    rng = np.random.default_rng(seed)
    specs = [dict(kind="conv2d_transpose", name="up", k=2, stride=2, same=False, act="swish",
                  w=rng.normal(0, 0.5, (2, 2, 4, 1)), b=rng.normal(0, 0.1, 4)),
             dict(kind="conv2d", name="out", k=3, stride=1, same=True, act="linear",
                  w=rng.normal(0, 0.15, (3, 3, 4, out_channels)), b=rng.normal(0, 0.05, out_channels))]
    return srcfd.SRModel.from_layers(specs, in_shape, device=device)


def _tiny_inputs(in_shape, n_fields, seed=11):
    """Inputs and affine pairs that differ from sample to sample, so that a sample in the wrong place is a different field."""
    rng = np.random.default_rng(seed)
    n = 3 * n_fields
    x = rng.normal(0, 1, (n,) + tuple(in_shape)).astype(np.float32)
    ain = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(0.8, 1.2, n)], axis=1).astype(np.float32)
    aout = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(0.5, 1.5, n)], axis=1).astype(np.float32)
    return x, ain, aout


def _host_var(model, x, ain, aout, back=None):
    """The host recipe: (n_fields, 3, nx+2, ny+2) with Var[k, 1+i, 1+j] = field_k[j, i] in float64 and a zero ring."""
    if back is None:
        y = model.predict(x, in_affine=ain, out_affine=aout, nan_guard=True)[..., 0]
    else:
        y = model.predict_resampled(x, back, in_affine=ain, out_affine=aout, nan_guard=True)
    n, ny, nx = y.shape
    var = np.zeros((n // 3, 3, nx + 2, ny + 2))
    for s in range(n):
        var[s // 3, s % 3, 1:-1, 1:-1] = y[s].astype(np.float64).T
    return var


def _trace(b, n):
    """Per outer iteration: every case's iteration count, status, rms bits and sweep counts."""
    out = []
    for _ in range(n):
        it = b.run(1)
        out.append((it.tolist(), b.status.tolist(), _bits(b.rms).tolist(), b.counters()["last_sweeps"]))
    return out


def _check_against_reference_batch(fine, pbs, var_host, b, iterations=2):
    """`b` has just been primed by init_from_prediction: the same state, and then the same run, as a batch primed from the host."""
    ref = fine.FineSolverBatch(pbs)
    ref.init(var_host)
    got = b.Var
    _same(got, ref.Var)
    nx, ny = pbs[0].nx, pbs[0].ny
    corners = got[:, :, [0, 0, nx + 1, nx + 1], [0, ny + 1, 0, ny + 1]]
    assert (_bits(corners) == 0).all()
    assert b.iterations.tolist() == [0] * len(pbs) and b.status.tolist() == [RUNNING] * len(pbs)
    trace = _trace(b, iterations)
    assert trace == _trace(ref, iterations)
    _same(b.Var, ref.Var)
    ref.close()
    return got, trace


# ---------------------------------------------------------------------------------------------- 1: tiny, awkward meshes
def _three_problems(fine, coarse, nx, ny, lx=1.0, ly=1.0):
    return [fine.problem(Re, nx, ny, lx, ly, 0.001, "QUICK", None, bc) for Re, bc in
            ((100.0, coarse.LDC_SINGLE_LID), (400.0, coarse.LDC_DOUBLE_LID), (250.0, _neumann_side(coarse)))]


def test_float_path_34x40_one_full_and_one_partial_tile_per_axis(srcfd, fine, coarse):
    model = _tiny_model(srcfd, (17, 20, 1))
    assert model.output_shape == (34, 40, 1)
    x, ain, aout = _tiny_inputs((17, 20, 1), 3)
    pbs = _three_problems(fine, coarse, 40, 34)
    b = fine.FineSolverBatch(pbs)
    assert b.init_from_prediction(model, x, ain, aout) == 0
    var, _ = _check_against_reference_batch(fine, pbs, _host_var(model, x, ain, aout), b)
    assert var.shape == (3, 3, 42, 36)
    # the three cases hold three different fields, each with its own boundary values in the ring
    assert not np.array_equal(var[0], var[1]) and not np.array_equal(var[1], var[2])
    assert np.abs(var[:, :, 1:-1, 1:-1]).max() > 1e-2
    b.close()


def test_double_path_70x37_through_the_resampler(srcfd, fine, coarse, rs):
    model = _tiny_model(srcfd, (6, 6, 1))
    assert model.output_shape == (12, 12, 1)
    back = rs.square_to_rect_resampler(12, 70, 37, 10.0, 3.0, model.device)
    x, ain, aout = _tiny_inputs((6, 6, 1), 3)
    pbs = _three_problems(fine, coarse, 70, 37, 10.0, 3.0)
    b = fine.FineSolverBatch(pbs)
    assert b.init_from_prediction(model, x, ain, aout, resampler=back) == 0
    var, _ = _check_against_reference_batch(fine, pbs, _host_var(model, x, ain, aout, back), b)
    assert var.shape == (3, 3, 72, 39)
    b.close()


# ---------------------------------------------------------------------------------------------- 2: cases=
def test_cases_selects_the_warm_cases_and_the_others_start_from_zero(srcfd, fine, coarse):
    model = _tiny_model(srcfd, (17, 20, 1))
    x, ain, aout = _tiny_inputs((17, 20, 1), 2)
    pbs = _three_problems(fine, coarse, 40, 34) + [fine.problem(700.0, 40, 34, 1.0, 1.0, 0.001, "QUICK", None, coarse.LDC_DOUBLE_LID)]
    zero = fine.FineSolverBatch(pbs)
    zero_var = zero.Var
    zero.close()
    fields = _host_var(model, x, ain, aout)
    want = np.zeros((4, 3, 42, 36))
    want[2], want[0] = fields[0], fields[1]
    b = fine.FineSolverBatch(pbs)
    b.run(1)                                  # a state that is not the initial one: the call has to clear it
    assert b.init_from_prediction(model, x, ain, aout, cases=[2, 0]) == 0
    var, clean_trace = _check_against_reference_batch(fine, pbs, want, b)
    _same(var[[1, 3]], zero_var[[1, 3]])
    assert not np.array_equal(var[2], var[0])
    # the guard counts over the warm samples, and only those: a NaN in one warm input
    xn = x.copy()
    xn[4, 3, 5, 0] = np.nan
    _, n_bad = model.predict(xn, in_affine=ain, out_affine=aout, nan_guard=True, return_nonfinite=True)
    assert 0 < n_bad < 34 * 40
    assert b.init_from_prediction(model, xn, ain, aout, cases=[2, 0]) == n_bad
    wantn = np.zeros((4, 3, 42, 36))
    fn = _host_var(model, xn, ain, aout)
    wantn[2], wantn[0] = fn[0], fn[1]
    _same(b.Var, _primed(fine, pbs, wantn))
    # without the guard the NaN reaches case 0, which diverges in its first iteration; the others do not notice
    b.init_from_prediction(model, xn, ain, aout, nan_guard=False, cases=[2, 0])
    b.run(2)
    assert b.status.tolist() == [DIVERGED, RUNNING, RUNNING, RUNNING] and b.iterations.tolist() == [1, 2, 2, 2]
    # a second hand-off re-arms the diverged batch: the state it has just written and nothing else
    assert b.init_from_prediction(model, x, ain, aout, cases=[2, 0]) == 0
    _same(b.Var, var)
    assert b.iterations.tolist() == [0] * 4 and b.status.tolist() == [RUNNING] * 4
    assert _trace(b, 2) == clean_trace
    b.close()


def _primed(fine, pbs, var_host):
    ref = fine.FineSolverBatch(pbs)
    ref.init(var_host)
    var = ref.Var
    ref.close()
    return var


# ---------------------------------------------------------------------------------------------- 3: B = 1 is the single-case path
@pytest.mark.parametrize("resampled", [False, True])
def test_one_case_batch_equals_the_single_case_solver(srcfd, fine, coarse, rs, resampled):
    if resampled:
        model, in_shape, nx, ny, lx, ly = _tiny_model(srcfd, (6, 6, 1)), (6, 6, 1), 70, 37, 10.0, 3.0
        back = rs.square_to_rect_resampler(12, nx, ny, lx, ly, model.device)
        pb = fine.problem(300.0, nx, ny, lx, ly, 0.002, "UPWIND", None, None, bfs=_BFS)
    else:
        model, in_shape, nx, ny, back = _tiny_model(srcfd, (17, 20, 1)), (17, 20, 1), 40, 34, None
        pb = fine.problem(400.0, nx, ny, 1.0, 1.0, 0.001, "QUICK", None, coarse.LDC_DOUBLE_LID)
    x, ain, aout = _tiny_inputs(in_shape, 1)
    b = fine.FineSolverBatch([pb])
    s = fine.FineSolver(pb)
    assert b.init_from_prediction(model, x, ain, aout, resampler=back) == 0
    assert s.init_from_prediction(model, x, ain, aout, resampler=back) == 0
    _same(b.Var[0], s.Var)
    _check_against_reference_batch(fine, [pb], _host_var(model, x, ain, aout, back), b, iterations=0)
    for n in (1, 2):
        assert b.run(1).tolist() == [n] and s.run(1) == n
        _same(b.rms[0], s.rms)
        assert b.counters()["last_sweeps"][0] == s.counters()["last_sweeps"]
    _same(b.Var[0], s.Var)
    b.close()
    s.close()


# ---------------------------------------------------------------------------------------------- 4: at the workload's size, once
@pytest.fixture(scope="module")
def model(srcfd):
    require_gpu(srcfd)
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    enc_w = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
    return srcfd.SRModel.from_weights(enc_w, synth.synthetic_decoder_weights(1), device=0)


def _sr_inputs(srcfd, name):
    lr, hr = srcfd.load_stats(STATS_TXT, 10, 400)
    cf = srcfd.read_coarse_fields(os.path.join(GOLDEN, name))
    x = np.stack([cf[c].astype(np.float32) for c in "uvp"])[..., None]
    return x, np.array([lr[c] for c in "uvp"], np.float32), np.array([hr[c] for c in "uvp"], np.float32)


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _check_each_case_against_its_own_hand_off(fine, pbs, var, model, per_case, back=None):
    """Each case's interior within the project's f32 parity bar (1e-5 relative L2) of what the single-case hand-off writes for
    that case alone: both are f32-path predictions of the same inputs (each measured at 5.8e-7 from the float64 oracle), so the
    bar is met with a wide margin unless a case received another case's field or affine pair."""
    for i, (pb, (x, ain, aout)) in enumerate(zip(pbs, per_case)):
        s = fine.FineSolver(pb)
        s.init_from_prediction(model, x, ain, aout, resampler=back)
        solo = s.Var
        s.close()
        for k in range(3):
            err = _rel_l2(var[i, k, 1:-1, 1:-1], solo[k, 1:-1, 1:-1])
            print(f"case {i} plane {k}: rel L2 vs the single-case hand-off {err:.3e}")
            assert err <= 1e-5, (i, k, err)


def test_ldc_400x400_two_cases(srcfd, fine, coarse, model):
    per_case = [_sr_inputs(srcfd, "coarse_ldc_Re800_double_lid.h5"), _sr_inputs(srcfd, "coarse_ldc_Re1000_single_lid.h5")]
    x, ain, aout = (np.concatenate([pc[q] for pc in per_case]) for q in range(3))
    pbs = [fine.problem(800.0, 400, 400, bc=coarse.LDC_DOUBLE_LID), fine.problem(1000.0, 400, 400, bc=coarse.LDC_SINGLE_LID)]
    b = fine.FineSolverBatch(pbs)
    assert b.init_from_prediction(model, x, ain, aout) == 0
    var, _ = _check_against_reference_batch(fine, pbs, _host_var(model, x, ain, aout), b)
    b.close()
    _check_each_case_against_its_own_hand_off(fine, pbs, var, model, per_case)
    assert _rel_l2(var[0, 0, 1:-1, 1:-1], var[1, 0, 1:-1, 1:-1]) > 1e-3     # the two cases are told apart by that bar


def test_bfs_400x400_two_cases_through_the_resampler(srcfd, fine, rs, model):
    per_case = [_sr_inputs(srcfd, "coarse_bfs_Re400.h5")] * 2
    x, ain, aout = (np.concatenate([pc[q] for pc in per_case]) for q in range(3))
    back = rs.square_to_rect_resampler(400, 400, 400, 10.0, 3.0, model.device)
    pbs = [fine.problem(Re, 400, 400, 10.0, 3.0, 0.002, "UPWIND", None, None, bfs=_BFS) for Re in (400.0, 300.0)]
    b = fine.FineSolverBatch(pbs)
    assert b.init_from_prediction(model, x, ain, aout, resampler=back) == 0
    var, _ = _check_against_reference_batch(fine, pbs, _host_var(model, x, ain, aout, back), b)
    b.close()
    _check_each_case_against_its_own_hand_off(fine, pbs, var, model, per_case, back)


# ---------------------------------------------------------------------------------------------- 5: drop-ins
def test_sweep_drop_ins(srcfd, fine, coarse, dec_weights, tmp_path):
    kc = importlib.import_module("sr-for-cfd_amd.keras_compat")
    dec = str(tmp_path / "vanilla_decoder400_from_10_synthetic.h5")
    srcfd.SRModel.from_weights(None, dec_weights, device=-1).save_h5(None, dec)
    files = dict(stats_file=STATS_TXT, encoder_file=ENCODER_H5, decoder_file=dec)
    names = ("coarse_ldc_Re800_double_lid.h5", "coarse_ldc_Re1000_single_lid.h5")
    cfs = [srcfd.read_coarse_fields(os.path.join(GOLDEN, n)) for n in names]
    res, bcs = [800.0, 1000.0], [coarse.LDC_DOUBLE_LID, coarse.LDC_SINGLE_LID]
    got = fine.run_ml_accelerated_fine_simulations(cfs, res, 400, 400, max_iterations_fine=2, bc=bcs, output_name=str(tmp_path / "sweep"), **files)
    assert [(it, st) for _, it, st in got] == [(2, RUNNING)] * 2
    back = srcfd.read_coarse_fields(str(tmp_path / "sweep_Re1000_accelerated.h5"))
    np.testing.assert_array_equal(back["v"], got[1][0]["v"])
    # manual use of the class, with inputs stacked here
    handle = kc._device_handle((ENCODER_H5, dec), kc._DEFAULT_PRECISION)
    per_case = [_sr_inputs(srcfd, n) for n in names]
    x, ain, aout = (np.concatenate([pc[q] for pc in per_case]) for q in range(3))
    pbs = [fine.problem(Re, 400, 400, bc=bc) for Re, bc in zip(res, bcs)]
    b = fine.FineSolverBatch(pbs, 2, handle.device)
    b.init_from_prediction(handle, x, ain, aout)
    b.solve()
    for i in range(2):
        for c in "uvp":
            _same(got[i][0][c], b.fields(i)[c])
    assert b.iterations.tolist() == [2, 2]
    b.close()
    # one case per batch: the single-case drop-in, bit for bit
    one = fine.run_ml_accelerated_fine_simulations(cfs, res, 400, 400, max_iterations_fine=2, bc=bcs, max_batch=1, **files)
    for i in range(2):
        s, it, _ = fine.run_ml_accelerated_fine_simulation(cfs[i], res[i], 400, 400, max_iterations_fine=2, bc=bcs[i],
                                                           output_name=str(tmp_path / f"single{i}"), **files)
        assert (one[i][1], one[i][2]) == (it, RUNNING)
        for c in "uvp":
            _same(one[i][0][c], s.fields()[c])
        s.close()
    # the comparison: the warm half is the sweep above cut at one Reynolds number per pair, the cold half the normal sweep
    cmp_ = fine.compare_ml_and_normal_simulations(cfs, res, 400, 400, max_iterations_fine=2, bc=bcs, **files)
    cold = fine.run_normal_simulations(res, 400, 400, max_iterations=2, bc=bcs)
    assert [r["Re"] for r in cmp_] == res
    for r, (f_cold, it, st) in zip(cmp_, cold):
        assert (r["normal_iterations"], r["normal_status"]) == (it, st) == (2, RUNNING)
        assert (r["ml_iterations"], r["ml_status"]) == (2, RUNNING) and r["ratio"] == 1.0 and r["iterations_saved"] == 0
        for c in "uvp":
            _same(r["normal_fields"][c], f_cold[c])
        assert not np.array_equal(r["ml_fields"]["u"], r["normal_fields"]["u"])


# ---------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_leave_the_batch_usable(srcfd, fine, coarse, rs):
    L = importlib.import_module("sr-for-cfd_amd._lib")
    entry = "srcfd_fine_batch_init_from_prediction"
    model = _tiny_model(srcfd, (17, 20, 1))
    x, ain, aout = _tiny_inputs((17, 20, 1), 3)
    pbs = _three_problems(fine, coarse, 40, 34)
    b = fine.FineSolverBatch(pbs)
    b.init_from_prediction(model, x, ain, aout)
    before = b.Var
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = C.c_int64(0)

    def raw(batch=b._h, m=model._h, r=None, xs=ptr(x), n_warm=3, cases=None):
        idx = None if cases is None else (C.c_int * len(cases))(*cases)
        L.check(getattr(L.lib, entry)(batch, m, r, xs, n_warm, idx, ptr(ain), ptr(aout), 0, C.byref(bad)))

    # 1: null handle, model or x
    for kw in (dict(batch=None), dict(m=None), dict(xs=None)):
        with pytest.raises(ValueError, match=entry + ": bad arguments"):
            raw(**kw)
    # 2: n_warm outside 1..n_cases
    for n_warm, cases in ((0, [0]), (4, [0, 1, 2, 2]), (-1, [0])):
        with pytest.raises(ValueError, match=entry + f": n_warm {n_warm} is outside 1..3"):
            raw(n_warm=n_warm, cases=cases)
    with pytest.raises(ValueError, match=entry + ": n_warm 2 without a case list"):
        raw(n_warm=2)
    # 3: a case index out of range, or repeated
    with pytest.raises(ValueError, match=entry + r": cases\[1\] = 3 is outside 0..2"):
        b.init_from_prediction(model, x[:6], ain[:6], aout[:6], cases=[0, 3])
    with pytest.raises(ValueError, match=entry + r": cases\[0\] = -1 is outside 0..2"):
        raw(n_warm=1, cases=[-1])
    with pytest.raises(ValueError, match=entry + ": case 1 is listed twice"):
        raw(n_warm=2, cases=[1, 1])
    # 4: model and batch on different devices (a host-only model handle has none)
    host_model = _tiny_model(srcfd, (17, 20, 1), device=-1)
    with pytest.raises(ValueError, match=entry + ": model and batch are on different devices"):
        b.init_from_prediction(host_model, x, ain, aout)
    # 5: a prediction mesh that is not the batch's
    other = _tiny_model(srcfd, (20, 17, 1))
    with pytest.raises(ValueError, match=entry + r": the prediction's mesh \(34 x 40\) is not the batch's \(40 x 34\)"):
        b.init_from_prediction(other, x.reshape(9, 20, 17, 1), ain, aout)
    # 6: a multi-channel model
    two = _tiny_model(srcfd, (17, 20, 1), out_channels=2)
    with pytest.raises(ValueError, match=entry + ": single-channel models only"):
        b.init_from_prediction(two, x, ain, aout)
    # 7: a resampler that does not match the model
    wrong = rs.square_to_rect_resampler(12, 40, 34, 1.0, 1.0, model.device)
    with pytest.raises(ValueError, match=entry + ": resampler does not match the model"):
        b.init_from_prediction(model, x, ain, aout, resampler=wrong)
    # the class's own shape checks, before any device call
    for args, kw, text in (((x[:6], ain, aout), {}, r"x must have shape \(9, lr, lr, 1\)"),
                           ((x.reshape(9, 20, 17, 1), ain, aout), {}, r"x must have shape \(9, lr, lr, 1\)"),
                           ((x, ain[:6], aout), {}, r"in_affine must have shape \(9, 2\)"),
                           ((x, ain, aout.reshape(2, 9)), {}, r"out_affine must have shape \(9, 2\)"),
                           ((x, ain, aout), dict(cases=[0, 1, 2, 0]), "between 1 and 3 cases"),
                           ((x, ain, aout), dict(cases=[]), "between 1 and 3 cases"),
                           ((x[:6], ain[:6], aout[:6]), dict(cases=[1, 1]), "must not repeat a case")):
        with pytest.raises(ValueError, match=text):
            b.init_from_prediction(model, *args, **kw)
    # nothing was touched, and the batch goes on
    _same(b.Var, before)
    assert b.iterations.tolist() == [0, 0, 0]
    assert b.run(1).tolist() == [1, 1, 1]
    b.close()
