"""The resident mode of the fine-mesh solver (csrc/fine_solver.hip resident_kernel, fine.FineSolverBatch(resident=True)) on an
MI355X: one workgroup per case runs up to 100 outer iterations per launch.  Every case has the bits of the numpy specification
(tests/fine_solver_spec.py) -- and so of the launch-per-sweep mode -- whatever the mesh, the batch, its place in it and the chunking
of the run; every test also reads from counters() that the resident path ran: one launch and one host synchronisation per chunk
of at most 100 outer iterations, not per sweep."""
import importlib
import signal

import numpy as np
import pytest

from conftest import require_gpu
import fine_solver_spec as spec

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, DIVERGED = 0, 1, 2
CAP = spec.CAP
MAX = 64                                   # srcfd_fine_resident_supported's bound
_BFS = {"step_height": 1.0, "h": 2.0, "Ub": 1.0}
_LOOSE = {"u": 1e-2, "v": 1e-2, "p": 1e-2}


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _smooth_state(nx, ny, seed):
    """A seeded, smooth, non-zero state; u changes sign along the right boundary (backflow at a BFS outlet)."""
    rng = np.random.default_rng(seed)
    x = (np.arange(1, nx + 1) - 0.5) / nx
    y = (np.arange(1, ny + 1) - 0.5) / ny
    X, Y = np.meshgrid(x, y, indexing="ij")
    var = np.zeros((3, nx + 2, ny + 2))
    for k in range(3):
        a, b, c = rng.uniform(0.5, 1.5, 3)
        ph = rng.uniform(0, np.pi, 2)
        var[k, 1:-1, 1:-1] = 0.3 * a * np.sin(np.pi * (b * X) + ph[0]) * np.cos(np.pi * (c * Y) + ph[1]) + 0.05 * k
    return var


def _chunks(start, n, end=None):
    """Resident launches of run(n) from the common iteration count `start`: chunks end at the next multiple of 100 or with the
    budget; `end`: the iteration at which the last live case freezes, after which nothing is launched."""
    count, left, chunks = start, n, 0
    while left > 0 and (end is None or count < end):
        step = min(left, 100 - count % 100)
        count, left, chunks = count + step, left - step, chunks + 1
    return chunks


class _Counted:
    """Asserts on exit that the solver or batch enqueued exactly `chunks` operations with as many host synchronisations."""

    def __init__(self, s, chunks):
        self.s, self.chunks = s, chunks

    def __enter__(self):
        self.c0 = self.s.counters()
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            c1 = self.s.counters()
            assert (c1["launches"] - self.c0["launches"], c1["host_syncs"] - self.c0["host_syncs"]) == (self.chunks, self.chunks)
        return False


def _history(b, i):
    return np.array([b.residual_history[i][c] for c in "uvp"]).T.reshape(-1, 3)


# ---------------------------------------------------------------------------------------------- 1: every case at its own pace
def _staggered_problems(fine, coarse):
    """The first three of test_gpu_fine_batch's: 12x10, QUICK, dt 0.01, tolerances 1e-2, from zero; alone, the spec converges at
    211, 326 and 315."""
    return [fine.problem(Re, 12, 10, 1.0, 1.0, 0.01, "QUICK", _LOOSE, bc) for Re, bc in
            ((50.0, coarse.LDC_SINGLE_LID), (100.0, coarse.LDC_DOUBLE_LID), (100.0, coarse.LDC_SINGLE_LID))]


def test_cases_run_at_their_own_pace_with_the_specification_bits(fine, coarse):
    pbs = _staggered_problems(fine, coarse)
    snaps = []
    for pb in pbs:
        sp = spec.from_problem(pb)
        sp.init()
        snap = {}
        for stop in (250, 100000):
            sp.run(stop - sp.count)
            snap[sp.count] = (sp.Var.copy(), sp.rms.copy(), list(sp.sweeps[-1]), np.array(sp.history).reshape(-1, 3))
        snaps.append(snap)
    assert [max(s) for s in snaps] == [211, 326, 315]
    b = fine.FineSolverBatch(pbs, resident=True)

    def check(at):
        assert b.iterations.tolist() == at
        for i, n in enumerate(at):
            var, rms, sweeps, hist = snaps[i][n]
            _same(b.case_var(i), var)
            _same(b.rms[i], rms)
            assert b.counters()["last_sweeps"][i] == sweeps
            _same(_history(b, i), hist)
            assert len(hist) == n // 100

    with _Counted(b, 3):                      # 100, 200, 250
        assert b.run(250).tolist() == [211, 250, 250]
    assert b.status.tolist() == [CONVERGED, RUNNING, RUNNING]
    check([211, 250, 250])
    with _Counted(b, 2):                      # 300, 400: both live cases converge inside the second chunk
        assert b.run(1000).tolist() == [211, 326, 315]
    assert b.status.tolist() == [CONVERGED] * 3
    check([211, 326, 315])
    with _Counted(b, 0):                      # nothing is running
        b.run(10)
    b.close()


# ---------------------------------------------------------------------------------------------- 2: kernel edges
def _ldc(Re, nx, ny, scheme, dt=0.001):
    return lambda f, c: [f.problem(Re, nx, ny, 1.0, 1.0, dt, scheme, None, c.LDC_DOUBLE_LID),
                         f.problem(2.5 * Re, nx, ny, 1.0, 1.0, dt, scheme, None, c.LDC_SINGLE_LID)]


EDGES = {
    # the far reads of QUICK wrap and run on at every cell
    "3x3_quick": (_ldc(100.0, 3, 3, "QUICK"), 12),
    "3x5_upwind": (_ldc(100.0, 3, 5, "UPWIND"), 12),
    "5x3_upwind": (_ldc(100.0, 5, 3, "UPWIND"), 12),
    # the colour origins of odd and even rows, a row of 16 or 17 cells: the row tree crosses 16, 8 or 9 cells of one colour
    "17x16_quick": (_ldc(100.0, 17, 16, "QUICK"), 6),
    "16x17_quick": (_ldc(100.0, 16, 17, "QUICK"), 6),
    # the row tree crosses 32 (33 cells of a column of rows, 31 per row), 17 rows per colour origin
    "33x31_quick": (_ldc(100.0, 33, 31, "QUICK"), 5),
    "31x33_upwind": (_ldc(100.0, 31, 33, "UPWIND"), 5),
    # the largest supported mesh: a full wave per row, the most row partials, all of the LDS planes; from zero fields the pressure
    # solve stops by its rule at 567, 763, 895 and 988 sweeps
    "largest_square_from_zero": (lambda f, c: [f.problem(100.0, MAX, MAX, 1.0, 1.0, 0.01, "QUICK", None, c.LDC_DOUBLE_LID)], 4),
    # 64x64 QUICK Re 100 at dt 0.01 for 12 iterations from the smooth state: with this seeded state every pressure solve of the
    # spec runs into the cap (from fields close to the solution it takes 960-980 sweeps), so the case above is the one whose
    # long pressure solves end by the rule
    "largest_square": (lambda f, c: [f.problem(100.0, MAX, MAX, 1.0, 1.0, 0.01, "QUICK", None, c.LDC_DOUBLE_LID)], 12),
    "largest_x3": (_ldc(100.0, MAX, 3, "QUICK"), 4),
    "3xlargest": (_ldc(100.0, 3, MAX, "UPWIND"), 4),
    # the BFS inlet, outlet backflow, under-relaxation with per-case factors; the pressure solve hits the cap
    "bfs_upwind": (lambda f, c: [f.problem(Re, 37, 29, 10.0, 3.0, 0.002, "UPWIND", None, None, bfs=_BFS, relaxation_factors=rf)
                                 for Re, rf in ((200.0, {"u": 0.5, "v": 0.5, "p": 0.2}), (400.0, {"u": 0.7, "v": 0.6, "p": 0.3}))], 3),
    "bfs_quick": (lambda f, c: [f.problem(300.0, 21, 18, 10.0, 3.0, 0.002, "QUICK", None, None, bfs=_BFS)], 4),
}


@pytest.mark.parametrize("case", list(EDGES))
def test_edges_equal_the_specification(fine, coarse, case):
    make, iterations = EDGES[case]
    pbs = make(fine, coarse)
    starts = np.stack([_smooth_state(pb.nx, pb.ny, seed=7 + i) * (not case.endswith("_from_zero")) for i, pb in enumerate(pbs)])
    b = fine.FineSolverBatch(pbs, resident=True)
    b.init(starts)
    with _Counted(b, 1):
        assert b.run(iterations).tolist() == [iterations] * len(pbs)
    assert b.status.tolist() == [RUNNING] * len(pbs)
    var, sweeps = b.Var, b.counters()["last_sweeps"]
    for i, pb in enumerate(pbs):
        sp = spec.from_problem(pb)
        sp.init(starts[i])
        sp.run(iterations)
        assert sweeps[i] == sp.sweeps[-1], (case, i)
        _same(b.rms[i], sp.rms)
        _same(var[i], sp.Var)
        if case.startswith("bfs_upwind"):
            assert sp.sweeps[-1][2] == CAP
        if case == "largest_square":
            assert all(12 <= sw[0] <= 14 and sw[2] == CAP for sw in sp.sweeps)
        if case == "largest_square_from_zero":
            assert (pb.nx, pb.ny) == (64, 64) and [s[2] for s in sp.sweeps] == [567, 763, 895, 988]
    b.close()


# ---------------------------------------------------------------------------------------------- 3: divergence inside one launch
def test_a_case_that_diverges_inside_a_launch_is_frozen_there(fine, coarse):
    """20x15 UPWIND Re 100 double lid from zero, dt 0.05 and 0.1: alone, dt 0.1 runs all three solves into the cap in iteration 3
    and is non-finite at iteration 4; dt 0.05 stays finite, with 9 to 19 sweeps per u solve.  (The
    issue that asked for this test expected 33-35 momentum sweeps there; the specification, which is the yardstick, takes 9, 9, 9,
    12, 15 and 19, and the test asserts what the specification does.)"""
    pbs = [fine.problem(100.0, 20, 15, 1.0, 1.0, dt, "UPWIND", None, coarse.LDC_DOUBLE_LID) for dt in (0.05, 0.1)]
    ok, bad = (spec.from_problem(pb) for pb in pbs)
    ok.init()
    ok.run(6)
    bad.init()
    bad.run(3)
    assert bad.sweeps == [[13, 1, 98], [51, 35, 191], [CAP] * 3]
    with pytest.raises(ValueError, match="NaN/Inf"), np.errstate(over="ignore", invalid="ignore"):
        bad.run(1)
    assert np.isfinite(ok.rms).all() and [s[0] for s in ok.sweeps] == [9, 9, 9, 12, 15, 19]
    b = fine.FineSolverBatch(pbs, resident=True)
    with _Counted(b, 1):
        assert b.run(6).tolist() == [6, 4]
    assert b.status.tolist() == [RUNNING, DIVERGED]
    assert not np.isfinite(b.rms[1]).all()
    _same(b.case_var(0), ok.Var)
    _same(b.rms[0], ok.rms)
    assert b.counters()["last_sweeps"][0] == ok.sweeps[-1]
    with _Counted(b, 1):                      # the frozen case's workgroup returns at once
        assert b.run(1).tolist() == [7, 4]
    b.init()                                  # revives both
    assert b.status.tolist() == [RUNNING] * 2
    with _Counted(b, 1):
        assert b.run(1).tolist() == [1, 1]
    assert b.counters()["last_sweeps"] == [ok.sweeps[0], bad.sweeps[0]]
    b.close()
    # a single solver raises the reference's error and has to be initialised again
    s = fine.FineSolver(pbs[1], resident=True)
    with pytest.raises(ValueError, match="NaN/Inf"):
        s.run(6)
    with pytest.raises(ValueError, match="init first"):
        s.run(1)
    s.init()
    with _Counted(s, 1):
        assert s.run(3) == 3
    assert s.counters()["last_sweeps"] == [CAP] * 3
    s.close()


# ---------------------------------------------------------------------------------------------- 4, 5: chunks, resume, mode switch
def _pb_320(fine, coarse):
    """10x10 Re 100 single lid, dt 0.01, tolerances 1e-2: the spec converges at 320."""
    return fine.problem(100.0, 10, 10, 1.0, 1.0, 0.01, "QUICK", _LOOSE, coarse.LDC_SINGLE_LID)


@pytest.fixture(scope="module")
def spec_320(fine, coarse):
    sp = spec.from_problem(_pb_320(fine, coarse))
    sp.init()
    snap = {}
    for stop in (300, 100000):
        sp.run(stop - sp.count)
        snap[sp.count] = (sp.Var.copy(), sp.rms.copy(), list(sp.sweeps[-1]))
    assert sp.converged and sp.count == 320 and len(sp.history) == 3
    return sp, snap


def test_chunked_and_resumed_runs_equal_one_run(fine, coarse, spec_320):
    sp, snap = spec_320
    var, rms, sweeps = snap[320]
    a = fine.FineSolver(_pb_320(fine, coarse), resident=True)
    for n, at, chunks in ((99, 99, 1), (2, 101, 2), (400, 320, 3)):
        with _Counted(a, chunks):
            assert a.run(n) == at
    b = fine.FineSolverBatch([_pb_320(fine, coarse)], resident=True)
    with _Counted(b, 4):
        assert b.run(1000).tolist() == [320]
    assert b.status.tolist() == [CONVERGED]
    for got_var, got_rms, got_sweeps, hist in ((a.Var, a.rms, a.counters()["last_sweeps"], np.array([a.residual_history[c] for c in "uvp"]).T),
                                               (b.case_var(0), b.rms[0], b.counters()["last_sweeps"][0], _history(b, 0))):
        _same(got_var, var)
        _same(got_rms, rms)
        assert got_sweeps == sweeps
        assert hist.shape == (3, 3)
        _same(hist, np.array(sp.history))
    a.close()
    b.close()


@pytest.mark.parametrize("first", ["launches", "resident"])
def test_the_mode_may_change_between_two_runs(fine, coarse, spec_320, first):
    var, rms, sweeps = spec_320[1][300]
    s = fine.FineSolver(_pb_320(fine, coarse), resident=first == "resident")
    for resident in (first == "resident", first != "resident"):
        assert s.set_resident(resident) == resident
        c0 = s.counters()
        s.run(150)
        c1 = s.counters()
        grown = (c1["launches"] - c0["launches"], c1["host_syncs"] - c0["host_syncs"])
        if resident:
            assert grown == (2, 2)             # 0 -> 100 -> 150, or 150 -> 200 -> 300
        else:
            assert grown[0] > 150 * 20 and grown[1] >= 150 * 4
    assert s.iterations == 300
    _same(s.Var, var)
    _same(s.rms, rms)
    assert s.counters()["last_sweeps"] == sweeps
    assert len(s.residual_history["u"]) == 3   # 100, 200, 300
    s.close()


# ---------------------------------------------------------------------------------------------- 6: batch size and place
def test_bits_do_not_depend_on_the_batch_or_the_place_in_it(fine, coarse):
    me = fine.problem(100.0, 12, 10, 1.0, 1.0, 0.01, "QUICK", _LOOSE, coarse.LDC_DOUBLE_LID)
    others = [fine.problem(40.0 + 13.0 * i, 12, 10, 1.0, 1.0, 0.002 * (1 + i % 5), "QUICK", _LOOSE,
                           coarse.LDC_SINGLE_LID if i % 2 else coarse.LDC_DOUBLE_LID) for i in range(62)]
    solo = fine.FineSolver(me, resident=True)
    with _Counted(solo, 1):
        solo.run(30)
    b = fine.FineSolverBatch([me] + others + [me], resident=True)
    assert b.n_cases == 64
    with _Counted(b, 1):
        b.run(30)
    sweeps = b.counters()["last_sweeps"]
    for at in (0, 63):
        _same(b.case_var(at), solo.Var)
        _same(b.rms[at], solo.rms)
        assert sweeps[at] == solo.counters()["last_sweeps"]
    assert len({tuple(_bits(r).tolist()) for r in b.rms}) == 63
    solo.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 7: a long run, mode against mode
def test_three_thousand_iterations_equal_the_launch_mode(fine, coarse):
    pb = fine.problem(800.0, 10, 10, 1.0, 1.0, 0.001, "QUICK", None, coarse.LDC_DOUBLE_LID)
    got = {}
    for resident in (False, True):
        s = fine.FineSolver(pb, resident=resident)
        c0 = s.counters()
        assert s.run(3000) == 3000
        c1 = s.counters()
        got[resident] = (s.Var, s.rms, c1["last_sweeps"], [s.residual_history[c] for c in "uvp"],
                         (c1["launches"] - c0["launches"], c1["host_syncs"] - c0["host_syncs"]))
        s.close()
    assert got[True][4] == (30, 30) and got[False][4][0] > 3000 * 20
    _same(got[True][0], got[False][0])
    _same(got[True][1], got[False][1])
    assert got[True][2] == got[False][2]
    _same(np.array(got[True][3]), np.array(got[False][3]))
    assert len(got[True][3][0]) == 30


# ---------------------------------------------------------------------------------------------- 8: warm start
def test_warm_started_batches_agree_between_the_modes(srcfd, fine, coarse):
    """encoder_10 + decoder_50 at Keras' initial weights: one prediction into a two-case 50x50 batch in each mode."""
    from test_gpu_fine_batch_handoff import _host_var, _tiny_inputs
    family = importlib.import_module("sr-for-cfd_amd.family")
    enc, dec = family.keras_default_init(10, 50, seed=0)
    model = srcfd.SRModel.from_weights(enc, dec, device=0)
    assert model.output_shape == (50, 50, 1)
    x, ain, aout = _tiny_inputs((10, 10, 1), 2)
    pbs = [fine.problem(Re, 50, 50, 1.0, 1.0, 0.001, "QUICK", None, bc) for Re, bc in ((100.0, coarse.LDC_SINGLE_LID), (400.0, coarse.LDC_DOUBLE_LID))]
    host = fine.FineSolverBatch(pbs)
    host.init(_host_var(model, x, ain, aout))
    got = {}
    for resident in (False, True):
        b = fine.FineSolverBatch(pbs, resident=resident)
        assert b.init_from_prediction(model, x, ain, aout) == 0
        _same(b.Var, host.Var)
        c0 = b.counters()
        assert b.run(3).tolist() == [3, 3]
        c1 = b.counters()
        got[resident] = (b.Var, b.rms, c1["last_sweeps"], (c1["launches"] - c0["launches"], c1["host_syncs"] - c0["host_syncs"]))
        b.close()
    host.close()
    assert got[True][3] == (1, 1) and got[False][3][0] > 100
    _same(got[True][0], got[False][0])
    _same(got[True][1], got[False][1])
    assert got[True][2] == got[False][2]


# ---------------------------------------------------------------------------------------------- 9: drop-ins
def test_drop_ins_return_what_the_launch_mode_returns(fine, coarse, tmp_path):
    kw = dict(dt=0.01, convergence_criteria=_LOOSE, bc=coarse.LDC_DOUBLE_LID)
    a = fine.run_normal_simulations([100, 50, 150], 12, 10, max_batch=2, resident=True, **kw)
    b = fine.run_normal_simulations([100, 50, 150], 12, 10, max_batch=2, resident=False, **kw)
    assert [(it, st) for _, it, st in a] == [(it, st) for _, it, st in b] and all(st == CONVERGED for _, _, st in a)
    for (fa, _, _), (fb, _, _) in zip(a, b):
        for c in "uvp":
            _same(fa[c], fb[c])
    # the coarse sweep is a resident batch of its Reynolds numbers
    res = [100.0, 400.0, 250.0]
    fields = fine.run_coarse_simulations(res, 10, dt=0.01, convergence_criteria=_LOOSE, bc=coarse.LDC_DOUBLE_LID, output_dir=str(tmp_path / "c"))
    batch = fine.FineSolverBatch([fine.problem(Re, 10, 10, 1.0, 1.0, 0.01, "QUICK", _LOOSE, coarse.LDC_DOUBLE_LID) for Re in res], resident=True)
    c0 = batch.counters()
    batch.solve()
    c1 = batch.counters()
    n_chunks = c1["launches"] - c0["launches"]
    assert batch.status.tolist() == [CONVERGED] * 3
    assert n_chunks == c1["host_syncs"] - c0["host_syncs"] == _chunks(0, 100000, int(batch.iterations.max()))
    for i in range(3):
        assert sorted(fields[i]) == ["p", "u", "v"] and fields[i]["u"].shape == (10, 10)
        for c in "uvp":
            _same(fields[i][c], batch.fields(i)[c])
    batch.close()
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == sorted(f"coarse_Re{Re}_10x10_100000_coarse_iterations.h5" for Re in res)
    r = fine.run_bfs_coarse_simulations([200.0, 400.0], 10, max_iterations=3)
    assert len(r) == 2 and r[0]["u"].shape == (10, 10) and np.isfinite(r[1]["p"]).all()
    # the generator: the same groups and values in both modes
    datasets = importlib.import_module("sr-for-cfd_amd.datasets")
    h5 = importlib.import_module("sr-for-cfd_amd.h5")
    recs, files = [], []
    for resident in ("auto", False):
        path = str(tmp_path / f"sweep_{resident}.h5")
        recs.append(datasets.generate_simulation_file(path, reynolds_numbers=[50, 100], mesh_sizes=(10, 20), dt=0.01, convergence_criteria=_LOOSE,
                                                      max_batch=2, resident=resident))
        with h5.H5File(path) as f:
            files.append({g: {d: f.read(f"{g}/{d}") for d in f.keys(g)} for g in f.keys("/")})
    assert recs[0] == recs[1] and all(st == CONVERGED for *_, st in recs[0])
    assert sorted(files[0]) == sorted(files[1]) == sorted(f"Re{Re}_mesh{n}x{n}" for Re in (50, 100) for n in (10, 20))
    for g in files[0]:
        assert sorted(files[0][g]) == sorted(files[1][g])
        for d in files[0][g]:
            _same(files[0][g][d], files[1][g][d])


# ---------------------------------------------------------------------------------------------- 10: refusals
def test_a_mesh_above_the_bound_is_refused_and_auto_falls_back(fine, coarse):
    assert fine.resident_supported(MAX, MAX) and not fine.resident_supported(MAX + 1, MAX)
    pb = fine.problem(100.0, MAX + 1, MAX, 1.0, 1.0, 0.001, "UPWIND", None, coarse.LDC_DOUBLE_LID)
    with pytest.raises(ValueError, match=rf"{MAX} x {MAX} cells, not {MAX + 1} x {MAX}"):
        fine.FineSolverBatch([pb], resident=True)
    with pytest.raises(ValueError, match=rf"not {MAX + 1} x {MAX}"):
        fine.FineSolver(pb, resident=True)
    with pytest.raises(ValueError, match="resident must be"):
        fine.FineSolver(pb, resident="yes")
    b = fine.FineSolverBatch([pb])
    with pytest.raises(ValueError, match=rf"srcfd_fine_batch_set_mode: .* not {MAX + 1} x {MAX}"):
        b.set_resident(True)
    assert b.resident is False
    ref = fine.FineSolverBatch([pb], resident="auto")          # falls back
    assert ref.resident is False
    for s in (b, ref):
        c0 = s.counters()
        assert s.run(2).tolist() == [2]
        c1 = s.counters()
        assert c1["launches"] - c0["launches"] > 2 * 20 and c1["host_syncs"] - c0["host_syncs"] >= 2 * 4   # per sweep: the launch mode
    _same(b.Var, ref.Var)
    b.close()
    ref.close()
    with pytest.raises(ValueError, match=rf"not {MAX + 1} x {MAX}"):
        fine.run_normal_simulations([100], MAX + 1, MAX, max_iterations=1, resident=True)
    # on a supported mesh "auto" is resident
    s = fine.FineSolver(fine.problem(100.0, MAX, 7, 1.0, 1.0, 0.001, "UPWIND", None, coarse.LDC_DOUBLE_LID), resident="auto")
    assert s.resident is True
    with _Counted(s, 1):
        s.run(2)
    s.close()
