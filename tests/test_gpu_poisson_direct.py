"""The direct pressure solve (csrc/poisson_direct.hip, `pressure="direct"`) on an MI355X, held to the references of
tests/poisson_direct_ref.py.  The mode has no numpy twin with equal bits, so tests 1 to 3 compare the device with `DirectDST` under
`ref.bound`: 8 x the distance of the two CPU evaluations (`DirectDST`, `DirectGEMM`) at the same checkpoint, computed at test time and
never from the device's result; each test prints the device's distance beside it.  Tests 4 to 6: fixed points, independence of the
batch, and the handling of the modes (where the sweeps' bits must be exactly what they were)."""
import importlib
import signal
import types

import numpy as np
import pytest

from conftest import require_gpu
import fine_solver_spec as spec
import poisson_direct_ref as ref
import solver_cross as X

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, DIVERGED = 0, 1, 2
_BFS = {"step_height": 1.0, "h": 2.0, "Ub": 1.0}
_ZERO = {"u": 0.0, "v": 0.0, "p": 0.0}


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _cpu(cls, pb, var, iterations):
    sp = ref.from_problem(cls, pb)
    sp.init(var)
    sp.run(iterations)
    return sp


def _hold(label, device_var, dst_var, gemm_var):
    """The device within ref.bound of DirectDST, per field; prints the figures; returns the worst ratio distance / bound."""
    b = ref.bound(dst_var, gemm_var)
    d = ref.distances(device_var, dst_var)
    ratio = float((d / b).max())
    print(f"{label}: |device - DirectDST| u {d[0]:.2e} v {d[1]:.2e} p {d[2]:.2e}; bound u {b[0]:.2e} v {b[1]:.2e} p {b[2]:.2e}; "
          f"worst ratio {ratio:.3f}")
    assert np.isfinite(device_var).all()
    assert (d <= b).all(), (label, d, b)
    return ratio


# ---------------------------------------------------------------------------------------------- 1: one solve at every kernel edge
# 32 x 32 tiles, 32-deep chunks, 16 x 16 MFMA tiles, 4-deep MFMA steps: below one MFMA tile; row, column and K tails of a tile; one
# past a tile either way; several tiles with tails in both directions
LDC_EDGES = [(3, 3), (13, 9), (9, 13), (37, 29), (64, 65), (65, 64), (131, 67)]


def _edge_problem(fine, nx, ny, bfs):
    if bfs:
        return fine.problem(100.0, nx, ny, 10.0, 3.0, 0.01, "UPWIND", _ZERO, None, bfs=_BFS, relaxation_factors={"u": 0.5, "v": 0.5, "p": 0.2})
    return fine.problem(100.0, nx, ny, 2.0, 1.0, 0.01, "QUICK", _ZERO)


@pytest.mark.parametrize("nx,ny,bfs", [(nx, ny, False) for nx, ny in LDC_EDGES] + [(37, 29, True)])
def test_one_solve_at_every_kernel_edge(fine, nx, ny, bfs):
    pb = _edge_problem(fine, nx, ny, bfs)
    var = ref.smooth_state(nx, ny, seed=nx + ny)
    s = fine.FineSolver(pb, pressure="direct")
    s.init(var)
    assert s.run(1) == 1
    got = s.Var
    c = s.counters()
    s.close()
    assert c["last_sweeps"][2] == 1 and c["pressure_sweeps"] == 1 and c["pressure_solver"] == "direct"
    dst, gemm = _cpu(ref.DirectDST, pb, var, 1), _cpu(ref.DirectGEMM, pb, var, 1)
    _hold(f"{'bfs' if bfs else 'ldc'} {nx}x{ny}", got, dst.Var, gemm.Var)
    # ghosts, corners: the ring follows from the interior through the boundary conditions, the corners stay what init made them
    for k in range(3):
        for i, j in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            assert got[k, i, j] == 0.0
    if not bfs and (nx, ny) in (LDC_EDGES[0], LDC_EDGES[-1]):
        # the solved system itself (a cavity does not under-relax p, so the interior is the solve's own output): the worst-case
        # forward error of one solve, which carries kappa on purpose
        exact = _cpu(ref.DirectLU, pb, var, 1).Var if nx * ny <= ref.LU_MAX_CELLS else dst.Var
        rel = np.linalg.norm(got[2, 1:-1, 1:-1] - exact[2, 1:-1, 1:-1]) / np.linalg.norm(exact[2, 1:-1, 1:-1])
        fb = ref.forward_bound(nx, ny, 2.0 / nx, 1.0 / ny)
        print(f"ldc {nx}x{ny}: relative 2-norm distance of p to the {'LU' if nx * ny <= ref.LU_MAX_CELLS else 'DST'} solve {rel:.2e} (bound {fb:.2e})")
        assert rel <= fb


# ---------------------------------------------------------------------------------------------- 2: trajectories
TRAJECTORY_CASES = ("ldc_quick_wide_single_lid", "channel_quick", "ldc_upwind_right_wall", "bfs_upwind_relax", "bfs_quick_relax_rho")


def _trajectory_batches():
    out = {}
    for name in TRAJECTORY_CASES:
        out.setdefault(X.batch_key(name), []).append(name)
    return list(out.values())


@pytest.mark.parametrize("names", _trajectory_batches(), ids=lambda names: "+".join(names))
def test_trajectories_to_the_second_checkpoint(fine, names):
    pbs = [X.problem(name) for name in names]
    stops = sorted({K for name in names for K in X.CASES[name][2][:2]})
    b = fine.FineSolverBatch(pbs, pressure="direct")
    got = {}
    for K in stops:
        b.run(K - int(b.iterations.max()))
        got[K] = b.Var
    assert b.status.tolist() == [RUNNING] * len(names)
    assert all(sw[2] == 1 for sw in b.counters()["last_sweeps"])
    b.close()
    for i, (name, pb) in enumerate(zip(names, pbs)):
        dst, gemm = ref.from_problem(ref.DirectDST, pb), ref.from_problem(ref.DirectGEMM, pb)
        dst.init()
        gemm.init()
        for K in X.CASES[name][2][:2]:
            dst.run(K - dst.count)
            gemm.run(K - gemm.count)
            assert np.abs(dst.Var[0]).max() > 0.1
            _hold(f"{name} at {K}", got[K][i], dst.Var, gemm.Var)


# ---------------------------------------------------------------------------------------------- 3: 400 x 400
@pytest.mark.parametrize("config", ["ldc_quick_re1000_double_lid", "bfs_upwind_re400"])
def test_400x400_three_outer_iterations(fine, config):
    coarse = importlib.import_module("sr-for-cfd_amd.coarse")
    if config.startswith("ldc"):
        pb = fine.problem(1000.0, 400, 400, 1.0, 1.0, 0.001, "QUICK", _ZERO, coarse.LDC_DOUBLE_LID)
    else:
        pb = fine.problem(400.0, 400, 400, 10.0, 3.0, 0.002, "UPWIND", _ZERO, None, bfs=_BFS)
    s = fine.FineSolver(pb, pressure="direct")
    assert s.run(3) == 3
    got = s.Var
    c = s.counters()
    s.close()
    assert c["pressure_sweeps"] == 3 and c["last_sweeps"][2] == 1
    dst, gemm = _cpu(ref.DirectDST, pb, None, 3), _cpu(ref.DirectGEMM, pb, None, 3)
    assert np.abs(dst.Var[2]).max() > 0
    _hold(config, got, dst.Var, gemm.Var)


# ---------------------------------------------------------------------------------------------- 4: fixed points
@pytest.mark.parametrize("name", sorted(X.FIXED))
def test_fixed_points(fine, name):
    f = X.FIXED[name]
    pb = X.problem(name, tolerance=f["tolerance"])
    s = fine.FineSolverBatch([pb], pressure="direct")
    s.run(f["cap"])
    got, count, status = s.case_var(0), int(s.iterations[0]), int(s.status[0])
    s.close()
    dst = _cpu(ref.DirectDST, pb, None, f["cap"])
    host = X.host_solve(pb, f["cap"])
    assert host is not None and host[1] == f["host_iterations"]
    d = X.differences(got, host[0], pb)
    print(f"{name}: device converges at {count}, DirectDST at {dst.count}, the host solver at {host[1]}; "
          f"|device - host| u {d[0]:.2e} v {d[1]:.2e} p {d[2]:.2e}")
    assert status == CONVERGED and dst.converged
    assert abs(count - dst.count) <= 2
    assert d[0] <= X.VELOCITY_CAP and d[1] <= X.VELOCITY_CAP and d[2] <= X.PRESSURE_CAP


# ---------------------------------------------------------------------------------------------- 5: independence and freezing
def _five_problems(fine, tolerances=None):
    rows = [(100.0, 2.0, 1.0, 0.01, 1.0), (40.0, 1.0, 1.0, 0.005, 1.3), (250.0, 1.5, 1.0, 0.01, 0.8), (60.0, 1.0, 2.0, 0.02, 1.0),
            (400.0, 3.0, 1.0, 0.004, 1.1)]
    tolerances = tolerances or [_ZERO] * 5
    return [fine.problem(Re, 37, 29, lx, ly, dt, "QUICK", tol, rho=rho) for (Re, lx, ly, dt, rho), tol in zip(rows, tolerances)]


def test_cases_do_not_depend_on_their_batch(fine):
    pbs = _five_problems(fine)
    var = np.stack([ref.smooth_state(37, 29, seed=10 + i) for i in range(5)])
    solo = []
    for pb, v in zip(pbs, var):
        s = fine.FineSolver(pb, pressure="direct")
        s.init(v)
        s.run(6)
        solo.append(s.Var)
        s.close()
    assert len({a.tobytes() for a in solo}) == 5
    for order in (list(range(5)), list(range(5))[::-1]):
        b = fine.FineSolverBatch([pbs[i] for i in order], pressure="direct")
        b.init(var[order])
        assert b.run(6).tolist() == [6] * 5
        got = b.Var
        b.close()
        for slot, i in enumerate(order):
            _same(got[slot], solo[i])


def test_a_frozen_case_is_left_alone(fine):
    loose = {"u": 1e6, "v": 1e6, "p": 1e6}
    pbs = _five_problems(fine, [_ZERO, _ZERO, loose, _ZERO, _ZERO])
    var = np.stack([ref.smooth_state(37, 29, seed=20 + i) for i in range(5)])
    b = fine.FineSolverBatch(pbs, pressure="direct")
    b.init(var)
    assert b.run(1).tolist() == [1] * 5
    assert b.status.tolist() == [RUNNING, RUNNING, CONVERGED, RUNNING, RUNNING]
    frozen = b.case_var(2)
    others = b.Var
    assert b.run(5).tolist() == [6, 6, 1, 6, 6]
    _same(b.case_var(2), frozen)
    after = b.Var
    b.close()
    for i in (0, 1, 3, 4):
        assert not np.array_equal(after[i], others[i])
    # and the frozen case is what it would have been alone
    s = fine.FineSolver(pbs[2], pressure="direct")
    s.init(var[2])
    s.run(6)
    _same(s.Var, frozen)
    assert s.iterations == 1
    s.close()


# ---------------------------------------------------------------------------------------------- 6: mode handling
def test_default_is_the_sweeps_with_their_bits_also_after_a_round_trip(fine):
    pb = fine.problem(100.0, 13, 9, 2.0, 1.0, 0.01, "QUICK", _ZERO)
    var = ref.smooth_state(13, 9, seed=3)
    sp = spec.from_problem(pb)
    sp.init(var)
    sp.run(2)
    for make in (lambda: fine.FineSolver(pb), lambda: fine.FineSolverBatch([pb])):
        s = make()
        assert s.pressure == "sweeps" and s.counters()["pressure_solver"] == "sweeps"
        first = lambda: s.Var if isinstance(s, fine.FineSolver) else s.Var[0]
        start = var if isinstance(s, fine.FineSolver) else var[None]
        s.init(start)
        s.run(2)
        _same(first(), sp.Var)
        sweeps = s.counters()["last_sweeps"]
        sweeps = sweeps if isinstance(s, fine.FineSolver) else sweeps[0]
        assert sweeps == sp.sweeps[-1] and sweeps[2] > 1
        assert s.set_pressure_solver("direct") == "direct"
        s.init(start)
        s.run(2)
        assert s.counters()["pressure_solver"] == "direct"
        assert not np.array_equal(first(), sp.Var)
        assert s.set_pressure_solver("sweeps") == "sweeps"
        s.init(start)
        s.run(2)
        _same(first(), sp.Var)
        assert s.counters()["pressure_solver"] == "sweeps"
        s.close()


def test_switching_between_runs(fine):
    """Two direct iterations, then two with the sweeps, on one handle without a new init: the CPU does the same with DirectDST and
    with DirectGEMM, and the device stays within their bound."""
    pb = fine.problem(100.0, 13, 9, 2.0, 1.0, 0.01, "QUICK", _ZERO)
    var = ref.smooth_state(13, 9, seed=4)
    chains = []
    for cls in (ref.DirectDST, ref.DirectGEMM):
        sp = _cpu(cls, pb, var, 2)
        sp.solve_pressure = types.MethodType(spec.Spec.solve_pressure, sp)
        sp.run(2)
        assert sp.count == 4 and sp.sweeps[1][2] == 1 and sp.sweeps[3][2] > 1
        chains.append(sp)
    s = fine.FineSolver(pb, pressure="direct")
    s.init(var)
    s.run(2)
    assert s.counters()["last_sweeps"][2] == 1
    s.set_pressure_solver("sweeps")
    assert s.run(2) == 4
    c = s.counters()
    assert c["last_sweeps"][2] == chains[0].sweeps[3][2] and c["pressure_solver"] == "sweeps"
    _hold("direct, direct, sweeps, sweeps", s.Var, chains[0].Var, chains[1].Var)
    s.close()


def test_resident_and_direct_refuse_each_other(fine):
    pb = fine.problem(100.0, 13, 9, 2.0, 1.0, 0.01, "QUICK", _ZERO)
    var = ref.smooth_state(13, 9, seed=5)
    for make in (lambda **kw: fine.FineSolver(pb, **kw), lambda **kw: fine.FineSolverBatch([pb, pb], **kw)):
        s = make(resident=True)
        with pytest.raises(ValueError) as e:
            s.set_pressure_solver("direct")
        assert "SRCFD_PRESSURE_DIRECT" in str(e.value) and "SRCFD_FINE_MODE_RESIDENT" in str(e.value)
        assert s.resident and s.pressure == "sweeps" and s.counters()["pressure_solver"] == "sweeps"
        s.run(2)                                  # still resident, still usable
        assert np.all(np.asarray(s.iterations) == 2)
        s.close()
        s = make(pressure="direct")
        with pytest.raises(ValueError) as e:
            s.set_resident(True)
        assert "SRCFD_PRESSURE_DIRECT" in str(e.value) and "SRCFD_FINE_MODE_RESIDENT" in str(e.value)
        assert not s.resident and s.pressure == "direct"
        assert s.set_resident("auto") is False    # "auto" resolves to launches on a direct handle
        s.run(2)
        assert np.all(np.asarray(s.iterations) == 2)
        for bad in ("multigrid", "", None, 1):
            with pytest.raises(ValueError):
                s.set_pressure_solver(bad)
        assert s.pressure == "direct" and s.counters()["pressure_solver"] == "direct"
        s.close()
        with pytest.raises(ValueError):
            make(resident=True, pressure="direct")
        with pytest.raises(ValueError):
            make(pressure="exact")
        s = make(resident="auto", pressure="direct")
        assert not s.resident and s.pressure == "direct"
        s.close()
    L = importlib.import_module("sr-for-cfd_amd._lib")
    s = fine.FineSolver(pb)
    assert L.lib.srcfd_fine_solver_set_pressure_solver(s._h, 2) == L.EINVAL
    assert L.lib.srcfd_fine_solver_set_pressure_solver(None, 1) == L.EINVAL
    assert L.lib.srcfd_fine_batch_set_pressure_solver(None, 1) == L.EINVAL
    s.init(var)
    s.run(1)
    s.close()


def test_run_normal_simulations_passes_the_mode_on(fine):
    reynolds = [50.0, 100.0, 200.0]
    kw = dict(dt=0.01, scheme="QUICK", convergence_criteria={"u": 1e-4, "v": 1e-4, "p": 1e-4}, max_iterations=60)
    out = fine.run_normal_simulations(reynolds, 13, 9, max_batch=2, pressure="direct", **kw)
    cc = {"u": 1e-4, "v": 1e-4, "p": 1e-4, "continuity": 1e-6}
    pbs = [fine.problem(Re, 13, 9, 1.0, 1.0, 0.01, "QUICK", cc) for Re in reynolds]
    for a in (0, 2):
        b = fine.FineSolverBatch(pbs[a:a + 2], 60, pressure="direct")
        b.solve()
        for i in range(b.n_cases):
            fields, it, st = out[a + i]
            assert (it, st) == (int(b.iterations[i]), int(b.status[i]))
            for c in "uvp":
                _same(fields[c], b.fields(i)[c])
        b.close()
    sweeps = fine.run_normal_simulations(reynolds[:1], 13, 9, **kw)
    assert not np.array_equal(sweeps[0][0]["p"], out[0][0]["p"])
