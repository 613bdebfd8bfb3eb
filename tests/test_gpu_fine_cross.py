"""The device fine-mesh solver (csrc/fine_solver.hip, fine.FineSolver and fine.FineSolverBatch, resident and launch modes) on an
MI355X against the host solver srcfd_coarse_solve, on the cases of tests/solver_cross.py and at that table's bounds: rectangular
cells, UPWIND, rho != 1, under-relaxation, the backward-facing-step path, single lids, moving side walls, a channel with mixed
boundary types.  The numpy specification plays no part here; tests/test_fine_cross.py measured the bounds with it on the CPU.
All cases of one mesh, scheme and case type run as one batch, so Re, dt, lx, ly, rho, the boundary values and the relaxation
factors differ per case inside a batch."""
import importlib
import signal

import numpy as np
import pytest

from conftest import require_gpu
import solver_cross as X

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED = 0, 1
# seconds, sized to each test: the slowest, the five-case 13 x 9 batch through 400 outer iterations with its host solves, takes
# 0.4 s; the launch-mode test enqueues about 200 launches per outer iteration for 100 iterations and takes 0.25 s
_LIMITS = {"test_resident_batches_follow_the_host_solver": 10, "test_launch_mode_and_a_single_solver_give_the_resident_bits": 10,
           "test_device_converges_where_the_host_solver_converges": 10}


@pytest.fixture(autouse=True)
def _time_limit(request):
    """Every test here runs under its own time limit, sized to it (each takes a second or two)."""
    def _alarm(*_):
        raise TimeoutError(f"{request.node.name} exceeded its time limit")
    old = signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(_LIMITS[request.node.originalname])
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def fine(srcfd):
    require_gpu(srcfd)
    return importlib.import_module("sr-for-cfd_amd.fine")


_host_cache = {}


def _host(name, K):
    """The host solver's state after K outer iterations from zero fields at tolerance 0."""
    if (name, K) not in _host_cache:
        got = X.host_solve(X.problem(name), K)
        assert got is not None and got[1] == K, (name, K)
        assert np.abs(got[0][0, 1:-1, 1:-1]).max() >= X.MIN_SPEED, (name, K)
        _host_cache[name, K] = got[0]
    return _host_cache[name, K]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check(name, K, var):
    pb = X.problem(name)
    d = X.differences(var, _host(name, K), pb)
    bound = X.TRAJECTORY[name][1]
    print(f"{name} K {K}: |du| {d[0]:.3e} |dv| {d[1]:.3e} |dp| {d[2]:.3e}  bound {bound}")
    assert np.isfinite(var).all() and (d <= np.array(bound)).all(), (name, K, d, bound)


def _run_to_checkpoints(b, names, stop=None):
    """Runs a batch from zero fields through the union of its cases' checkpoints (up to `stop`); returns {(name, K): Var}."""
    wanted = sorted({K for n in names for K in X.CASES[n][2] if stop is None or K <= stop})
    out, at = {}, 0
    for K in wanted:
        assert b.run(K - at).tolist() == [K] * len(names)
        at = K
        assert b.status.tolist() == [RUNNING] * len(names)
        var = b.Var
        for i, n in enumerate(names):
            if K in X.CASES[n][2]:
                out[n, K] = var[i]
    return out


@pytest.mark.parametrize("key", list(X.batches()), ids=lambda k: f"{k[0]}x{k[1]}_{k[2].lower()}_{'bfs' if k[3] else 'ldc'}")
def test_resident_batches_follow_the_host_solver(fine, key):
    names = X.batches()[key]
    b = fine.FineSolverBatch([X.problem(n) for n in names], resident=True)
    assert b.resident is True and b.n_cases == len(names) >= 2
    c0 = b.counters()
    states = _run_to_checkpoints(b, names)
    c1 = b.counters()
    # the resident path ran: one launch and one host synchronisation per chunk of at most 100 outer iterations
    assert c1["launches"] - c0["launches"] == c1["host_syncs"] - c0["host_syncs"] <= 3 * len(names) + 4
    b.close()
    assert sorted(states) == sorted((n, K) for n in names for K in X.CASES[n][2])
    for (n, K), var in states.items():
        _check(n, K, var)


def test_launch_mode_and_a_single_solver_give_the_resident_bits(fine):
    """The BFS UPWIND batch once more with one launch per sweep, and one of its cases as a FineSolver: the resident bits."""
    names = X.batches()[10, 7, "UPWIND", True]
    stop = 100
    got = {}
    for resident in (True, False):
        b = fine.FineSolverBatch([X.problem(n) for n in names], resident=resident)
        assert b.resident is resident
        c0 = b.counters()
        got[resident] = _run_to_checkpoints(b, names, stop)
        c1 = b.counters()
        if not resident:
            assert c1["launches"] - c0["launches"] > 20 * stop          # per sweep: the launch mode
        b.close()
    assert sorted(got[True]) == sorted(got[False]) and len(got[True]) >= 3 * len(names) - 1
    for k in got[True]:
        np.testing.assert_array_equal(_bits(got[False][k]), _bits(got[True][k]), err_msg=str(k))
        _check(*k, got[False][k])
    name = "bfs_upwind_step_geometry"
    s = fine.FineSolver(X.problem(name))
    assert s.resident is False
    for K in X.CASES[name][2]:
        assert s.run(K - s.iterations) == K
        var = s.Var
        np.testing.assert_array_equal(_bits(var), _bits(got[True][name, K]))
        _check(name, K, var)
    s.close()


@pytest.mark.parametrize("name", list(X.FIXED))
def test_device_converges_where_the_host_solver_converges(fine, name):
    f = X.FIXED[name]
    pb = X.problem(name, f["tolerance"])
    host = X.host_solve(pb, f["cap"])
    assert host is not None and host[1] < f["cap"] and (host[2] <= f["tolerance"]).all()
    assert np.abs(host[0][0, 1:-1, 1:-1]).max() >= X.MIN_SPEED
    b = fine.FineSolverBatch([pb], resident=True)
    it = int(b.run(f["cap"])[0])
    var, sweeps = b.case_var(0), b.counters()["last_sweeps"][0]
    d = X.differences(var, host[0], pb)
    print(f"{name}: host {host[1]}, device {it} iterations, last sweeps {sweeps}; |du| {d[0]:.3e} |dv| {d[1]:.3e} |dp| {d[2]:.3e}  bound {f['bound']}")
    assert b.status.tolist() == [CONVERGED] and (b.rms[0] <= f["tolerance"]).all()
    assert abs(it - host[1]) <= 2
    # what the specification, whose bits the device has, showed on the CPU (the host solver does not report its inner sweeps)
    assert it == f["spec_iterations"] and sweeps == f["last_sweeps"]
    assert (d <= np.array(f["bound"])).all(), (name, d, f["bound"])
    b.close()
