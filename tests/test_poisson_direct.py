"""The direct pressure solve on the CPU: the basis the library builds (srcfd_poisson_basis, csrc/poisson_plan.cpp), the three
references of tests/poisson_direct_ref.py against each other, and the direct mode as the limit of the red-black sweeps -- the
specification with an exact pressure solve against the unchanged specification on the cases of tests/solver_cross.py, along
trajectories and at the fixed points.  Nothing here needs a GPU; tests/test_gpu_poisson_direct.py holds the device to these
references."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import fine_solver_spec as spec
import poisson_direct_ref as ref
import solver_cross as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("sr-for-cfd_amd._lib")


# ---------------------------------------------------------------------------------------------- 1: the basis
def _basis(L, n):
    S, lam = np.full((n, n), np.nan), np.full(n, np.nan)
    L.check(L.lib.srcfd_poisson_basis(n, S.ctypes.data_as(C.c_void_p), lam.ctypes.data_as(C.c_void_p)))
    return S, lam


@pytest.mark.parametrize("n", [1, 3, 9, 37, 64, 65, 400])
def test_basis_is_symmetric_orthogonal_and_has_the_eigenvalues(L, n):
    S, lam = _basis(L, n)
    assert np.array_equal(S.view(np.uint64), S.T.copy().view(np.uint64)), "S is not symmetric to the bit"
    # S S = I with the products and sums in long double: the bound is about S's entries (rounded once, |s|^2 <= 2 / (n + 1), n
    # products), not about the rounding of a float64 matrix product
    Sl = S.astype(np.longdouble)
    err = float(np.abs(Sl @ Sl - np.eye(n, dtype=np.longdouble)).max())
    print(f"n {n}: max |S S - I| = {err / U:.2f} u (bound 16 u)")
    assert err <= 16 * U
    want = ref.eigenvalues(n)       # -4 sin^2(pi (a + 1) / (2 (n + 1))) in numpy's long double
    ulps = np.abs(lam - want) / np.spacing(np.abs(want))
    print(f"n {n}: lambda within {ulps.max():.1f} ulp of the long-double form (bound 4)")
    assert ulps.max() <= 4
    # the entries themselves, against numpy's long double: a transposed index or a wrong normalisation is not a rounding matter
    assert np.abs(S - ref.basis(n)).max() <= 4 * U


def test_basis_refuses_n_below_1_and_skips_null_outputs(L):
    one = np.array([7.0])
    for n in (0, -5):
        assert L.lib.srcfd_poisson_basis(n, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == L.EINVAL
        assert "srcfd_poisson_basis" in L.last_error()
    assert one[0] == 7.0
    with pytest.raises(ValueError):
        L.check(L.lib.srcfd_poisson_basis(0, None, None))
    lam = np.zeros(4)
    assert L.lib.srcfd_poisson_basis(4, None, lam.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(lam, _basis(L, 4)[1])


def test_plan_check_under_sanitizers():
    """tools/poisson_plan_check.cpp + poisson_plan.cpp under AddressSanitizer + UBSan, on the CPU: n = 1 .. 70 and 400, the padded
    form the kernels read included."""
    csrc = os.path.join(ROOT, "sr-for-cfd_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "poisson_plan_check"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "sr-for-cfd_amd", "lib", "poisson_plan_check_asan")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["71"]


def test_constants_and_exports_match_the_header(L):
    text = open(os.path.join(ROOT, "include", "srcfd.h")).read()
    assert "#define SRCFD_PRESSURE_SWEEPS 0" in text and "#define SRCFD_PRESSURE_DIRECT 1" in text
    assert (L.PRESSURE_SWEEPS, L.PRESSURE_DIRECT) == (0, 1) and L.PRESSURE_SOLVERS == {"sweeps": 0, "direct": 1}
    for name in ("srcfd_fine_batch_set_pressure_solver", "srcfd_fine_solver_set_pressure_solver", "srcfd_poisson_basis"):
        assert name in L.EXPORTED and f"int {name}(" in text


# ---------------------------------------------------------------------------------------------- 2: the three references agree
def _one_solve_state(cls, nx, ny, lx, ly, seed):
    """A cavity specification of class `cls` primed from a smooth non-zero state: `solve_pressure` on it is one exact solve
    with non-zero rhs and non-zero ghosts on all four sides."""
    sp = cls(nx, ny, lx, ly, 100.0, 1.3, 0.01, "QUICK", [0.0] * 3, [[0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 1, 0]],
             [[0, 0, 1.0, 0], [0] * 4, [0, 0.25, 0, -0.5]])
    sp.init(ref.smooth_state(nx, ny, seed))
    return sp


@pytest.mark.parametrize("nx,ny", [(3, 3), (13, 9), (37, 29)])
def test_three_references_agree_on_one_solve(nx, ny):
    lx, ly = 2.0, 1.0
    sols = {}
    for cls in (ref.DirectLU, ref.DirectDST, ref.DirectGEMM):
        sp = _one_solve_state(cls, nx, ny, lx, ly, seed=nx)
        g = sp.rhs_and_ghosts()
        assert np.abs(sp.Var[2][[0, -1], 1:-1]).min() > 0 and np.abs(sp.Var[2][1:-1, [0, -1]]).min() > 0 and np.abs(g).min() > 0
        assert sp.solve_pressure() == 1
        sols[cls.__name__] = sp.Var[2, 1:-1, 1:-1].copy()
        # the solved system itself, with the stencil of Spec.solve_pressure: the ghosts are still in place
        P = sp.Var[2]
        Fd = sp.volp * ((P[2:, 1:-1] - 2 * P[1:-1, 1:-1] + P[:-2, 1:-1]) / sp.dx ** 2 + (P[1:-1, 2:] - 2 * P[1:-1, 1:-1] + P[1:-1, :-2]) / sp.dy ** 2)
        F = sp.Ff
        rhs = sp.rho / sp.dt * (F[0] + F[1] + F[2] + F[3])[1:-1, 1:-1]
        assert np.linalg.norm(rhs - Fd) <= 1e-9 * np.linalg.norm(rhs), cls.__name__
    bound = ref.forward_bound(nx, ny, lx / nx, ly / ny)
    lu = sols["DirectLU"]
    for a, b in (("DirectLU", "DirectDST"), ("DirectLU", "DirectGEMM"), ("DirectDST", "DirectGEMM")):
        d = np.linalg.norm(sols[a] - sols[b]) / np.linalg.norm(lu)
        print(f"{nx}x{ny}: {a} - {b} = {d:.2e} relative (bound {bound:.2e})")
        assert d <= bound


# ---------------------------------------------------------------------------------------------- 3: the direct mode is the sweeps' limit
TRAJECTORY_CASES = ("ldc_quick_wide_single_lid", "ldc_upwind_fixed", "bfs_upwind_defaults", "bfs_quick_defaults")
# outer iterations to convergence at tolerance 1e-8 with an exact pressure solve (measured with DirectDST on the CPU); the sweeps' own
# counts are solver_cross.FIXED's spec_iterations
DIRECT_FIXED_ITERATIONS = {"ldc_quick_rho_fixed": 441, "ldc_upwind_fixed": 767, "bfs_upwind_fixed": 701}


def _run(cls, pb, checkpoints):
    sp = ref.from_problem(cls, pb) if cls is not spec.Spec else spec.from_problem(pb)
    sp.init()
    out = {}
    for K in checkpoints:
        sp.run(K - sp.count)
        out[K] = sp.Var.copy()
    return sp, out


@pytest.fixture(scope="module")
def sweeps_trajectories():
    """The unchanged specification at every checkpoint of the trajectory cases, computed once."""
    return {name: _run(spec.Spec, X.problem(name), X.CASES[name][2])[1] for name in TRAJECTORY_CASES}


def _within_caps(cls, name, sweeps):
    """Whether `cls` stays within the caps of the sweeps' trajectory of case `name`; the largest differences."""
    pb = X.problem(name)
    try:
        _, direct = _run(cls, pb, X.CASES[name][2])
    except ValueError:          # non-finite residuals
        return False, np.full(3, np.inf)
    worst = np.max([X.differences(direct[K], sweeps[K], pb) for K in X.CASES[name][2]], axis=0)
    ok = bool(np.isfinite(worst).all() and worst[0] <= X.VELOCITY_CAP and worst[1] <= X.VELOCITY_CAP and worst[2] <= X.PRESSURE_CAP)
    return ok, worst


@pytest.mark.parametrize("name", TRAJECTORY_CASES)
def test_direct_trajectory_stays_with_the_sweeps(name, sweeps_trajectories):
    ok, worst = _within_caps(ref.DirectDST, name, sweeps_trajectories[name])
    print(f"{name}: max |direct - sweeps| u {worst[0]:.2e} v {worst[1]:.2e} p {worst[2]:.2e} (caps {X.VELOCITY_CAP:g}, {X.PRESSURE_CAP:g})")
    assert ok, worst


@pytest.mark.parametrize("name", sorted(X.FIXED))
def test_direct_and_sweeps_share_the_fixed_point(name):
    f = X.FIXED[name]
    pb = X.problem(name, tolerance=f["tolerance"])
    sweeps, a = _run(spec.Spec, pb, (f["cap"],))
    direct, b = _run(ref.DirectDST, pb, (f["cap"],))
    assert sweeps.converged and direct.converged
    d = X.differences(a[f["cap"]], b[f["cap"]], pb)
    print(f"{name}: sweeps converge at {sweeps.count}, direct at {direct.count}; states differ by u {d[0]:.1e} v {d[1]:.1e} p {d[2]:.1e}")
    assert abs(sweeps.count - f["spec_iterations"]) <= 2
    assert abs(direct.count - DIRECT_FIXED_ITERATIONS[name]) <= 2
    assert d[0] <= X.VELOCITY_CAP and d[1] <= X.VELOCITY_CAP and d[2] <= X.PRESSURE_CAP


# ---------------------------------------------------------------------------------------------- 4: sensitivity
@pytest.mark.parametrize("flaw", ["swap_dx_dy", "drop_ghost", "lambda_of_n_plus_1"])
def test_a_flawed_direct_solve_leaves_the_caps(flaw, sweeps_trajectories):
    """Comparison 3 with one mistake in DirectDST alone: the cases do not all stay within the caps."""
    flawed = type(f"DirectDST_{flaw}", (ref.DirectDST,), {flaw: True})
    results = {name: _within_caps(flawed, name, sweeps_trajectories[name]) for name in TRAJECTORY_CASES}
    for name, (ok, worst) in results.items():
        print(f"{flaw}, {name}: within caps {ok}; u {worst[0]:.2e} v {worst[1]:.2e} p {worst[2]:.2e}")
    assert not all(ok for ok, _ in results.values())
    # the cavity with dx != dy and Neumann pressure walls sees all three mistakes by itself
    assert not results["ldc_quick_wide_single_lid"][0]
