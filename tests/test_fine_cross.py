"""The fine-mesh solver's numpy specification (tests/fine_solver_spec.py, the bits the device must produce) against the host
solver srcfd_coarse_solve on the cases of tests/solver_cross.py: rectangular cells, UPWIND, rho != 1, under-relaxation, the whole
backward-facing-step path, single lids, moving side walls and a channel with mixed boundary types.  No GPU.  This is where the
bounds of the case table are measured: every test prints its figures before it asserts them against the table, and
test_gpu_fine_cross.py holds the device to the same numbers.

Three legs: trajectories from zero fields at tolerance 0, the cheapest cases to convergence, and perturbed problems given to the
specification alone, which the comparison has to reject."""
import importlib

import numpy as np
import pytest

import solver_cross as X


@pytest.fixture(scope="module", autouse=True)
def _library(srcfd):
    return importlib.import_module("sr-for-cfd_amd._lib")


_host_cache = {}


def _host_checkpoints(name):
    """The host solver's states at the case's checkpoints, from zero fields at tolerance 0 (None: non-finite residuals)."""
    if name not in _host_cache:
        pb = X.problem(name)
        _host_cache[name] = {K: X.host_solve(pb, K) for K in X.CASES[name][2]}
    return _host_cache[name]


def _host_fixed(name):
    key = (name, "fixed")
    if key not in _host_cache:
        f = X.FIXED[name]
        _host_cache[key] = X.host_solve(X.problem(name, f["tolerance"]), f["cap"])
    return _host_cache[key]


# ---------------------------------------------------------------------------------------------- the table itself
def test_table_covers_the_features_and_keeps_the_caps():
    kws = {n: c[1] for n, c in X.CASES.items()}
    assert set(X.TRAJECTORY) == set(X.CASES) and set(X.FIXED) <= set(X.CASES) and 2 <= len(X.FIXED) <= 3
    for name, (feature, kw, Ks) in X.CASES.items():
        assert feature and max(kw["nx"], kw["ny"]) <= X.MAX_CELLS, name
        assert len(Ks) == 3 and list(Ks) == sorted(set(Ks)) and Ks[-1] <= 400, name
        assert kw["lx"] / kw["nx"] != kw["ly"] / kw["ny"], name           # dx != dy everywhere
        fine = importlib.import_module("sr-for-cfd_amd.fine")
        assert fine.resident_supported(kw["nx"], kw["ny"]), name
    for table in (X.TRAJECTORY, {n: (f["measured"], f["bound"]) for n, f in X.FIXED.items()}):
        for name, (measured, bound) in table.items():
            assert len(measured) == len(bound) == 3 and all(m > 0 for m in measured), name
            assert bound == pytest.approx([X.MARGIN * m for m in measured], rel=1e-9), name
            assert bound[0] <= X.VELOCITY_CAP and bound[1] <= X.VELOCITY_CAP and bound[2] <= X.PRESSURE_CAP, name
    for f in X.FIXED.values():
        assert f["tolerance"] in (1e-8, 1e-9) and f["cap"] <= X.FIXED_CAP and f["host_iterations"] < f["cap"]
    ldc = [n for n, kw in kws.items() if "bfs" not in kw]
    bfs = [n for n, kw in kws.items() if "bfs" in kw]
    # both aspect orders, both schemes on both case types, rho on both case types
    assert any(kws[n]["nx"] > kws[n]["ny"] for n in ldc) and any(kws[n]["nx"] < kws[n]["ny"] for n in ldc)
    for group in (ldc, bfs):
        assert {kws[n]["scheme"] for n in group} == {"QUICK", "UPWIND"}
        assert any(kws[n].get("rho", 1.0) not in (1.0,) for n in group)
    # every side carries a non-zero Dirichlet value for some variable in some case; a single lid, a left wall, a bottom lid alone
    moving = {n: {(c, s) for c in "uvp" for s, (t, v) in kws[n]["bc"][c].items() if t == "dirichlet" and v != 0.0} for n in ldc}
    assert {s for m in moving.values() for _, s in m} == {"left", "right", "top", "bottom"}
    for only in (("u", "top"), ("v", "left"), ("u", "bottom")):
        assert any(m == {only} for m in moving.values()), only
    # the channel's mixed types
    pb = X.problem("channel_quick")
    assert pb.case_type == 0 and [list(r) for r in pb.bc_type] == [[0, 1, 0, 0], [0, 1, 0, 0], [1, 0, 1, 1]]
    assert pb.bc_value[0][0] == 1.0 and pb.bc_value[2][1] == 0.25 and not X.pressure_is_floating(pb)
    assert all(X.pressure_is_floating(X.problem(n)) == (n != "channel_quick") for n in ldc)
    # the four BFS variants at lx 10, ly 3
    assert all((kws[n]["lx"], kws[n]["ly"]) == (10.0, 3.0) and not X.pressure_is_floating(X.problem(n)) for n in bfs)
    pb = X.problem("bfs_upwind_defaults")
    assert (pb.case_type, pb.step_height, pb.channel_height, pb.bulk_velocity, list(pb.relax)) == (1, 1.0, 2.0, 1.0, [0.5, 0.5, 0.2])
    assert list(X.problem("bfs_upwind_relax").relax) == [0.7, 0.6, 0.3]
    assert list(X.problem("bfs_upwind_no_relaxation").relax) == [1.0, 1.0, 1.0]
    assert list(X.problem("bfs_upwind_fixed").relax) == [0.5, 0.5, 0.2]
    pb = X.problem("bfs_upwind_step_geometry")
    assert (pb.step_height, pb.channel_height, pb.bulk_velocity) == (1.3, 1.7, 0.8)
    wall, inlet = X.inlet_rows(pb)
    assert (wall, inlet) == ([1, 2, 3], [4, 5, 6, 7])
    dy = pb.ly / pb.ny
    assert (wall[-1] - 0.5) * dy < pb.step_height < (inlet[0] - 0.5) * dy       # strictly between two cell centres
    assert X.inlet_rows(X.problem("bfs_upwind_defaults")) == ([1, 2], [3, 4, 5, 6, 7])   # step 1.0: between 0.643 and 1.071
    # every batch of the GPU test holds cases that differ in Re, dt and more
    for names in X.batches().values():
        assert len(names) >= 2 and len({kws[n]["Re"] for n in names}) >= 2 and len({kws[n]["dt"] for n in names}) >= 2, names


def test_inlet_rows_are_the_rows_the_host_solver_treats_as_wall_and_inlet():
    """From the host solver's own state: on a wall row the ghost cell mirrors u to zero on the face, on an inlet row to the parabola."""
    pb = X.problem("bfs_upwind_step_geometry")
    var, it, _ = X.host_solve(pb, 5)
    wall, inlet = X.inlet_rows(pb)
    face = 0.5 * (var[0, 0, 1:-1] + var[0, 1, 1:-1])
    yp = (np.array(inlet) - 0.5) * (pb.ly / pb.ny) - pb.step_height
    np.testing.assert_allclose(face[np.array(wall) - 1], 0.0, atol=1e-15)
    np.testing.assert_allclose(face[np.array(inlet) - 1], 6.0 * pb.bulk_velocity * (yp / pb.channel_height) * (1.0 - yp / pb.channel_height), atol=1e-15)
    assert (face[np.array(inlet) - 1] > 0.3).all()


# ---------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize("name", list(X.CASES))
def test_trajectory_stays_within_inner_tolerance_noise_of_the_host_solver(name):
    Ks = X.CASES[name][2]
    pb = X.problem(name)
    host = _host_checkpoints(name)
    for K in Ks:
        assert host[K] is not None, f"{name}: the host solver is not finite at {K}"
        var, it, rms = host[K]
        assert it == K and np.isfinite(var).all() and np.isfinite(rms).all()
        assert np.abs(var[0, 1:-1, 1:-1]).max() >= X.MIN_SPEED, (name, K)
    sp, states = X.spec_run(pb, Ks)
    assert sp.count == Ks[-1] and not sp.converged
    measured, bound = X.TRAJECTORY[name]
    worst = np.zeros(3)
    for K in Ks:
        d = X.differences(states[K], host[K][0], pb)
        print(f"{name} K {K}: |du| {d[0]:.3e} |dv| {d[1]:.3e} |dp| {d[2]:.3e}  max |u| {np.abs(host[K][0][0, 1:-1, 1:-1]).max():.3f}")
        worst = np.maximum(worst, d)
    print(f"{name} worst {worst[0]:.3e} {worst[1]:.3e} {worst[2]:.3e}  table {measured}  bound {bound}")
    assert (worst <= np.array(bound)).all(), (name, worst, bound)


# ---------------------------------------------------------------------------------------------- fixed points
@pytest.mark.parametrize("name", list(X.FIXED))
def test_both_codes_converge_to_one_fixed_point_at_one_iteration(name):
    f = X.FIXED[name]
    pb = X.problem(name, f["tolerance"])
    var, it, rms = _host_fixed(name)
    assert it < f["cap"] and (rms <= f["tolerance"]).all() and it == f["host_iterations"]
    assert np.abs(var[0, 1:-1, 1:-1]).max() >= X.MIN_SPEED
    sp, _ = X.spec_run(pb, (f["cap"],))
    d = X.differences(sp.Var, var, pb)
    print(f"{name}: host {it}, specification {sp.count} iterations, last sweeps {sp.sweeps[-1]}; |du| {d[0]:.3e} |dv| {d[1]:.3e} |dp| {d[2]:.3e}")
    assert sp.converged and sp.count == f["spec_iterations"] and abs(sp.count - it) <= 2
    assert sp.sweeps[-1] == f["last_sweeps"]
    assert (d <= np.array(f["bound"])).all(), (name, d, f["bound"])


# ---------------------------------------------------------------------------------------------- sensitivity
_STEP_UP = {"step_height": 1.0 + 3.0 / 7.0, "h": 2.0, "Ub": 1.0}        # one cell of the 10 x 7 mesh: row 3 turns from inlet to wall
# perturbation: (case the host solver gets as it is, what the specification gets instead, whether it moves the fixed point)
PERTURBATIONS = {
    "relax_p_0.2_to_0.3": ("bfs_upwind_fixed", dict(relaxation_factors={"u": 0.5, "v": 0.5, "p": 0.3}), False),
    "dt_times_1.1": ("bfs_upwind_fixed", dict(dt=0.4 * 1.1), True),
    "step_height_one_cell_up": ("bfs_upwind_fixed", dict(bfs=_STEP_UP), True),
    "bulk_velocity_times_0.9": ("bfs_upwind_fixed", dict(bfs={"step_height": 1.0, "h": 2.0, "Ub": 0.9}), True),
    "rho_1.3_to_1.0": ("ldc_quick_rho_fixed", dict(rho=1.0), True),
    "lx_and_ly_exchanged": ("ldc_quick_rho_fixed", dict(lx=1.0, ly=1.5), True),
    "upwind_for_quick": ("ldc_quick_rho_fixed", dict(scheme="UPWIND"), True),
    "lid_on_bottom_for_top": ("ldc_quick_rho_fixed", dict(bc=X._walls(u_bottom=1.5)), True),
}


@pytest.mark.parametrize("perturbation", list(PERTURBATIONS))
def test_a_perturbed_specification_is_rejected(perturbation):
    """The comparison can fail: one modestly changed parameter moves the specification past 10 x the bound at some checkpoint
    of the trajectory leg; the fixed-point leg sees exactly the changes that move the fixed point, and passes on the other.
    Measured, as multiples of the bound (trajectory | fixed point): relax 9.6e4 | 0.32, dt 3.3e4 | 2.6e3, step_height 1.4e5 |
    1.1e5, bulk velocity 3.1e4 | 2.5e4, rho 2.1e4 | 2.1e4, lx / ly 6.6e4 | 6.7e4, UPWIND 7.8e3 | 8.0e3, lid 1.6e5 | 1.7e5.
    (The issue that asked for this test expected dt to leave the fixed point alone, as the relaxation factors do.  It does
    not: at the fixed point the momentum solve still moves u by dt / rho grad p, which the projection takes back, so the
    converged velocity carries a splitting term of order dt -- in the host solver as in the specification.  At dt 0.4 -> 0.44
    that is 1.5e-2, and the test asserts what both codes do.)"""
    name, changed, moves_fixed_point = PERTURBATIONS[perturbation]
    Ks, f = X.CASES[name][2], X.FIXED[name]
    host = _host_checkpoints(name)
    pb = X.problem(name, f["tolerance"])
    sp, states = X.spec_run(X.problem(name, f["tolerance"], **changed), Ks)
    assert sp.count == Ks[-1] and not sp.converged
    ratio = max((X.differences(states[K], host[K][0], pb) / np.array(X.TRAJECTORY[name][1])).max() for K in Ks)
    sp.run(f["cap"] - sp.count)
    assert sp.converged
    fixed_ratio = (X.differences(sp.Var, _host_fixed(name)[0], pb) / np.array(f["bound"])).max()
    print(f"{perturbation} on {name}: trajectory {ratio:.3g} x bound, fixed point {fixed_ratio:.3g} x bound after {sp.count} iterations")
    assert ratio >= 10.0
    if moves_fixed_point:
        assert fixed_ratio >= 10.0
    else:
        assert fixed_ratio <= 1.0
