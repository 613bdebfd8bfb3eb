"""The device fine-mesh solver (csrc/fine_solver.hip, sr-for-cfd_amd/fine.py) on an MI355X: the same bits as its numpy
specification (tests/fine_solver_spec.py), pinned to the reference's stored coarse field, the SR hand-off straight into the
device state, resumable and deterministic runs, and the reference's drop-in functions."""
import importlib
import os
import signal

import numpy as np
import pytest

from conftest import ENCODER_H5, GOLDEN, STATS_TXT, require_gpu
import fine_solver_spec as spec

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit(request):
    """Every test here runs under its own time limit (the slowest, the 59 765-iteration pinned run, takes well under it)."""
    def _alarm(*_):
        raise TimeoutError(f"{request.node.name} exceeded its time limit")
    old = signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(240)
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


def _cases(fine, coarse):
    return {
        "ldc_quick_double_lid": fine.problem(1000.0, 37, 29, 1.0, 1.0, 0.001, "QUICK", None, coarse.LDC_DOUBLE_LID),
        "bfs_upwind": fine.problem(400.0, 37, 29, 10.0, 3.0, 0.002, "UPWIND", None, None,
                                   bfs={"step_height": 1.0, "h": 2.0, "Ub": 1.0}),
        # QUICK at the Neumann outlet with backflow reads past the plane (Grid::vw's run-on reads)
        "bfs_quick_outlet_backflow": fine.problem(400.0, 37, 29, 10.0, 3.0, 0.002, "QUICK", None, None,
                                                  bfs={"step_height": 1.0, "h": 2.0, "Ub": 1.0}),
    }


@pytest.mark.parametrize("case", ["ldc_quick_double_lid", "bfs_upwind", "bfs_quick_outlet_backflow"])
def test_device_equals_the_specification_bit_for_bit(fine, coarse, case):
    pb = _cases(fine, coarse)[case]
    var0 = _smooth_state(37, 29, seed=7)
    sp = spec.from_problem(pb)
    sp.init(var0)
    s = fine.FineSolver(pb)
    s.init(var0)
    np.testing.assert_array_equal(_bits(s.Var), _bits(sp.Var))
    if case == "bfs_quick_outlet_backflow":
        f0 = sp.Ff[0, 37, 1:-1]
        assert (f0 < 0).any(), "the state has no backflow at the outlet: the run-on reads are not exercised"
    for n in range(1, 6):
        assert s.run(1) == n
        sp.run(1)
        assert s.counters()["last_sweeps"] == sp.sweeps[-1], (n, s.counters()["last_sweeps"], sp.sweeps[-1])
        np.testing.assert_array_equal(_bits(s.rms), _bits(sp.rms))
    np.testing.assert_array_equal(_bits(s.Var), _bits(sp.Var))
    assert s.iterations == sp.count == 5


def test_pinned_to_the_reference_field(srcfd, fine, coarse):
    """10x10, Re 800, double lid, from zero to the iteration at which the reference wrote its stored field
    (tests/test_coarse_solver.py CASES).  Measured (the device equals tests/fine_solver_spec.py bit for bit): u 6.1e-8,
    v 3.4e-8, p 2.4e-8 -- inside the reference's own run-to-run spread of 1.9e-7; bound = 3 x measured."""
    ref = srcfd.read_coarse_fields(os.path.join(GOLDEN, "coarse_ldc_Re800_double_lid.h5"))
    s = fine.FineSolver(fine.problem(800.0, 10, 10, bc=coarse.LDC_DOUBLE_LID, convergence_criteria={"u": 0.0, "v": 0.0, "p": 0.0}))
    assert s.run(59765) == 59765
    got = s.fields()
    bound = {"u": 1.8e-7, "v": 1.0e-7, "p": 7.2e-8}
    assert np.abs(got["u"] - ref["u"]).max() <= bound["u"]
    assert np.abs(got["v"] - ref["v"]).max() <= bound["v"]
    dp = got["p"] - ref["p"]            # all-Neumann pressure: defined up to a constant
    assert np.abs(dp - dp.mean()).max() <= bound["p"]


@pytest.fixture(scope="module")
def model(srcfd):
    require_gpu(srcfd)
    synth = importlib.import_module("sr-for-cfd_amd.synth")
    enc_w = srcfd.SRModel.load_h5(ENCODER_H5, None, device=-1).weights()
    return srcfd.SRModel.from_weights(enc_w, synth.synthetic_decoder_weights(1), device=0)


def _sr_inputs(srcfd, name):
    lr, hr = srcfd.load_stats(STATS_TXT, 10, 400)
    coarse = srcfd.read_coarse_fields(os.path.join(GOLDEN, name))
    x = np.stack([coarse[c].astype(np.float32) for c in "uvp"])[..., None]
    return x, np.array([lr[c] for c in "uvp"], np.float32), np.array([hr[c] for c in "uvp"], np.float32)


def test_hand_off_into_the_device_state_ldc(srcfd, fine, coarse, model):
    pipeline = importlib.import_module("sr-for-cfd_amd.pipeline")
    x, ain, aout = _sr_inputs(srcfd, "coarse_ldc_Re800_double_lid.h5")
    types, values = pipeline.bc_arrays(coarse.LDC_DOUBLE_LID)
    host = model.predict_into_solver_state(x, types, values, in_affine=ain, out_affine=aout, nan_guard=True)
    pb = fine.problem(800.0, 400, 400, bc=coarse.LDC_DOUBLE_LID)
    s = fine.FineSolver(pb)
    assert s.init_from_prediction(model, x, ain, aout) == 0
    dev = s.Var
    np.testing.assert_array_equal(dev, host)
    t = fine.FineSolver(pb)
    t.init(host)
    np.testing.assert_array_equal(_bits(t.Var), _bits(dev))


def test_hand_off_into_the_device_state_bfs(srcfd, fine, model):
    pipeline = importlib.import_module("sr-for-cfd_amd.pipeline")
    rs = importlib.import_module("sr-for-cfd_amd.resample")
    x, ain, aout = _sr_inputs(srcfd, "coarse_bfs_Re400.h5")
    nx, ny, lx, ly = 400, 400, 10.0, 3.0
    back = rs.square_to_rect_resampler(400, nx, ny, lx, ly, model.device)
    pb = fine.problem(400.0, nx, ny, lx, ly, 0.002, "UPWIND", None, None, bfs={"step_height": 1.0, "h": 2.0, "Ub": 1.0})
    coarse_mod = importlib.import_module("sr-for-cfd_amd.coarse")
    types, values = pipeline.bc_arrays(coarse_mod.BFS_RUN_COARSE_DEFAULT)
    prof = pipeline.bfs_inlet_profiles(ny, ly / ny, 1.0, 2.0, 1.0)
    host = model.predict_into_solver_state(x, types, values, left_profiles=prof, resampler=back, in_affine=ain, out_affine=aout,
                                           nan_guard=True)
    s = fine.FineSolver(pb)
    s.init_from_prediction(model, x, ain, aout, back)
    dev = s.Var
    np.testing.assert_array_equal(dev, host)
    t = fine.FineSolver(pb)
    t.init(host)
    np.testing.assert_array_equal(_bits(t.Var), _bits(dev))


def test_resume_and_determinism_at_400(fine, coarse):
    pb = fine.problem(1000.0, 400, 400, bc=coarse.LDC_DOUBLE_LID)
    a = fine.FineSolver(pb)
    a.run(3)
    a.run(2)
    b = fine.FineSolver(pb)
    assert b.run(5) == 5
    c = fine.FineSolver(pb)
    c.run(5)
    np.testing.assert_array_equal(_bits(a.Var), _bits(b.Var))
    np.testing.assert_array_equal(_bits(b.Var), _bits(c.Var))
    np.testing.assert_array_equal(_bits(a.rms), _bits(b.rms))
    cnt = b.counters()
    sweeps = cnt["momentum_sweeps"] + cnt["pressure_sweeps"]
    # no host synchronisation per sweep: a few per outer iteration (one per inner-solve chunk + one at its end)
    assert cnt["host_syncs"] <= 6 * 5 + 1, cnt
    assert sweeps >= 50 * cnt["host_syncs"], cnt


def test_drop_ins(srcfd, fine, coarse, tmp_path):
    s, it, t = fine.run_normal_simulation(1000.0, 400, 400, max_iterations=3, output_name=str(tmp_path / "cavity"), bc=coarse.LDC_DOUBLE_LID)
    assert it == 3 and t > 0 and s.Var.shape == (3, 402, 402)
    back = srcfd.read_coarse_fields(str(tmp_path / "cavity_normal.h5"))
    np.testing.assert_array_equal(back["u"], s.Var[0, 1:-1, 1:-1].T)
    # the reference's extract_centerlines (PyCFD_ML_accelerated.py:1236-1271) reads only solver.Var
    u_field = s.Var[0, 1:-1, 1:-1].T.copy()
    assert u_field[:, 400 // 2].shape == (400,) and s.mesh.lx == 1.0 and s.mesh.ly == 1.0
    # residual_history every 100 iterations
    s, it, _ = fine.run_normal_simulation(100.0, 12, 12, convergence_criteria={"u": 0.0, "v": 0.0, "p": 0.0}, max_iterations=250,
                                          output_name=None)
    assert it == 250 and [len(s.residual_history[c]) for c in "uvp"] == [2, 2, 2]
    # huge tolerances: one iteration
    s, it, _ = fine.run_normal_simulation(100.0, 12, 12, convergence_criteria={"u": 1e9, "v": 1e9, "p": 1e9}, output_name=None)
    assert it == 1
    # a NaN initial field is the reference's ValueError
    nan = {c: np.full((12, 12), np.nan) for c in "uvp"}
    with pytest.raises(ValueError, match="Solver failed: NaN/Inf in residuals"):
        fine.run_fine_simulation_with_ml_init(100.0, 12, 12, nan, output_name=None)
    # BFS defaults (dt 0.002, UPWIND, lx 10, ly 3)
    s, it, _ = fine.run_bfs_normal_simulation(400.0, 40, 20, max_iterations=2, output_name=None)
    assert it == 2 and s.mesh.lx == 10.0 and s.mesh.ly == 3.0 and s.problem.scheme == 1 and s.problem.dt == 0.002


def test_ml_accelerated_drop_in_equals_the_solver_path(srcfd, fine, coarse, dec_weights, tmp_path):
    pipeline = importlib.import_module("sr-for-cfd_amd.pipeline")
    dec = str(tmp_path / "vanilla_decoder400_from_10_synthetic.h5")
    srcfd.SRModel.from_weights(None, dec_weights, device=-1).save_h5(None, dec)
    cf = srcfd.read_coarse_fields(os.path.join(GOLDEN, "coarse_ldc_Re800_double_lid.h5"))
    s, it, _ = fine.run_ml_accelerated_fine_simulation(cf, 800.0, 400, 400, max_iterations_fine=2, output_name=str(tmp_path / "acc"),
                                                       stats_file=STATS_TXT, encoder_file=ENCODER_H5, decoder_file=dec, bc=coarse.LDC_DOUBLE_LID)
    assert it == 2 and (tmp_path / "acc_accelerated.h5").exists()
    hr = pipeline.ml_super_resolution(cf, 10, 400, STATS_TXT, ENCODER_H5, dec)
    r, it2, _ = fine.run_fine_simulation_with_ml_init(800.0, 400, 400, hr, max_iterations=2, output_name=None, bc=coarse.LDC_DOUBLE_LID)
    assert it2 == 2
    np.testing.assert_array_equal(_bits(s.Var), _bits(r.Var))
