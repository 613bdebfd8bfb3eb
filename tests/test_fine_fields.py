"""Device fields in and out of the fine solver (srcfd_fine_batch_init_from_fields_device, srcfd_fine_batch_get_fields_device, their
single-case forms and srcfd_resample_device_f64; fine.FineSolverBatch.init_from_fields / fields_device and the sweeps on top of
them): everything that needs no GPU -- the interpolation matrices of the control arm against scipy, the entries in the header, the
library and the ctypes table, what they answer without a device, and the refusals the Python side raises before it calls the
library.  The kernels and the bits: tests/test_gpu_fine_fields.py."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ENCODER_H5, ROOT, STATS_TXT
from test_device_args import OnDevice

ENTRIES = {   # name -> (number of parameters, index of the dtype parameter or None)
    "srcfd_resample_device_f64": (5, None),
    "srcfd_fine_batch_init_from_fields_device": (7, 3),
    "srcfd_fine_batch_get_fields_device": (6, 4),
    "srcfd_fine_solver_init_from_fields_device": (5, 3),
    "srcfd_fine_solver_get_fields_device": (4, 2),
}


@pytest.fixture(scope="module")
def fine(srcfd):
    return importlib.import_module("sr-for-cfd_amd.fine")


@pytest.fixture(scope="module")
def L(srcfd):
    return importlib.import_module("sr-for-cfd_amd._lib")


# ---------------------------------------------------------------------------------------------- the control arm's matrices
@pytest.mark.parametrize("h,w,ny,nx", [(10, 10, 37, 29), (10, 7, 14, 9)])
def test_interpolation_matrices_are_scipys_bicubic_spline(fine, h, w, ny, nx):
    """Ry @ F @ Rx.T against RectBivariateSpline on the reference's nodes, at the bar tests/test_resample.py holds: 1e-12."""
    from scipy.interpolate import RectBivariateSpline
    lx, ly = 10.0, 3.0
    Ry, Rx = fine.interpolation_matrices(h, w, nx, ny, lx, ly)
    assert Ry.shape == (ny, h) and Rx.shape == (nx, w)
    F = np.random.default_rng(7).normal(size=(h, w))
    want = RectBivariateSpline(np.linspace(0, ly, h), np.linspace(0, lx, w), F, kx=3, ky=3)(np.linspace(0, ly, ny), np.linspace(0, lx, nx))
    got = Ry @ F @ Rx.T
    err = np.abs(got - want).max()
    print(f"({h}, {w}) -> ({ny}, {nx}): max |Ry F Rx^T - RectBivariateSpline| = {err:.3e}")
    assert err <= 1e-12
    # an interpolating spline: the coarse nodes that are fine nodes too keep their values (the end points always are)
    np.testing.assert_allclose(got[[0, 0, -1, -1], [0, -1, 0, -1]], F[[0, 0, -1, -1], [0, -1, 0, -1]], rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------- the ABI surface
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_is_declared_exported_and_bound(L, entry):
    n_params, _ = ENTRIES[entry]
    text = open(os.path.join(ROOT, "include", "srcfd.h")).read()
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{entry} is not declared in include/srcfd.h"
    assert len(m.group(1).split(",")) == n_params
    assert hasattr(L.lib, entry) and entry in L.EXPORTED
    fn = getattr(L.lib, entry)
    assert fn.restype is C.c_int and len(fn.argtypes) == n_params
    assert fn.argtypes[-1] is C.c_void_p            # the stream


def test_null_handles_are_refused_as_the_neighbouring_entries_refuse_them(L):
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)
    calls = {"srcfd_resample_device_f64": (None, p, 1, p, None),
             "srcfd_fine_batch_init_from_fields_device": (None, None, p, L.F64, 1, None, None),
             "srcfd_fine_batch_get_fields_device": (None, 1, None, p, L.F64, None),
             "srcfd_fine_solver_init_from_fields_device": (None, None, p, L.F64, None),
             "srcfd_fine_solver_get_fields_device": (None, p, L.F64, None)}
    assert set(calls) == set(ENTRIES)
    for entry, args in calls.items():
        with pytest.raises(ValueError, match=entry + ": bad arguments"):
            L.check(getattr(L.lib, entry)(*args))


def test_without_a_device_the_new_names_raise_no_device_error(srcfd, fine):
    """No handle exists without a device, so the new methods are out of reach and the sweeps fail where their neighbours do: at the
    first handle they create."""
    if srcfd.device_count() > 0:
        return                                      # with a device these calls compute: tests/test_gpu_fine_fields.py
    coarse = [{c: np.zeros((10, 10)) for c in "uvp"}]
    with pytest.raises(srcfd.NoDeviceError):
        fine.interpolation_resampler(10, 10, 20, 20)
    with pytest.raises(srcfd.NoDeviceError):
        fine.FineSolverBatch([fine.problem(100.0, 20, 20)])
    with pytest.raises(srcfd.NoDeviceError):
        fine.run_interpolated_fine_simulations(coarse, [100.0], 20, 20)
    with pytest.raises(srcfd.NoDeviceError):
        fine.run_bfs_interpolated_fine_simulations(coarse, [100.0], 20, 20)
    with pytest.raises(srcfd.NoDeviceError):
        fine.compare_warm_starts(coarse, [100.0], 20, 20)          # no model files: the "interp" and "zero" arms
    with pytest.raises(srcfd.NoDeviceError):
        fine.run_nested_simulations([100.0], [(12, 12), (24, 20)])


# ---------------------------------------------------------------------------------------------- signatures
def test_signatures(fine):
    for cls in (fine.FineSolverBatch, fine.FineSolver):
        assert callable(cls.init_from_fields) and callable(cls.fields_device)
    assert list(inspect.signature(fine.FineSolverBatch.init_from_fields).parameters) == ["self", "fields", "cases", "resampler", "stream"]
    assert list(inspect.signature(fine.FineSolverBatch.fields_device).parameters) == ["self", "cases", "dtype", "out", "stream"]
    assert list(inspect.signature(fine.interpolation_resampler).parameters) == ["lr_h", "lr_w", "nx", "ny", "lx", "ly", "device"]
    model_only = {"stats_file", "encoder_file", "decoder_file", "precision", "use_aspect_ratio_correction", "use_adaptive_normalization",
                  "blend_factor"}
    for interp, ml in (("run_interpolated_fine_simulations", "run_ml_accelerated_fine_simulations"),
                       ("run_bfs_interpolated_fine_simulations", "run_bfs_ml_accelerated_fine_simulations")):
        a, b = inspect.signature(getattr(fine, interp)).parameters, inspect.signature(getattr(fine, ml)).parameters
        assert list(a) == [n for n in b if n not in model_only], interp
        for n in a:
            if n != "device":                      # no model loader to choose one: device 0
                assert a[n].default == b[n].default, (interp, n)
    for cmp_, two in (("compare_warm_starts", "compare_ml_and_normal_simulations"), ("compare_bfs_warm_starts", "compare_bfs_ml_and_normal_simulations")):
        a, b = inspect.signature(getattr(fine, cmp_)).parameters, inspect.signature(getattr(fine, two)).parameters
        assert list(a) == list(b)[:4] + ["arms"] + list(b)[4:], cmp_
        assert tuple(a["arms"].default) == ("ml", "interp", "zero")
    assert list(inspect.signature(fine.run_nested_simulations).parameters)[:2] == ["reynolds", "meshes"]


# ---------------------------------------------------------------------------------------------- refusals before the library
class _Mesh:
    nx, ny = 8, 6


@pytest.fixture
def no_library_calls(L, monkeypatch):
    """Every new entry is replaced by a function that fails the test: the refusals below are raised before the library is reached."""
    def forbidden(*a):
        raise AssertionError("the library was called")
    for entry in ENTRIES:
        monkeypatch.setattr(L.lib, entry, forbidden)
    monkeypatch.setattr(L.lib, "srcfd_resample_device", forbidden)


def _handles(fine):
    """A batch of 4 cases, a solver and a resampler (6, 5) -> (6, 8) that own nothing: the argument checks read attributes only."""
    rs = importlib.import_module("sr-for-cfd_amd.resample")
    b = object.__new__(fine.FineSolverBatch)
    b.n_cases, b.device, b.mesh, b._h = 4, 0, _Mesh, None
    s = object.__new__(fine.FineSolver)
    s.device, s.mesh, s._h = 0, _Mesh, None
    r = object.__new__(rs.Resampler)
    r.in_h, r.in_w, r.out_h, r.out_w, r.device, r._h = 6, 5, 6, 8, 0, None
    return b, s, r


def _dev(*shape, dtype=torch.float64, index=0):
    return OnDevice(torch.zeros(shape, dtype=dtype), index)


def test_init_from_fields_refusals(fine, no_library_calls):
    b, s, r = _handles(fine)
    ok = _dev(6, 6, 8)
    cases = [
        (dict(fields=ok, cases=[1, 1]), "must not repeat a case"),
        (dict(fields=ok, cases=[0, 1, 2, 3, 0]), "between 1 and 4 cases"),
        (dict(fields=ok, cases=[]), "between 1 and 4 cases"),
        (dict(fields=_dev(7, 6, 8)), r"first dimension must be 3 \* n_warm = 6"),                     # not a multiple of three
        (dict(fields=ok, cases=[2]), r"first dimension must be 3 \* n_warm = 3"),                      # two fields, one case
        (dict(fields=_dev(15, 6, 8)), "between 1 and 4 warm cases"),                                  # five fields, four cases
        (dict(fields=_dev(6, 48)), r"must have shape \(3 \* n_warm, 6, 8\)"),
        (dict(fields=torch.zeros(6, 6, 8, dtype=torch.float64)), "fields must be a CUDA tensor"),
        (dict(fields=OnDevice(torch.zeros(6, 8, 6, dtype=torch.float64).transpose(1, 2))), "fields is not contiguous"),
        (dict(fields=OnDevice(torch.zeros(6, 6, 16, dtype=torch.float64)[:, :, ::2])), "fields is not contiguous"),
        (dict(fields=_dev(6, 8, 6)), r"fields has shape \(6, 8, 6\), expected \(6, 6, 8\)"),          # (nx, ny) for (ny, nx)
        (dict(fields=_dev(6, 6, 8, dtype=torch.float16)), "fields has dtype torch.float16"),
        (dict(fields=_dev(6, 6, 8, index=1)), "fields is on device cuda:1"),
        (dict(fields=np.zeros((6, 8, 6))), r"per-field shape \(8, 6\), expected \(6, 8\)"),            # numpy: refused before the upload
        (dict(fields=ok, resampler=r), r"fields has shape \(6, 6, 8\), expected \(6, 6, 5\)"),         # the resampler's input
    ]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            b.init_from_fields(**kw)
    off = object.__new__(type(r))
    off.in_h, off.in_w, off.out_h, off.out_w, off.device, off._h = 6, 5, 8, 6, 0, None
    with pytest.raises(ValueError, match=r"resampler ends at \(8, 6\), the mesh takes fields of \(6, 8\)"):
        b.init_from_fields(_dev(6, 6, 5), resampler=off)
    r.device = 1
    with pytest.raises(ValueError, match="resampler is on device cuda:1, the solver is on cuda:0"):
        b.init_from_fields(_dev(6, 6, 5), resampler=r)
    # the single case: one field
    for fields, text in ((ok, "between 1 and 1 warm cases"), (_dev(4, 6, 8), r"first dimension must be 3 \* n_warm = 3"),
                         (torch.zeros(3, 6, 8), "must be a CUDA tensor"),
                         (OnDevice(torch.zeros(3, 8, 6).transpose(1, 2)), "not contiguous")):
        with pytest.raises(ValueError, match=text):
            s.init_from_fields(fields)


def test_fields_device_refusals(fine, no_library_calls):
    b, s, _ = _handles(fine)
    for kw, text in ((dict(cases=[2, 2]), "must not repeat a case"),
                     (dict(cases=[0, 1, 2, 3, 1]), "between 1 and 4 cases"),
                     (dict(dtype=torch.float16, out=_dev(12, 6, 8)), "dtype must be torch.float64 or torch.float32"),
                     (dict(out=torch.zeros(12, 6, 8, dtype=torch.float64)), "out must be a CUDA tensor"),
                     (dict(out=_dev(12, 6, 8, dtype=torch.float32)), "out has dtype torch.float32, expected torch.float64"),
                     (dict(out=_dev(6, 6, 8)), r"out has shape \(6, 6, 8\), expected \(12, 6, 8\)"),
                     (dict(out=_dev(12, 6, 8), cases=[3, 0]), r"out has shape \(12, 6, 8\), expected \(6, 6, 8\)"),
                     (dict(out=OnDevice(torch.zeros(12, 8, 6, dtype=torch.float64).transpose(1, 2))), "out is not contiguous")):
        with pytest.raises(ValueError, match=text):
            b.fields_device(**kw)
    with pytest.raises(ValueError, match=r"out has shape \(6, 6, 8\), expected \(3, 6, 8\)"):
        s.fields_device(out=_dev(6, 6, 8))


def test_resampler_apply_device_f64_takes_float64_and_apply_device_still_float32_only(fine, no_library_calls):
    _, _, r = _handles(fine)
    for x, text in ((_dev(2, 6, 5, dtype=torch.float32), "x has dtype torch.float32, expected torch.float64"),
                    (torch.zeros(2, 6, 5, dtype=torch.float64), "x must be a CUDA tensor"),
                    (OnDevice(torch.zeros(2, 5, 6, dtype=torch.float64).transpose(1, 2)), "x is not contiguous"),
                    (_dev(2, 6, 6), r"x has per-sample shape \(6, 6\), expected \(6, 5\)")):
        with pytest.raises(ValueError, match=text):
            r.apply_device_f64(x, out=_dev(2, 6, 8))
    with pytest.raises(ValueError, match="out has dtype torch.float32, expected torch.float64"):
        r.apply_device_f64(_dev(2, 6, 5), out=_dev(2, 6, 8, dtype=torch.float32))
    with pytest.raises(ValueError, match="x has dtype torch.float64, expected torch.float32"):       # the existing call keeps its contract
        r.apply_device(_dev(2, 6, 5), out=_dev(2, 6, 8))
    # good arguments pass the checks and reach the library: float64 the new entry, float32 the old one
    for method, dtype in ((r.apply_device_f64, torch.float64), (r.apply_device, torch.float32)):
        with pytest.raises(AssertionError, match="the library was called"):
            method(_dev(2, 6, 5, dtype=dtype), out=_dev(2, 6, 8), stream=0)


def test_sweep_refusals_come_before_any_handle(fine, tmp_path):
    coarse = [{c: np.zeros((10, 10)) for c in "uvp"} for _ in range(2)]
    missing = str(tmp_path / "nothing_here.h5")
    for f in (fine.compare_warm_starts, fine.compare_bfs_warm_starts):
        with pytest.raises(ValueError, match="arms must be distinct names"):
            f(coarse, [100.0, 200.0], 20, 20, arms=("interp", "interp"))
        with pytest.raises(ValueError, match="arms must be distinct names"):
            f(coarse, [100.0, 200.0], 20, 20, arms=("zero", "warm"))
        with pytest.raises(ValueError, match="one set of coarse fields per Reynolds number"):
            f(coarse, [100.0], 20, 20)
        with pytest.raises(ValueError, match="the 'ml' arm needs"):
            f(coarse, [100.0, 200.0], 20, 20, arms=("ml",))
        with pytest.raises(FileNotFoundError, match="Decoder model not found"):      # some files given: all three must exist
            f(coarse, [100.0, 200.0], 20, 20, stats_file=STATS_TXT, encoder_file=ENCODER_H5, decoder_file=missing)
        with pytest.raises(ValueError, match="max_batch must be at least 2"):
            f(coarse, [100.0, 200.0], 20, 20, arms=("interp", "zero"), max_batch=1)
    for f in (fine.run_interpolated_fine_simulations, fine.run_bfs_interpolated_fine_simulations):
        with pytest.raises(ValueError, match="one set of coarse fields per Reynolds number"):
            f(coarse, [100.0], 20, 20)
    with pytest.raises(ValueError, match="at least one"):
        fine.run_nested_simulations([100.0], [])
    with pytest.raises(ValueError, match="one cap or one per level"):
        fine.run_nested_simulations([100.0], [(12, 12), (24, 20)], max_iterations=[5, 5, 5])
