"""The batched SR hand-off (srcfd_fine_batch_init_from_prediction, fine.FineSolverBatch.init_from_prediction and the sweep drop-ins
on top of it): everything of it that needs no GPU -- the entry point in the header, the library and the ctypes table, and the
refusals the drop-ins raise before they touch a device.  Constructing a FineSolverBatch needs a device, so the method's own shape
refusals are in tests/test_gpu_fine_batch_handoff.py."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ENCODER_H5, ROOT, STATS_TXT

ENTRY = "srcfd_fine_batch_init_from_prediction"
SWEEPS = ("run_ml_accelerated_fine_simulations", "run_bfs_ml_accelerated_fine_simulations", "compare_ml_and_normal_simulations",
          "compare_bfs_ml_and_normal_simulations")


@pytest.fixture(scope="module")
def fine(srcfd):
    return importlib.import_module("sr-for-cfd_amd.fine")


def test_entry_point_is_declared_exported_and_bound(srcfd):
    L = importlib.import_module("sr-for-cfd_amd._lib")
    text = open(os.path.join(ROOT, "include", "srcfd.h")).read()
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{ENTRY} is not declared in include/srcfd.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 10
    assert params[0].startswith("srcfd_fine_batch*") and params[4] == "int n_warm" and params[5] == "const int* cases"
    assert hasattr(L.lib, ENTRY), f"{ENTRY} is not exported"
    assert ENTRY in L.EXPORTED
    fn = getattr(L.lib, ENTRY)
    assert fn.restype is C.c_int and len(fn.argtypes) == 10
    assert fn.argtypes[4] is C.c_int and fn.argtypes[5] == C.POINTER(C.c_int) and fn.argtypes[9] == C.POINTER(C.c_int64)


def test_null_handles_are_refused_without_a_device(srcfd):
    L = importlib.import_module("sr-for-cfd_amd._lib")
    x = np.zeros((3, 4, 4, 1), np.float32)
    bad = C.c_int64(0)
    with pytest.raises(ValueError, match=ENTRY + ": bad arguments"):
        L.check(getattr(L.lib, ENTRY)(None, None, None, x.ctypes.data_as(C.c_void_p), 1, None, None, None, 0, C.byref(bad)))


def test_class_method_and_sweep_functions_exist_with_the_single_case_keywords(fine):
    sig = inspect.signature(fine.FineSolverBatch.init_from_prediction)
    assert list(sig.parameters) == ["self", "model", "x", "in_affine", "out_affine", "resampler", "nan_guard", "cases"]
    assert sig.parameters["nan_guard"].default is True and sig.parameters["cases"].default is None
    for batched, single in (("run_ml_accelerated_fine_simulations", "run_ml_accelerated_fine_simulation"),
                            ("compare_ml_and_normal_simulations", "run_ml_accelerated_fine_simulation"),
                            ("run_bfs_ml_accelerated_fine_simulations", "run_bfs_ml_accelerated_fine_simulation"),
                            ("compare_bfs_ml_and_normal_simulations", "run_bfs_ml_accelerated_fine_simulation")):
        b = inspect.signature(getattr(fine, batched)).parameters
        s = inspect.signature(getattr(fine, single)).parameters
        assert list(b)[:4] == ["coarse_fields_list", "reynolds", "nx", "ny"]
        # the same keyword arguments with the same defaults, then max_batch and device
        assert list(b)[4:] == list(s)[4:] + ["max_batch", "device"], batched
        for name in list(s)[4:]:
            assert b[name].default == s[name].default, (batched, name)
        assert b["max_batch"].default == 8


def _coarse(n):
    return [{c: np.zeros((10, 10)) for c in "uvp"} for _ in range(n)]


@pytest.mark.parametrize("name", SWEEPS)
def test_missing_model_files_raise_up_front(fine, name, tmp_path):
    f = getattr(fine, name)
    missing = str(tmp_path / "nothing_here.h5")
    with pytest.raises(FileNotFoundError, match="Decoder model not found"):
        f(_coarse(2), [100.0, 200.0], 400, 400, stats_file=STATS_TXT, encoder_file=ENCODER_H5, decoder_file=missing)
    with pytest.raises(FileNotFoundError, match="Encoder model not found"):
        f(_coarse(2), [100.0, 200.0], 400, 400, stats_file=STATS_TXT, encoder_file=missing, decoder_file=missing)
    with pytest.raises(FileNotFoundError, match="Stats file not found"):
        f(_coarse(2), [100.0, 200.0], 400, 400)     # the default file names, which the test's directory does not hold


@pytest.mark.parametrize("name", SWEEPS)
def test_wrong_list_lengths_raise_value_error(fine, name):
    coarse = importlib.import_module("sr-for-cfd_amd.coarse")
    f = getattr(fine, name)
    with pytest.raises(ValueError, match="one per Reynolds number"):
        f(_coarse(2), [100.0, 200.0], 400, 400, stats_file=STATS_TXT, encoder_file=ENCODER_H5, decoder_file=ENCODER_H5,
          bc=[coarse.LDC_DOUBLE_LID] * 3)
    with pytest.raises(ValueError, match="one set of coarse fields per Reynolds number"):
        f(_coarse(3), [100.0, 200.0], 400, 400, stats_file=STATS_TXT, encoder_file=ENCODER_H5, decoder_file=ENCODER_H5)


def test_batched_preparation_stacks_the_single_case_recipe(srcfd, monkeypatch):
    """pipeline._prepare_batch is pipeline._prepare per field, stacked: the aspect-ratio matrices, the float32 cast and the
    adaptive blend are one shared function.  The model handle and the resampler need a device and are stubbed out."""
    pipeline = importlib.import_module("sr-for-cfd_amd.pipeline")
    kc = importlib.import_module("sr-for-cfd_amd.keras_compat")
    rs = importlib.import_module("sr-for-cfd_amd.resample")

    class _Handle:
        device = 0

    monkeypatch.setattr(kc, "_device_handle", lambda paths, precision, device=None: _Handle)
    monkeypatch.setattr(rs, "square_to_rect_resampler", lambda *a: "back")
    rng = np.random.default_rng(3)
    fields = [{c: rng.normal(size=(10, 10)) for c in "uvp"} for _ in range(3)]
    for aspect, adaptive in ((False, False), (True, True), (False, True)):
        args = (10, 400, STATS_TXT, ENCODER_H5, ENCODER_H5, aspect, 10.0, 3.0, adaptive, 0.3, None)
        model, x, ain, aout, back = pipeline._prepare_batch(fields, *args)
        assert model is _Handle and back == ("back" if aspect else None)
        assert x.shape == (9, 10, 10, 1) and x.dtype == np.float32 and ain.shape == aout.shape == (9, 2)
        for i, cf in enumerate(fields):
            _, x1, ain1, aout1, back1, _ = pipeline._prepare(cf, *args, pipeline._quiet)
            np.testing.assert_array_equal(x[3 * i:3 * i + 3].view(np.uint32), x1.view(np.uint32))
            np.testing.assert_array_equal(ain[3 * i:3 * i + 3].view(np.uint32), ain1.view(np.uint32))
            np.testing.assert_array_equal(aout[3 * i:3 * i + 3].view(np.uint32), aout1.view(np.uint32))
            assert back1 == back
