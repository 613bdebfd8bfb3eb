"""CPU tests of the device scorer's summation plan (csrc/score_plan.cpp, srcfd_score_plan) and of its surface: the order of float32
additions the kernel takes from the plan is numpy's, for every path of numpy's pairwise sum and for the family's field sizes.
No tolerance anywhere: float32 bit patterns."""
import ctypes as C
import importlib
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import score_ref as sr
from conftest import ROOT


def _L():
    return importlib.import_module("sr-for-cfd_amd._lib")


def _score():
    return importlib.import_module("sr-for-cfd_amd.score")


def _arrays(n):
    """Mixed-sign data of very different magnitudes (the order of additions shows), positive data (what |d| and d^2 are), and a
    standardised-field-like one."""
    rng = np.random.default_rng(n)
    return [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32),
            np.abs(rng.standard_normal(n)).astype(np.float32),
            (rng.standard_normal(n) * 0.37 + 0.11).astype(np.float32)]


def _bits(v):
    return np.float32(v).view(np.uint32)


def test_numpy_reduces_in_buffers_of_8192():
    assert np.getbufsize() == sr.CHUNK


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_restatement_equals_numpy_sum(n):
    """Guards tests/score_ref.py against the installed numpy: if this fails, numpy's order changed and the kernel's must follow."""
    assert np.getbufsize() == sr.CHUNK
    for a in _arrays(n):
        assert _bits(sr.numpy_sum_restated(a)) == _bits(np.sum(a)), n
        assert _bits(np.float32(sr.numpy_sum_restated(a) / np.float32(n))) == _bits(np.mean(a)), n


def test_one_tree_over_the_field_is_not_numpy():
    """Why the plan has chunks: a single pairwise tree over 8193 and more elements gives other bits on some arrays."""
    differ = 0
    for seed in range(20):
        a = (np.random.default_rng(seed).standard_normal(8193 + seed) * 100).astype(np.float32)
        differ += _bits(sr.pairwise(a)) != _bits(np.sum(a))
    assert differ > 0


@pytest.mark.parametrize("n", sr.LENGTHS)
def test_plan_tables_sum_like_numpy(srcfd, n):
    plan = _score().score_plan(n)
    assert plan["elems"] == n and plan["chunk"] == sr.CHUNK and plan["n_chunks"] == -(-n // sr.CHUNK)
    assert (plan["full"] is not None) == (n >= sr.CHUNK) and (plan["last"] is not None) == (n % sr.CHUNK != 0)
    for table in (plan["full"], plan["last"]):
        if table is None:
            continue
        leaves, nodes = table["leaves"], table["nodes"]
        assert len(leaves) <= 127 and len(nodes) == len(leaves) - 1 and all(1 <= ln <= sr.LEAF for _, ln in leaves)
        assert max([h for _, _, h in nodes], default=0) <= 7
        for i, (left, right, h) in enumerate(nodes):        # children first, heights consistent
            assert left < len(leaves) + i and right < len(leaves) + i
            hc = [0 if c < len(leaves) else nodes[c - len(leaves)][2] for c in (left, right)]
            assert h == max(hc) + 1
    for a in _arrays(n):
        assert _bits(sr.plan_sum(plan, a)) == _bits(np.sum(a)), n


def test_plan_of_the_notebook_field():
    plan = _score().score_plan(160_000)
    assert plan["n_chunks"] == 20
    assert [ln for _, ln in plan["full"]["leaves"]] == [128] * 64
    assert [ln for _, ln in plan["last"]["leaves"]] == [64, 72] * 32       # 4352 halves evenly down to 136, which splits 64 + 72 (n2 -= n2 % 8)
    unbalanced = _score().score_plan(257)["last"]
    assert [ln for _, ln in unbalanced["leaves"]] == [128, 64, 65]
    assert unbalanced["nodes"] == [[1, 2, 1], [0, 3, 2]]


@pytest.mark.parametrize("elems", [0, -1, -160_000, 2_560_001, 1 << 40])
def test_unsupported_sizes_are_refused_with_a_message(srcfd, elems):
    L = _L()
    buf = C.create_string_buffer(1 << 15)
    assert L.lib.srcfd_score_plan(elems, buf, len(buf)) == L.EINVAL
    msg = L.last_error()
    assert "srcfd_score_plan" in msg and "2560000" in msg, msg
    with pytest.raises(ValueError, match="2560000"):
        _score().score_plan(elems)
    # the host-pointer entry refuses the size before it looks for a device
    z = np.zeros(1, np.float32)
    m = np.zeros(8, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.lib.srcfd_score_fields(0, p(z), p(z), 1, elems, None, None, p(m)) == L.EINVAL
    assert "srcfd_score_fields" in L.last_error()


def test_largest_field_and_small_buffer(srcfd):
    L = _L()
    plan = _score().score_plan(2_560_000)
    assert plan["n_chunks"] == 313 and plan["last"] is not None
    small = C.create_string_buffer(16)
    assert L.lib.srcfd_score_plan(160_000, small, len(small)) == L.EINVAL and "buffer too small" in L.last_error()


def test_symbols_are_declared_exported_and_bound(srcfd):
    L = _L()
    header = open(os.path.join(ROOT, "include", "srcfd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(L.LIB_PATH)
    for name in ("srcfd_score_plan", "srcfd_score_fields", "srcfd_evalset_create", "srcfd_evalset_score", "srcfd_evalset_destroy"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert hasattr(lib, name), name
        assert name in L.EXPORTED and getattr(L.lib, name).argtypes is not None, name
    assert "#define SRCFD_SCORE_FIELDS 8" in code and L.SCORE_FIELDS == 8 and L.SCORE_NAMES == sr.NAMES
    for k, name in enumerate(sr.NAMES):
        assert re.search(r"#define SRCFD_SCORE_%s %d\b" % (name.upper(), k), code), name
    # no scoring entry point takes a stream
    for m in re.finditer(r"\bint (srcfd_(?:score|evalset)_\w+)\s*\(([^;]*)\);", code):
        assert "stream" not in m.group(2), m.group(1)
    assert srcfd.EvalSet is _score().EvalSet and srcfd.score_fields is _score().score_fields
    assert {"EvalSet", "score_fields"} <= set(srcfd.__all__)
    assert callable(importlib.import_module("sr-for-cfd_amd.datasets").evalset_from_split)


def test_fit_validation_defaults_to_off():
    train = importlib.import_module("sr-for-cfd_amd.train")
    params = inspect.signature(train.fit).parameters
    assert params["validation"].default is None and params["validation_every"].default == 1
    main = importlib.import_module("sr-for-cfd_amd.train_main")
    assert "--validate-every" in inspect.getsource(main.main) and "evaluate_for_re" in dir(main)


def test_nmae_formula_is_train_mains(srcfd):
    """`EvalSet.score`'s nmae_percent from (mae, truth_min, truth_max) against evaluate_for_re's expression on the arrays."""
    rng = np.random.default_rng(5)
    t = (rng.standard_normal((4, 50, 50)) * 3 + 1).astype(np.float32)
    p = t + (rng.standard_normal(t.shape) * 0.1).astype(np.float32)
    m = sr.notebook_metrics(p, t)
    got = _score().nmae_percent(m["mae"], m["truth_min"], m["truth_max"])
    for i in range(4):
        mae = float(np.mean(np.abs(t[i] - p[i])))
        rng_ = float(np.max(t[i]) - np.min(t[i]))
        assert got[i] == mae / (rng_ + 1e-8) * 100
    assert _score().nmae_percent(np.float32([1.0]), np.float32([2.0]), np.float32([2.0]))[0] == 1.0 / 1e-8 * 100   # constant field


def test_plan_checker_builds_and_passes_under_the_sanitizers():
    """tools/score_plan_check.cpp + score_plan.cpp under AddressSanitizer + UBSan, on the CPU: every chunk length 1 .. 8192, every
    field size 1 .. 20 000 and the family's up to 1600 x 1600."""
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "sr-for-cfd_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "score_plan_check"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "sr-for-cfd_amd", "lib", "score_plan_check_asan")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert int(out.stdout.split()[0]) >= 8192 + 20_000


def test_evalset_from_split_selects_and_keeps_the_bookkeeping(srcfd, monkeypatch):
    """Host side of datasets.evalset_from_split with the device handle stubbed out: which samples, which affines."""
    ds = importlib.import_module("sr-for-cfd_amd.datasets")
    made = {}

    class Stub:
        def __init__(self, x_lr, x_hr, in_affine=None, pred_affine=None, truth_affine=None, device=0):
            made.update(x=x_lr, y=x_hr, ia=in_affine, pa=pred_affine, ta=truth_affine, device=device)

    monkeypatch.setattr(_score(), "EvalSet", Stub)
    n = 9
    data = dict(x_lr_test=np.arange(n * 4, dtype=np.float32).reshape(n, 2, 2, 1), x_hr_test=np.arange(n * 16, dtype=np.float32).reshape(n, 4, 4, 1),
                res_test=np.array([800, 800, 800, 900, 900, 900, 800, 800, 800]), comps_test=np.array(list("uvpuvpuvp")),
                stats_hr={"u": (0.1, 2.0), "v": (-0.2, 3.0), "p": (0.3, 0.5)})
    es = ds.evalset_from_split(data, reynolds=800, device=3)
    assert es.index.tolist() == [0, 1, 2, 6, 7, 8] and es.res_test.tolist() == [800] * 6 and "".join(es.comps_test) == "uvpuvp"
    assert made["ia"] is None and made["device"] == 3 and made["pa"] is made["ta"] and made["pa"].dtype == np.float32
    np.testing.assert_array_equal(made["pa"], np.float32([[0.1, 2.0], [-0.2, 3.0], [0.3, 0.5]] * 2))
    np.testing.assert_array_equal(made["x"], data["x_lr_test"][es.index])
    np.testing.assert_array_equal(made["y"], data["x_hr_test"][es.index])
    assert ds.evalset_from_split(data, device=0).index.tolist() == list(range(n))
    assert ds.evalset_from_split(data, reynolds=[900, 1000]).index.tolist() == [3, 4, 5]
