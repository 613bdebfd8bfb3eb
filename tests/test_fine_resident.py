"""What the resident mode of the fine-mesh solver (csrc/fine_solver.hip resident_kernel) has that needs no GPU: the entry points,
the host-only mesh rule, the `resident=` keyword down to the generator, and the kernel's reduction loops, restated in numpy lane
for lane, against the specification's 256-slot trees (tests/fine_solver_spec.py) bit for bit."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import fine_solver_spec as spec

MAX = 64      # srcfd_fine_resident_supported's bound
ENTRIES = {"srcfd_fine_resident_supported": ["int nx", "int ny"],
           "srcfd_fine_batch_set_mode": ["srcfd_fine_batch* b", "int mode"],
           "srcfd_fine_solver_set_mode": ["srcfd_fine_solver* s", "int mode"]}


@pytest.fixture(scope="module")
def L(srcfd):
    return importlib.import_module("sr-for-cfd_amd._lib")


@pytest.fixture(scope="module")
def fine(srcfd):
    return importlib.import_module("sr-for-cfd_amd.fine")


@pytest.fixture(scope="module")
def largest(L):
    """The supported maximum, asked of the library: the reductions below are checked up to it."""
    n = max(n for n in range(3, 1025) if L.lib.srcfd_fine_resident_supported(n, n))
    assert n == MAX and not any(L.lib.srcfd_fine_resident_supported(m, 3) or L.lib.srcfd_fine_resident_supported(3, m) for m in range(n + 1, 1025))
    return n


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entry_point_is_declared_exported_and_bound(L, entry):
    text = open(os.path.join(ROOT, "include", "srcfd.h")).read()
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{entry} is not declared in include/srcfd.h"
    assert [p.strip() for p in m.group(1).split(",")] == ENTRIES[entry]
    assert hasattr(L.lib, entry), f"{entry} is not exported"
    assert entry in L.EXPORTED
    fn = getattr(L.lib, entry)
    assert fn.restype is C.c_int and len(fn.argtypes) == 2 and fn.argtypes[1] is C.c_int
    assert re.search(r"#define\s+SRCFD_FINE_MODE_LAUNCHES\s+0\b", text) and re.search(r"#define\s+SRCFD_FINE_MODE_RESIDENT\s+1\b", text)
    assert (L.FINE_MODE_LAUNCHES, L.FINE_MODE_RESIDENT) == (0, 1)


def test_the_mesh_rule_needs_no_device(L, fine):
    for nx, ny in ((3, 3), (10, 10), (64, 64), (64, 3), (3, 64), (MAX, MAX), (MAX, 3)):
        assert L.lib.srcfd_fine_resident_supported(nx, ny) == 1 and fine.resident_supported(nx, ny) is True
    for nx, ny in ((400, 400), (MAX + 1, MAX), (MAX, MAX + 1), (2, 10), (10, 2), (0, 10), (10, 0), (-3, 10), (10, -3), (-1, -1)):
        assert L.lib.srcfd_fine_resident_supported(nx, ny) == 0 and fine.resident_supported(nx, ny) is False
    # every valid mesh up to 64 x 64
    assert all(L.lib.srcfd_fine_resident_supported(nx, ny) == 1 for nx in range(3, 65) for ny in range(3, 65))


def test_null_handles_are_refused(L):
    for entry in ("srcfd_fine_batch_set_mode", "srcfd_fine_solver_set_mode"):
        for mode in (0, 1):
            with pytest.raises(ValueError, match=entry + ": bad arguments"):
                L.check(getattr(L.lib, entry)(None, mode))


def test_the_keyword_exists_and_defaults_to_the_launch_mode(fine):
    datasets = importlib.import_module("sr-for-cfd_amd.datasets")
    for fn in (fine.FineSolver.__init__, fine.FineSolverBatch.__init__, fine.run_normal_simulations, fine.run_bfs_normal_simulations,
               fine.run_ml_accelerated_fine_simulations, fine.compare_ml_and_normal_simulations,
               fine.run_bfs_ml_accelerated_fine_simulations, fine.compare_bfs_ml_and_normal_simulations,
               datasets.generate_simulation_file):
        assert inspect.signature(fn).parameters["resident"].default is False, fn.__qualname__
    assert callable(fine.FineSolver.set_resident) and callable(fine.FineSolverBatch.set_resident)
    # the coarse sweeps keep the arguments and defaults of the host functions, then max_batch and device
    coarse = importlib.import_module("sr-for-cfd_amd.coarse")
    for many, one in ((fine.run_coarse_simulations, coarse.run_coarse_simulation), (fine.run_bfs_coarse_simulations, coarse.run_bfs_coarse_simulation)):
        a, b = inspect.signature(many).parameters, inspect.signature(one).parameters
        assert list(a) == ["reynolds"] + list(b)[1:] + ["max_batch", "device"]
        assert all(a[k].default == b[k].default for k in list(b)[1:])
        assert a["max_batch"].default == 64 and a["device"].default == 0
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="resident must be"):
            fine._resident_mode(bad, 10, 10)
    assert [fine._resident_mode(r, n, n) for r, n in ((False, 10), (True, 10), ("auto", 10), ("auto", 400), (True, 400))] == [0, 1, 1, 0, 1]


def test_the_generator_hands_the_keyword_to_the_solve(srcfd, tmp_path):
    datasets = importlib.import_module("sr-for-cfd_amd.datasets")
    calls = []

    def stub(reynolds, nx, ny, **kw):
        calls.append((nx, dict(kw)))
        return [({c: np.full((ny, nx), float(Re)) for c in "uvp"}, 7, 1) for Re in reynolds]

    for resident in ("auto", True):
        calls.clear()
        rec = datasets.generate_simulation_file(str(tmp_path / f"{resident}.h5"), reynolds_numbers=[100, 200], mesh_sizes=(4, 5), max_batch=8,
                                                resident=resident, solve=stub)
        assert rec == [(100, 4, 7, 1), (200, 4, 7, 1), (100, 5, 7, 1), (200, 5, 7, 1)]
        assert [n for n, _ in calls] == [4, 5] and all(kw["resident"] is resident and kw["max_batch"] == 8 for _, kw in calls)
    # the default leaves a solve of the old signature as it was
    calls.clear()
    datasets.generate_simulation_file(str(tmp_path / "default.h5"), reynolds_numbers=[100], mesh_sizes=(4,), solve=stub)
    assert "resident" not in calls[0][1]


# ---------------------------------------------------------------------------------------------- the kernel's reductions, in numpy
def _shfl_down(v, s):
    """__shfl_down(v, s, 64): lane l reads lane l + s, a lane past the end its own value."""
    out = v.copy()
    out[:64 - s] = v[s:]
    return out


def _res_tree(v, w):
    """res_tree: v[t] += v[t + s] for s = w/2 .. 1 in every lane at once; lane 0 of each aligned group of w lanes is the result."""
    s = w >> 1
    while s > 0:
        v = v + _shfl_down(v, s)
        s >>= 1
    return v


def _res_lanes(elements):
    w = 1
    while w < elements:
        w <<= 1
    w = 64 if elements > 32 else w
    return w, 64 // w


def _row_sums(vals, n_waves):
    """res_row_pass for one summand: vals (nx, ny) -> the nx row partials, rows dealt to `n_waves` waves."""
    nx, ny = vals.shape
    w, rows = _res_lanes(ny)
    out = np.full(nx, np.nan)
    lane = np.arange(64)
    seg, t = lane // w, lane % w
    for wave in range(n_waves):
        for r0 in range(wave * rows, nx, n_waves * rows):
            a = np.zeros(64)
            for l in range(64):
                i = r0 + seg[l]
                if i < nx:
                    if t[l] < ny:
                        a[l] = vals[i, t[l]]
            a = _res_tree(a, w)
            for l in range(64):
                if t[l] == 0 and r0 + seg[l] < nx:
                    out[r0 + seg[l]] = a[l]
    return out


def _colour_sums(vals, colour, n_waves):
    """The pressure half sweep's partials: vals (nx, ny) holds R^2 of every cell; row i (1-based), colour c takes j = j0, j0 + 2, ..."""
    nx, ny = vals.shape
    w, rows = _res_lanes((ny + 1) // 2)
    out = np.full(nx, np.nan)
    lane = np.arange(64)
    seg, t = lane // w, lane % w
    for wave in range(n_waves):
        for r0 in range(wave * rows, nx, n_waves * rows):
            a = np.zeros(64)
            for l in range(64):
                i = r0 + seg[l] + 1
                j = (1 if ((i + 1) & 1) == colour else 2) + 2 * t[l]
                if i <= nx and j <= ny:
                    a[l] = vals[i - 1, j - 1]
            a = _res_tree(a, w)
            for l in range(64):
                if t[l] == 0 and r0 + seg[l] < nx:
                    out[r0 + seg[l]] = a[l]
    return out


def _res_sum256(p):
    n = len(p)
    lane = np.arange(64)
    a = [np.where(lane + o < n, np.append(p, np.zeros(256))[lane + o], 0.0) for o in (0, 64, 128, 192)]
    return _res_tree((a[0] + a[2]) + (a[1] + a[3]), 64)[0]


def _summands(rng, shape):
    """Non-negative float64 over the whole exponent range, with exact zeros and subnormals mixed in."""
    v = rng.random(shape) * 10.0 ** rng.uniform(-300, 300, shape)
    kind = rng.integers(0, 6, shape)
    v = np.where(kind == 0, 0.0, v)
    v = np.where(kind == 1, rng.integers(1, 1 << 40, shape) * 5e-324, v)
    return v * 10.0 ** -rng.integers(0, 4) ** 4       # some arrays wholly small, so that sums stay near the subnormals


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_row_trees_equal_the_specification_for_every_row_length(largest):
    rng = np.random.default_rng(20)
    with np.errstate(over="ignore"):
        for ny in range(1, largest + 1):
            vals = _summands(rng, (7, ny))
            want = spec._sum256(vals)
            for n_waves in (1, 3, 8):
                np.testing.assert_array_equal(_bits(_row_sums(vals, n_waves)), _bits(want), err_msg=f"row length {ny}, {n_waves} waves")


def test_colour_trees_equal_the_specification_for_every_row_length(largest):
    rng = np.random.default_rng(21)
    with np.errstate(over="ignore"):
        for ny in range(1, largest + 1):
            nx = 4 + ny % 3
            sp = spec.Spec(nx, ny, 1.0, 1.0, 100.0, 1.0, 0.01, "UPWIND", [1e-6] * 3, np.zeros((3, 4), int), np.zeros((3, 4)))
            vals = _summands(rng, (nx, ny))
            for colour in (0, 1):
                want = sp._colour_partials(vals, colour)
                for n_waves in (1, 2, 8):
                    np.testing.assert_array_equal(_bits(_colour_sums(vals, colour, n_waves)), _bits(want),
                                                  err_msg=f"{nx} x {ny}, colour {colour}, {n_waves} waves")


def test_the_partial_tree_equals_the_specification_for_every_count(largest):
    rng = np.random.default_rng(22)
    with np.errstate(over="ignore"):
        for n in range(1, 2 * largest + 1):
            p = _summands(rng, (n,))
            np.testing.assert_array_equal(_bits(_res_sum256(p)), _bits(spec._sum256(p[None, :])[0]), err_msg=f"{n} partials")
