"""The training-set generator's file logic (datasets.generate_simulation_file with an injected solver), append_solution's
unchanged default output, and the batched fine-mesh solver's footprint -- everything of the batch feature that needs no GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def datasets(srcfd):
    return importlib.import_module("sr-for-cfd_amd.datasets")


@pytest.fixture(scope="module")
def h5(srcfd):
    return importlib.import_module("sr-for-cfd_amd.h5")


def _field(Re, n, k):
    """A recognisable (ny, nx) field: the value says which Re, component, row and column it is."""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return Re + 0.1 * k + 1e-3 * y + 1e-6 * x


class _Stub:
    """A `run_normal_simulations` that records its calls; status per Re from `status` (default converged)."""

    def __init__(self, status=None):
        self.calls = []
        self.status = status or {}

    def __call__(self, reynolds, nx, ny, dt=0.001, scheme="QUICK", convergence_criteria=None, max_iterations=100000, bc=None,
                 max_batch=8, device=0):
        self.calls.append(dict(reynolds=list(reynolds), nx=nx, ny=ny, dt=dt, scheme=scheme, cc=convergence_criteria,
                               max_iterations=max_iterations, bc=bc, max_batch=max_batch, device=device))
        return [({c: _field(Re, nx, k) for k, c in enumerate("uvp")}, 10 * Re + nx, self.status.get(Re, 1)) for Re in reynolds]


def test_generator_writes_the_notebook_schema(datasets, h5, tmp_path):
    path = str(tmp_path / "simulation_result_double_lid.h5")
    stub = _Stub()
    rec = datasets.generate_simulation_file(path, reynolds_numbers=[100, 200, 300], mesh_sizes=(4, 7), dt=0.01, max_iterations=1234,
                                            convergence_criteria={"u": 1e-3}, max_batch=2, device=0, solve=stub)
    assert rec == [(Re, n, 10 * Re + n, 1) for n in (4, 7) for Re in (100, 200, 300)]
    # batches are cut at max_batch per mesh size, and the solve's arguments are passed on
    assert [(c["nx"], c["ny"], c["reynolds"]) for c in stub.calls] == [(4, 4, [100, 200]), (4, 4, [300]), (7, 7, [100, 200]), (7, 7, [300])]
    for c in stub.calls:
        assert c["dt"] == 0.01 and c["scheme"] == "QUICK" and c["max_iterations"] == 1234 and c["cc"] == {"u": 1e-3}
        assert c["bc"] is importlib.import_module("sr-for-cfd_amd.coarse").LDC_DOUBLE_LID and c["max_batch"] == 2
    with h5.H5File(path) as f:
        assert sorted(f.keys("/")) == sorted(f"Re{Re}_mesh{n}x{n}" for n in (4, 7) for Re in (100, 200, 300))
        for n in (4, 7):
            X, Y = np.meshgrid(np.linspace(0, 1.0, n), np.linspace(0, 1.0, n))
            for Re in (100, 200, 300):
                g = f"Re{Re}_mesh{n}x{n}"
                assert sorted(f.attr_names(g)) == ["bc_type", "case_name", "nx", "ny", "reynolds_number", "total_points"]
                assert f.attr_str(g, "bc_type") == ["double_lid(u_top=1,u_bottom=1)"]
                assert f.attr_str(g, "case_name") == ["double lid driven cavity"]
                assert f.attr_num(g, "reynolds_number")[0] == Re
                assert [f.attr_num(g, a)[0] for a in ("nx", "ny", "total_points")] == [n, n, n * n]
                assert sorted(f.keys(g)) == ["p", "u", "v", "x", "y"]
                np.testing.assert_array_equal(f.read(f"{g}/x"), X.flatten())
                np.testing.assert_array_equal(f.read(f"{g}/y"), Y.flatten())
                for k, c in enumerate("uvp"):
                    d = f.read(f"{g}/{c}")
                    assert d.dtype == np.float64 and d.shape == (n * n,)
                    np.testing.assert_array_equal(d.reshape(n, n), _field(Re, n, k))      # row-major (ny, nx)
    x_lr, x_hr, res, comps, bcs = datasets.load_paired_reynolds_multi([path], 4, 7)
    assert x_lr.shape == (9, 4, 4, 1) and x_hr.shape == (9, 7, 7, 1) and set(bcs) == {"double_lid(u_top=1,u_bottom=1)"}
    np.testing.assert_array_equal(x_hr[1, ..., 0], _field(100, 7, 1).astype(np.float32))


def test_generator_skips_diverged_writes_capped_and_keeps_earlier_groups(datasets, h5, tmp_path):
    path = str(tmp_path / "sweep.h5")
    # Re 200 diverges (status 2); Re 300 only reaches max_iterations (status 0): written, like the notebook's
    rec = datasets.generate_simulation_file(path, reynolds_numbers=[100, 200, 300], mesh_sizes=(5,), max_batch=8,
                                            solve=_Stub({200: 2, 300: 0}))
    assert rec == [(100, 5, 1005, 1), (200, 5, 2005, 2), (300, 5, 3005, 0)]
    with h5.H5File(path) as f:
        assert sorted(f.keys("/")) == ["Re100_mesh5x5", "Re300_mesh5x5"]
    # a second call for the same path with other Re keeps the earlier groups, attributes and values (the notebook appends)
    before = {}
    with h5.H5File(path) as f:
        for g in f.keys("/"):
            before[g] = ({a: (f.attr_str(g, a) if a in ("bc_type", "case_name") else f.attr_num(g, a).tolist()) for a in f.attr_names(g)},
                         {d: f.read(f"{g}/{d}") for d in f.keys(g)})
    rec = datasets.generate_simulation_file(path, reynolds_numbers=[150], mesh_sizes=(5, 6), bc_type="other", solve=_Stub())
    assert rec == [(150, 5, 1505, 1), (150, 6, 1506, 1)]
    with h5.H5File(path) as f:
        assert sorted(f.keys("/")) == ["Re100_mesh5x5", "Re150_mesh5x5", "Re150_mesh6x6", "Re300_mesh5x5"]
        assert f.attr_str("Re150_mesh6x6", "bc_type") == ["other"]
        for g, (attrs, data) in before.items():
            assert {a: (f.attr_str(g, a) if a in ("bc_type", "case_name") else f.attr_num(g, a).tolist()) for a in f.attr_names(g)} == attrs
            for d, v in data.items():
                got = f.read(f"{g}/{d}")
                assert got.dtype == v.dtype
                np.testing.assert_array_equal(got, v)


def test_generated_file_opens_in_h5py(datasets, tmp_path):
    h5py = pytest.importorskip("h5py")
    path = str(tmp_path / "sweep.h5")
    datasets.generate_simulation_file(path, reynolds_numbers=[100], mesh_sizes=(4,), solve=_Stub())
    datasets.generate_simulation_file(path, reynolds_numbers=[200], mesh_sizes=(4,), solve=_Stub())
    with h5py.File(path, "r") as f:
        assert sorted(f) == ["Re100_mesh4x4", "Re200_mesh4x4"]
        g = f["Re200_mesh4x4"]
        assert g.attrs["nx"] == 4 and g.attrs["reynolds_number"] == 200.0
        np.testing.assert_array_equal(g["v"][...].reshape(4, 4), _field(200, 4, 1))


def _append_solution_before(writer, Re, n, fields, bc_type, case_name=""):
    """datasets.append_solution as it was before it learnt `lx` / `ly`."""
    g = f"Re{Re}_mesh{n}x{n}"
    writer.group(g)
    writer.attr(g, "bc_type", bc_type)
    if case_name:
        writer.attr(g, "case_name", case_name)
    writer.attr(g, "reynolds_number", np.float64(Re))
    writer.attr(g, "nx", np.int64(n))
    writer.attr(g, "ny", np.int64(n))
    writer.attr(g, "total_points", np.int64(n * n))
    for c in "uvp":
        writer.dataset(f"{g}/{c}", np.asarray(fields[c], np.float64).reshape(-1))


def test_append_solution_default_output_is_unchanged(datasets, h5, tmp_path):
    fields = {c: _field(400, 6, k) for k, c in enumerate("uvp")}
    a, b = h5.H5Writer(), h5.H5Writer()
    for case_name in ("", "a cavity"):
        _append_solution_before(a, 400 + len(case_name), 6, fields, "single_lid", case_name)
        datasets.append_solution(b, 400 + len(case_name), 6, fields, "single_lid", case_name)
    a.save(str(tmp_path / "a.h5"))
    b.save(str(tmp_path / "b.h5"))
    assert (tmp_path / "a.h5").read_bytes() == (tmp_path / "b.h5").read_bytes()
    # only one of lx / ly: still no x / y
    c = h5.H5Writer()
    datasets.append_solution(c, 400, 6, fields, "single_lid", lx=2.0)
    datasets.append_solution(c, 500, 6, fields, "single_lid", lx=2.0, ly=3.0)
    c.save(str(tmp_path / "c.h5"))
    with h5.H5File(str(tmp_path / "c.h5")) as f:
        assert sorted(f.keys("Re400_mesh6x6")) == ["p", "u", "v"]
        X, Y = np.meshgrid(np.linspace(0, 2.0, 6), np.linspace(0, 3.0, 6))
        np.testing.assert_array_equal(f.read("Re500_mesh6x6/x"), X.flatten())
        np.testing.assert_array_equal(f.read("Re500_mesh6x6/y"), Y.flatten())


def test_batch_footprint_needs_no_device(srcfd):
    """n_cases x ((14 planes x (nx+2)(ny+2) + 9 nx) x 8 bytes + one status block + one parameter block): the per-case blocks
    are the same small size for every mesh and batch size."""
    L = importlib.import_module("sr-for-cfd_amd._lib")

    def footprint(nx, ny, B):
        out = C.c_int64(0)
        L.check(L.lib.srcfd_fine_batch_footprint(nx, ny, B, C.byref(out)))
        return out.value

    def fields(nx, ny, B):
        return B * (14 * (nx + 2) * (ny + 2) + 9 * nx) * 8

    per_case = footprint(3, 3, 1) - fields(3, 3, 1)
    assert 56 <= per_case <= 1024          # the status block (6 ints and 3 doubles) and the parameter block
    for nx, ny, B in ((3, 3, 1), (12, 10, 4), (131, 530, 2), (400, 400, 8), (400, 400, 64), (4096, 4096, 64)):
        assert footprint(nx, ny, B) == fields(nx, ny, B) + B * per_case, (nx, ny, B)
    for nx, ny, B in ((2, 10, 1), (10, 4097, 1), (10, 10, 0), (10, 10, 65)):
        with pytest.raises(ValueError, match="srcfd_fine_batch_footprint"):
            footprint(nx, ny, B)
    with pytest.raises(ValueError, match="n_cases 65"):      # refused before any device is looked for
        h = C.c_void_p()
        L.check(L.lib.srcfd_fine_batch_create((L.CoarseProblem * 65)(), 65, 0, C.byref(h)))
