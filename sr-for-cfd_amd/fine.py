"""The fine-mesh solve the SR warm start is for, on the device: `run_fine_simulation_with_ml_init`, `run_normal_simulation` and
`run_ml_accelerated_fine_simulation` of the reference's lid-driven-cavity solver (PyCFD_ML_accelerated.py:882-966, 1024-1184) and
of its backward-facing-step solver (bfs_ml_accelerated.py:1140-1300, 1384-1518; `run_bfs_*` here, as
coarse.run_bfs_coarse_simulation), on libsrcfd's float64 device solver (csrc/fine_solver.hip, C ABI `srcfd_fine_solver_*`).

`FineSolver` keeps the state on the device; `.Var` is a host copy in the reference's layout (3, nx+2, ny+2), and `.mesh` has the
reference's MeshParameters fields, so the reference's `extract_centerlines(solver, nx, ny)` works on it unchanged.  The loop is
srcfd_coarse_solve's; its inner sweeps are Jacobi (momentum) and red-black (pressure) -- tests/fine_solver_spec.py is the
specification.  No plots; `output_name` writes the HDF5 field file in coarse.save_coarse_fields' layout.

`FineSolverBatch` runs B cases of one mesh in one set of launches (`srcfd_fine_batch_*`; the same solver, of which a `FineSolver`
is a batch of one), each with the bits of a `FineSolver` of its own; `run_normal_simulations` / `run_bfs_normal_simulations` are `run_normal_simulation` /
`run_bfs_normal_simulation` for a list of Reynolds numbers on it (the sweeps of sr-simulation-data-creation.ipynb cell 2).
`FineSolverBatch.init_from_prediction` warm-starts any subset of a batch from one SR call (srcfd_fine_batch_init_from_prediction);
`run_ml_accelerated_fine_simulations` / `run_bfs_ml_accelerated_fine_simulations` are the warm-started drop-ins for a sweep, and
`compare_ml_and_normal_simulations` / `compare_bfs_ml_and_normal_simulations` run each Reynolds number warm and cold in one batch.
`init_from_fields` / `fields_device` (both classes) start cases from fields that are on the device already and return them there
(srcfd_fine_batch_init_from_fields_device / _get_fields_device); on them, `run_interpolated_fine_simulations` is the control arm of a
warm-start study, `compare_warm_starts` runs the arms "ml", "interp" and "zero" in one batch, and `run_nested_simulations` is grid
sequencing (`run_bfs_interpolated_fine_simulations`, `compare_bfs_warm_starts` for the step).

`resident=` (False, True or "auto") on the solver classes and the sweep functions selects the resident mode for meshes of at most
64 x 64 cells (`resident_supported`): one workgroup per case runs many outer iterations per launch, with the same bits.
`run_coarse_simulations` / `run_bfs_coarse_simulations` solve the coarse fields of a whole sweep as one resident batch.

`pressure=` ("sweeps", the default, or "direct") on the solver classes and on every function here that runs a fine solve selects
the inner pressure solver (`FineSolverBatch.set_pressure_solver`): "direct" replaces the red-black sweeps by an exact solve of four
float64 matrix products, in launch mode only.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib as L
from .coarse import BFS_RUN_COARSE_DEFAULT, LDC_SINGLE_LID, SIDES, _bc_dicts, _bc_entry, save_coarse_fields

COMPONENTS = ("u", "v", "p")
_DEFAULT_CC = {"u": 1e-6, "v": 1e-6, "p": 1e-6, "continuity": 1e-6}


class MeshParameters:
    """PyCFD_ML_accelerated.py:69-77."""

    def __init__(self, nx: int, ny: int, lx: float = 1.0, ly: float = 1.0):
        self.nx, self.ny, self.lx, self.ly = nx, ny, lx, ly
        self.dx, self.dy = lx / nx, ly / ny
        self.volp = self.dx * self.dy


def problem(Re: float, nx: int, ny: int, lx: float = 1.0, ly: float = 1.0, dt: float = 0.001, scheme: str = "QUICK",
            convergence_criteria: Optional[Dict[str, float]] = None, bc=None, rho: float = 1.0, bfs: Optional[Dict[str, float]] = None,
            relaxation_factors: Optional[Dict[str, float]] = None) -> L.CoarseProblem:
    """The srcfd_coarse_problem of a solve (the same fields coarse.solve_coarse fills)."""
    if scheme not in ("QUICK", "UPWIND"):
        raise ValueError(f"scheme must be 'QUICK' or 'UPWIND', not {scheme!r}")
    cc = {"u": 1e-6, "v": 1e-6, "p": 1e-6}
    cc.update(convergence_criteria or {})
    pb = L.CoarseProblem()
    pb.nx, pb.ny, pb.lx, pb.ly = int(nx), int(ny), float(lx), float(ly)
    pb.reynolds, pb.rho, pb.dt = float(Re), float(rho), float(dt)
    pb.scheme = 0 if scheme == "QUICK" else 1
    pb.max_iterations = 0
    d_all = _bc_dicts(bc, BFS_RUN_COARSE_DEFAULT if bfs is not None else LDC_SINGLE_LID)
    for k, c in enumerate(COMPONENTS):
        pb.tolerance[k] = float(cc[c])
        for s_, side in enumerate(SIDES):
            t, v = _bc_entry(d_all[c][side])
            pb.bc_type[k][s_] = 0 if t == "dirichlet" else 1
            pb.bc_value[k][s_] = v
    if bfs is not None:
        rf = {"u": 0.5, "v": 0.5, "p": 0.2} if relaxation_factors is None else relaxation_factors
        pb.case_type = 1
        for k, c in enumerate(COMPONENTS):
            pb.relax[k] = float(rf.get(c, 0.2 if c == "p" else 0.5))
        pb.step_height, pb.channel_height, pb.bulk_velocity = float(bfs["step_height"]), float(bfs["h"]), float(bfs["Ub"])
    return pb


def resident_supported(nx: int, ny: int) -> bool:
    """Whether an nx x ny mesh can run in the resident mode (srcfd_fine_resident_supported; needs no device)."""
    return bool(L.lib.srcfd_fine_resident_supported(int(nx), int(ny)))


def _resident_mode(resident, nx: int, ny: int, pressure: str = "sweeps") -> int:
    """The srcfd mode of a `resident=` keyword: False launches, True resident (the library refuses an unsupported mesh and a
    handle whose pressure solver is "direct"), "auto" resident where `resident_supported` holds and the pressure solver is the
    sweeps -- the resident mode has no direct path."""
    if resident == "auto":
        return L.FINE_MODE_RESIDENT if resident_supported(nx, ny) and pressure != "direct" else L.FINE_MODE_LAUNCHES
    if resident is True or resident is False:
        return L.FINE_MODE_RESIDENT if resident else L.FINE_MODE_LAUNCHES
    raise ValueError(f"resident must be False, True or 'auto', not {resident!r}")


def _pressure_code(name) -> int:
    """The srcfd constant of a `pressure=` keyword, "sweeps" or "direct"."""
    if not isinstance(name, str) or name not in L.PRESSURE_SOLVERS:
        raise ValueError(f"pressure must be one of {tuple(L.PRESSURE_SOLVERS)}, not {name!r}")
    return L.PRESSURE_SOLVERS[name]


def _stream_handle(stream, device: int):
    """The hipStream_t of `stream` -- a torch stream, a raw handle, or None for torch's current stream on `device`."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(torch.device("cuda", device))
    return C.c_void_p(getattr(stream, "cuda_stream", stream))


def _case_list(cases, n_cases: int):
    """`cases` as a list of distinct ints (None stays None); ValueError before anything reaches the library."""
    if cases is None:
        return None
    case_list = [int(c) for c in cases]
    if not 1 <= len(case_list) <= n_cases:
        raise ValueError(f"cases must name between 1 and {n_cases} cases, not {len(case_list)}")
    if len(set(case_list)) != len(case_list):
        raise ValueError(f"cases must not repeat a case: {case_list}")
    return case_list


def _fields_in(fields, n_cases: int, cases, hw, device: int):
    """The `fields` of an init_from_fields call, checked: (tensor, pointer, srcfd dtype, n_warm, ctypes case list).  A torch
    tensor must be a contiguous float32 or float64 CUDA tensor (3 * n_warm, h, w) on `device` (_lib.device_ptr); a numpy array of
    that shape is uploaded once, float32 as it is and anything else as float64.  Every refusal is a ValueError raised before the
    library is called; the returned tensor keeps the memory alive for the call."""
    import torch
    case_list = _case_list(cases, n_cases)
    shape = tuple(int(d) for d in getattr(fields, "shape", ()))
    if len(shape) != 3:
        raise ValueError(f"fields must have shape (3 * n_warm, {hw[0]}, {hw[1]}): u, v, p of each field, not {shape}")
    n_warm = len(case_list) if case_list is not None else shape[0] // 3
    if not 1 <= n_warm <= n_cases:
        raise ValueError(f"fields has shape {shape}: its first dimension must be 3 * n_warm for between 1 and {n_cases} warm cases")
    if shape[0] != 3 * n_warm:
        raise ValueError(f"fields has shape {shape}: its first dimension must be 3 * n_warm = {3 * n_warm} (u, v, p of each of "
                         f"{n_warm} field(s))")
    if isinstance(fields, np.ndarray):
        if shape[1:] != tuple(hw):
            raise ValueError(f"fields has per-field shape {shape[1:]}, expected {tuple(hw)}")
        host = np.ascontiguousarray(fields, dtype=np.float32 if fields.dtype == np.float32 else np.float64)
        fields = torch.from_numpy(host).to(torch.device("cuda", device))
    ptr = L.device_ptr(fields, "fields", (torch.float32, torch.float64), (3 * n_warm,) + tuple(hw), device, exact=True)
    idx = None if case_list is None else (C.c_int * n_warm)(*case_list)
    return fields, ptr, L.F32 if fields.dtype == torch.float32 else L.F64, n_warm, idx


def _fields_out(n: int, hw, dtype, out, device: int):
    """The output of a fields_device call: (tensor, pointer, srcfd dtype).  dtype: torch.float64 (None) or torch.float32; `out`,
    when given, is a contiguous CUDA tensor (3 * n, ny, nx) of that dtype on `device`, otherwise one is allocated."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"dtype must be torch.float64 or torch.float32, not {dtype}")
    shape = (3 * n,) + tuple(hw)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=torch.device("cuda", device))
    return out, L.device_ptr(out, "out", dtype, shape, device, exact=True), L.F32 if dtype == torch.float32 else L.F64


def _resampler_fits(resampler, mesh, device: int):
    """(h, w) of the fields a mesh takes through `resampler` (None: the mesh itself); ValueError when it does not end at the mesh."""
    if resampler is None:
        return (mesh.ny, mesh.nx)
    if (resampler.out_h, resampler.out_w) != (mesh.ny, mesh.nx):
        raise ValueError(f"resampler ends at ({resampler.out_h}, {resampler.out_w}), the mesh takes fields of ({mesh.ny}, {mesh.nx})")
    if int(resampler.device) != int(device):
        raise ValueError(f"resampler is on device cuda:{resampler.device}, the solver is on cuda:{device}")
    return (resampler.in_h, resampler.in_w)


class FineSolver:
    """Device-resident float64 solver state for one problem (srcfd_fine_solver_*).  Starts from `_initialize_fields`.
    `resident`: see `set_resident`; `pressure`: see `set_pressure_solver`."""

    def __init__(self, pb: L.CoarseProblem, max_iterations: int = 100000, device: int = 0, resident=False, pressure: str = "sweeps"):
        self.problem = pb
        self.device = int(device)
        self.max_iterations = int(max_iterations)
        self.mesh = MeshParameters(pb.nx, pb.ny, pb.lx, pb.ly)
        self.residual_history = {"u": [], "v": [], "p": []}
        self.iterations = 0
        self.rms = np.zeros(3)
        self._h = C.c_void_p()
        L.check(L.lib.srcfd_fine_solver_create(C.byref(pb), int(device), C.byref(self._h)))
        self.resident = False
        self.pressure = "sweeps"
        try:
            self.set_pressure_solver(pressure)
            self.set_resident(resident)
        except ValueError:
            self.close()
            raise
        self.init()

    def close(self) -> None:
        if getattr(self, "_h", None):
            L.lib.srcfd_fine_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_resident(self, resident) -> bool:
        """False: one launch per inner sweep (the default).  True: the resident mode, one workgroup for the case and up to 100
        outer iterations per launch; ValueError on a mesh that `resident_supported` refuses, and the solver keeps its mode.
        "auto": resident where supported.  The bits are the same, and the mode may change between any two `run` calls.
        Returns whether the solver is now resident."""
        mode = _resident_mode(resident, self.mesh.nx, self.mesh.ny, self.pressure)
        L.check(L.lib.srcfd_fine_solver_set_mode(self._h, mode))
        self.resident = mode == L.FINE_MODE_RESIDENT
        return self.resident

    def set_pressure_solver(self, name: str) -> str:
        """`FineSolverBatch.set_pressure_solver` for the one case (srcfd_fine_solver_set_pressure_solver)."""
        L.check(L.lib.srcfd_fine_solver_set_pressure_solver(self._h, _pressure_code(name)))
        self.pressure = name
        return self.pressure

    @property
    def shape(self):
        return (3, self.mesh.nx + 2, self.mesh.ny + 2)

    def _reset(self):
        self.residual_history = {"u": [], "v": [], "p": []}
        self.iterations = 0

    def init(self, Var: Optional[np.ndarray] = None) -> None:
        """Var None: zero fields; otherwise its interior (3, nx+2, ny+2).  Then BCs, Old = Var, linear_interpolation."""
        if Var is None:
            L.check(L.lib.srcfd_fine_solver_init(self._h, None))
        else:
            Var = np.ascontiguousarray(Var, dtype=np.float64)
            if Var.shape != self.shape:
                raise ValueError(f"Var must have shape {self.shape}, not {Var.shape}")
            L.check(L.lib.srcfd_fine_solver_init(self._h, Var.ctypes.data_as(C.c_void_p)))
        self._reset()

    def init_fields(self, fields: Dict[str, np.ndarray]) -> None:
        """The reference's injection `Var[k, 1:-1, 1:-1] = fields[c].T` (fields (ny, nx)), then the priming of `init`."""
        Var = np.zeros(self.shape)
        for k, c in enumerate(COMPONENTS):
            Var[k, 1:-1, 1:-1] = np.asarray(fields[c]).T
        self.init(Var)

    def init_from_prediction(self, model, x, in_affine=None, out_affine=None, resampler=None, nan_guard: bool = True) -> int:
        """SR of the (3, lr, lr, 1) batch `x` straight into the device state (srcfd_fine_solver_init_from_prediction).
        Returns the number of NaN / Inf values the guard replaced."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        aff = [None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(3, 2) for a in (in_affine, out_affine)]
        bad = C.c_int64(0)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        L.check(L.lib.srcfd_fine_solver_init_from_prediction(self._h, model._h, resampler._h if resampler is not None else None,
                                                             p(x), p(aff[0]), p(aff[1]), L.FLAG_NAN_GUARD if nan_guard else 0,
                                                             C.byref(bad)))
        self._reset()
        return int(bad.value)

    def init_from_fields(self, fields, resampler=None, stream=None) -> None:
        """`FineSolverBatch.init_from_fields` for the one case: `fields` (3, h, w), u, v, p
        (srcfd_fine_solver_init_from_fields_device)."""
        hw = _resampler_fits(resampler, self.mesh, self.device)
        fields, ptr, code, _, _ = _fields_in(fields, 1, None, hw, self.device)
        L.check(L.lib.srcfd_fine_solver_init_from_fields_device(self._h, resampler._h if resampler is not None else None, ptr, code,
                                                                _stream_handle(stream, self.device)))
        self._reset()

    def fields_device(self, dtype=None, out=None, stream=None):
        """`FineSolverBatch.fields_device` for the one case: a (3, ny, nx) CUDA tensor (srcfd_fine_solver_get_fields_device)."""
        out, ptr, code = _fields_out(1, (self.mesh.ny, self.mesh.nx), dtype, out, self.device)
        L.check(L.lib.srcfd_fine_solver_get_fields_device(self._h, ptr, code, _stream_handle(stream, self.device)))
        return out

    def run(self, n: int) -> int:
        """Up to n more outer iterations; returns the outer iterations since init."""
        it = C.c_int(0)
        rms = (C.c_double * 3)()
        hist = np.zeros((n // 100 + 1, 3))
        before = self.iterations
        try:
            L.check(L.lib.srcfd_fine_solver_run(self._h, int(n), C.byref(it), rms, hist.ctypes.data_as(C.c_void_p), hist.shape[0]))
        except ValueError as e:
            if "NaN" in str(e):
                raise ValueError("Solver failed: NaN/Inf in residuals") from e   # what the reference raises (PyCFD...:487-492)
            raise
        self.iterations = int(it.value)
        self.rms = np.array(list(rms))
        for r in hist[:self.iterations // 100 - before // 100]:
            for k, c in enumerate(COMPONENTS):
                self.residual_history[c].append(float(r[k]))
        return self.iterations

    def solve(self, max_iterations: Optional[int] = None) -> int:
        """Runs until converged or `max_iterations` outer iterations in all (default: the problem's cap)."""
        cap = self.max_iterations if max_iterations is None else int(max_iterations)
        return self.run(max(0, cap - self.iterations))

    @property
    def Var(self) -> np.ndarray:
        out = np.empty(self.shape)
        L.check(L.lib.srcfd_fine_solver_get_state(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def counters(self) -> Dict[str, object]:
        c = (C.c_int64 * 4)()
        s = (C.c_int * 3)()
        L.check(L.lib.srcfd_fine_solver_counters(self._h, c, s))
        return {"momentum_sweeps": c[0], "pressure_sweeps": c[1], "launches": c[2], "host_syncs": c[3], "last_sweeps": list(s),
                "pressure_solver": self.pressure}

    def fields(self) -> Dict[str, np.ndarray]:
        V = self.Var
        return {c: V[k, 1:-1, 1:-1].T.copy() for k, c in enumerate(COMPONENTS)}

    def save(self, path: str, Re: float, bfs_step_height: Optional[float] = None) -> None:
        save_coarse_fields(path, self.fields(), Re, self.mesh.lx, self.mesh.ly, bfs_step_height=bfs_step_height)


class FineSolverBatch:
    """B cases of one mesh, scheme and case type in one set of launches (srcfd_fine_batch_*): each case computes what a
    `FineSolver` of its own computes, bit for bit.  `status[i]` is 0 while case i runs (or only the iteration budget ended),
    1 converged, 2 diverged (non-finite residuals; the other cases go on, nothing is raised).  `resident`: see `set_resident`;
    `pressure`: see `set_pressure_solver`."""

    def __init__(self, problems: Sequence[L.CoarseProblem], max_iterations: int = 100000, device: int = 0, resident=False,
                 pressure: str = "sweeps"):
        self.problems = list(problems)
        self.n_cases = len(self.problems)
        self.device = int(device)
        self.max_iterations = int(max_iterations)
        arr = (L.CoarseProblem * max(self.n_cases, 1))(*self.problems)
        self._h = C.c_void_p()
        L.check(L.lib.srcfd_fine_batch_create(arr, self.n_cases, int(device), C.byref(self._h)))
        pb = self.problems[0]
        self.mesh = MeshParameters(pb.nx, pb.ny, pb.lx, pb.ly)
        self.resident = False
        self.pressure = "sweeps"
        try:
            self.set_pressure_solver(pressure)
            self.set_resident(resident)
        except ValueError:
            self.close()
            raise
        self.init()

    def set_resident(self, resident) -> bool:
        """False: every case shares one launch per inner sweep (the default).  True: the resident mode, one workgroup per case
        and up to 100 outer iterations per launch, so that no case waits for another's inner solves; ValueError on a mesh that
        `resident_supported` refuses, and the batch keeps its mode.  "auto": resident where supported.  The bits are the same,
        and the mode may change between any two `run` calls.  Returns whether the batch is now resident."""
        mode = _resident_mode(resident, self.mesh.nx, self.mesh.ny, self.pressure)
        L.check(L.lib.srcfd_fine_batch_set_mode(self._h, mode))
        self.resident = mode == L.FINE_MODE_RESIDENT
        return self.resident

    def set_pressure_solver(self, name: str) -> str:
        """"sweeps" (the default): the red-black pressure sweeps, the bits of tests/fine_solver_spec.py.  "direct": every inner
        pressure solve is solved exactly by four float64 matrix products on the sine bases of the mesh (csrc/poisson_direct.hip;
        srcfd_fine_batch_set_pressure_solver): four launches and no status read in place of up to 1 000 sweeps, counted as one sweep.
        The direct mode reaches the sweeps' fixed point along its own trajectory, has no numpy twin with equal bits, and runs in
        launch mode only: ValueError on a resident handle (and from `set_resident(True)` on a direct one), the handle unchanged;
        `resident="auto"` resolves to launches.  ValueError for any other name.  May change between any two `run` calls.
        Returns the name now in force."""
        L.check(L.lib.srcfd_fine_batch_set_pressure_solver(self._h, _pressure_code(name)))
        self.pressure = name
        return self.pressure

    def close(self) -> None:
        if getattr(self, "_h", None):
            L.lib.srcfd_fine_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def shape(self):
        return (self.n_cases, 3, self.mesh.nx + 2, self.mesh.ny + 2)

    def init(self, Var: Optional[np.ndarray] = None) -> None:
        """Var None: zero fields; otherwise the interiors of (B, 3, nx+2, ny+2).  Every case runs again from iteration 0."""
        if Var is None:
            L.check(L.lib.srcfd_fine_batch_init(self._h, None))
        else:
            Var = np.ascontiguousarray(Var, dtype=np.float64)
            if Var.shape != self.shape:
                raise ValueError(f"Var must have shape {self.shape}, not {Var.shape}")
            L.check(L.lib.srcfd_fine_batch_init(self._h, Var.ctypes.data_as(C.c_void_p)))
        self._reset()

    def init_from_prediction(self, model, x, in_affine=None, out_affine=None, resampler=None, nan_guard: bool = True,
                             cases: Optional[Sequence[int]] = None) -> int:
        """SR of n_warm coarse fields -- `x` (3 * n_warm, lr, lr, 1), u, v, p of each, affines (3 * n_warm, 2) -- straight into
        the device state of the cases `cases` (None: every case, field i into case i); the other cases start from zero fields.
        Every case runs again from iteration 0 (srcfd_fine_batch_init_from_prediction).  Returns the number of NaN / Inf values
        the guard replaced in the warm fields.  The network picks its kernels by the sample count, so a warm case's initial
        bits are those of a 3 * n_warm-sample prediction and depend on n_warm; what the solver makes of a given Var does not."""
        case_list = None if cases is None else [int(c) for c in cases]
        n_warm = self.n_cases if case_list is None else len(case_list)
        if not 1 <= n_warm <= self.n_cases:
            raise ValueError(f"cases must name between 1 and {self.n_cases} cases, not {n_warm}")
        if case_list is not None and len(set(case_list)) != n_warm:
            raise ValueError(f"cases must not repeat a case: {case_list}")
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 4 or x.shape[0] != 3 * n_warm or tuple(x.shape[1:]) != tuple(model.input_shape) or x.shape[3] != 1:
            raise ValueError(f"x must have shape ({3 * n_warm}, lr, lr, 1) for {n_warm} warm cases and the model's input, not {x.shape}")
        aff = []
        for name, a in (("in_affine", in_affine), ("out_affine", out_affine)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.shape != (3 * n_warm, 2):
                    raise ValueError(f"{name} must have shape ({3 * n_warm}, 2), not {a.shape}")
            aff.append(a)
        bad = C.c_int64(0)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        idx = None if case_list is None else (C.c_int * n_warm)(*case_list)
        L.check(L.lib.srcfd_fine_batch_init_from_prediction(self._h, model._h, resampler._h if resampler is not None else None, p(x),
                                                            n_warm, idx, p(aff[0]), p(aff[1]), L.FLAG_NAN_GUARD if nan_guard else 0,
                                                            C.byref(bad)))
        self._reset()
        return int(bad.value)

    def init_from_fields(self, fields, cases: Optional[Sequence[int]] = None, resampler=None, stream=None) -> None:
        """Starts the cases `cases` (None: case i from field i) from fields that are on the device already, every other case
        from zero fields, and every case again from iteration 0 (srcfd_fine_batch_init_from_fields_device).  `fields`:
        (3 * n_warm, h, w), u, v, p of each field in the layout of the SR prediction and the coarse-field dicts (field[j, i] is
        cell (i, j)); a contiguous float32 or float64 CUDA tensor, or a numpy array, which is uploaded once.  (h, w) is the
        mesh's (ny, nx), or with `resampler` its input, and the fields go through it in float64.  Values are taken as they are:
        there is no NaN guard.  `stream`: the torch stream the fields were produced on (None: the current one); the solver
        waits for it on the device, so the caller does not synchronise first, and the call returns when the state is primed."""
        hw = _resampler_fits(resampler, self.mesh, self.device)
        fields, ptr, code, n_warm, idx = _fields_in(fields, self.n_cases, cases, hw, self.device)
        L.check(L.lib.srcfd_fine_batch_init_from_fields_device(self._h, resampler._h if resampler is not None else None, ptr, code,
                                                               n_warm, idx, _stream_handle(stream, self.device)))
        self._reset()

    def fields_device(self, cases: Optional[Sequence[int]] = None, dtype=None, out=None, stream=None):
        """The fields of the cases `cases` (None: all, in order) as a (3 * n, ny, nx) CUDA tensor, u, v, p of each: what
        `fields(i)` returns, without a host copy (srcfd_fine_batch_get_fields_device).  dtype: torch.float64 (the default, an exact
        copy) or torch.float32 (rounded to nearest); `out`: a tensor to write into.  Complete at return, and `stream` (None: the
        current torch stream) waits for it as well."""
        case_list = _case_list(cases, self.n_cases)
        n = self.n_cases if case_list is None else len(case_list)
        out, ptr, code = _fields_out(n, (self.mesh.ny, self.mesh.nx), dtype, out, self.device)
        idx = None if case_list is None else (C.c_int * n)(*case_list)
        L.check(L.lib.srcfd_fine_batch_get_fields_device(self._h, n, idx, ptr, code, _stream_handle(stream, self.device)))
        return out

    def _reset(self) -> None:
        self.residual_history: List[Dict[str, List[float]]] = [{"u": [], "v": [], "p": []} for _ in range(self.n_cases)]
        self.iterations = np.zeros(self.n_cases, dtype=np.int64)
        self.status = np.zeros(self.n_cases, dtype=np.int64)
        self.rms = np.zeros((self.n_cases, 3))

    def run(self, n: int) -> np.ndarray:
        """Up to n more outer iterations of every running case; returns the per-case iteration counts."""
        B, rows = self.n_cases, int(n) // 100 + 1
        it, st = (C.c_int * B)(), (C.c_int * B)()
        rms, hist = np.zeros((B, 3)), np.zeros((B, rows, 3))
        before = self.iterations
        L.check(L.lib.srcfd_fine_batch_run(self._h, int(n), it, st, rms.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p), rows))
        self.iterations = np.array(list(it), dtype=np.int64)
        self.status = np.array(list(st), dtype=np.int64)
        self.rms = rms
        for i in range(B):
            for r in hist[i, :self.iterations[i] // 100 - before[i] // 100]:
                for k, c in enumerate(COMPONENTS):
                    self.residual_history[i][c].append(float(r[k]))
        return self.iterations

    def solve(self, max_iterations: Optional[int] = None) -> np.ndarray:
        """Runs until no case is running or the running ones have done `max_iterations` outer iterations in all."""
        cap = self.max_iterations if max_iterations is None else int(max_iterations)
        return self.run(max(0, cap - int(self.iterations.max(initial=0))))

    @property
    def Var(self) -> np.ndarray:
        out = np.empty(self.shape)
        L.check(L.lib.srcfd_fine_batch_get_state(self._h, -1, out.ctypes.data_as(C.c_void_p)))
        return out

    def case_var(self, i: int) -> np.ndarray:
        out = np.empty(self.shape[1:])
        L.check(L.lib.srcfd_fine_batch_get_state(self._h, int(i), out.ctypes.data_as(C.c_void_p)))
        return out

    def fields(self, i: int) -> Dict[str, np.ndarray]:
        V = self.case_var(i)
        return {c: V[k, 1:-1, 1:-1].T.copy() for k, c in enumerate(COMPONENTS)}

    def counters(self) -> Dict[str, object]:
        c = (C.c_int64 * 4)()
        s = (C.c_int * (3 * self.n_cases))()
        L.check(L.lib.srcfd_fine_batch_counters(self._h, c, s))
        return {"momentum_sweeps": c[0], "pressure_sweeps": c[1], "launches": c[2], "host_syncs": c[3],
                "last_sweeps": [list(s[3 * i:3 * i + 3]) for i in range(self.n_cases)], "pressure_solver": self.pressure}


def _finish(solver: FineSolver, Re, output_name, suffix, bfs_step_height=None):
    t0 = time.time()
    it = solver.solve()
    elapsed = time.time() - t0
    if output_name is not None:
        name = output_name if output_name.endswith(suffix) else f"{output_name}{suffix}"
        d = os.path.dirname(name)
        if d:
            os.makedirs(d, exist_ok=True)
        solver.save(f"{name}.h5", Re, bfs_step_height=bfs_step_height)
    return solver, it, elapsed


# ---------------------------------------------------------------------------------------------- lid-driven cavity
def run_fine_simulation_with_ml_init(Re: float, nx: int, ny: int, ml_initial_fields: Dict[str, np.ndarray], dt: float = 0.001,
                                     scheme: str = "QUICK", convergence_criteria: Optional[Dict[str, float]] = None,
                                     max_iterations: int = 100000, output_name: Optional[str] = "cavity_accelerated", bc=None,
                                     pressure: str = "sweeps") -> tuple:
    """PyCFD_ML_accelerated.py:882-963: (solver, iterations, time_elapsed); fields (ny, nx) are injected transposed."""
    s = FineSolver(problem(Re, nx, ny, 1.0, 1.0, dt, scheme, convergence_criteria or _DEFAULT_CC, bc), max_iterations, pressure=pressure)
    s.init_fields(ml_initial_fields)
    return _finish(s, Re, output_name, "_accelerated")


def run_normal_simulation(Re: float, nx: int, ny: int, dt: float = 0.001, scheme: str = "QUICK",
                          convergence_criteria: Optional[Dict[str, float]] = None, max_iterations: int = 100000,
                          output_name: Optional[str] = "cavity_normal", bc=None, pressure: str = "sweeps") -> tuple:
    """PyCFD_ML_accelerated.py:1126-1184: the same solve from zero fields."""
    s = FineSolver(problem(Re, nx, ny, 1.0, 1.0, dt, scheme, convergence_criteria or _DEFAULT_CC, bc), max_iterations, pressure=pressure)
    return _finish(s, Re, output_name, "_normal")


def _per_case(bc, n):
    """One BC set for every case, or a list with one per case."""
    if isinstance(bc, (list, tuple)):
        if len(bc) != n:
            raise ValueError(f"bc must be one boundary-condition set or a list of {n}, one per Reynolds number")
        return list(bc)
    return [bc] * n


def _solve_in_batches(problems, max_iterations, max_batch, device, warm_start=None, resident=False, pressure="sweeps"):
    """warm_start(batch, a): starts the batch of problems[a : a + batch.n_cases] (default: from zero fields, as created)."""
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    out = []
    for a in range(0, len(problems), max_batch):
        b = FineSolverBatch(problems[a:a + max_batch], max_iterations, device, resident=resident, pressure=pressure)
        try:
            if warm_start is not None:
                warm_start(b, a)
            b.solve()
            out += [(b.fields(i), int(b.iterations[i]), int(b.status[i])) for i in range(b.n_cases)]
        finally:
            b.close()
    return out


def run_normal_simulations(reynolds: Sequence[float], nx: int, ny: int, dt: float = 0.001, scheme: str = "QUICK",
                           convergence_criteria: Optional[Dict[str, float]] = None, max_iterations: int = 100000, bc=None,
                           max_batch: int = 8, device: int = 0, resident=False, pressure: str = "sweeps") -> list:
    """`run_normal_simulation` for a list of Reynolds numbers, `max_batch` cases at a time on the batched device solver:
    a list of (fields, iterations, status) in input order; fields are the (ny, nx) u, v, p, status as FineSolverBatch's.
    `bc`: one boundary-condition set or a list with one per Reynolds number.  `resident`: as FineSolverBatch.set_resident."""
    reynolds = list(reynolds)
    bcs = _per_case(bc, len(reynolds))
    pbs = [problem(Re, nx, ny, 1.0, 1.0, dt, scheme, convergence_criteria or _DEFAULT_CC, b) for Re, b in zip(reynolds, bcs)]
    return _solve_in_batches(pbs, max_iterations, max_batch, device, resident=resident, pressure=pressure)


def _coarse_sweep(problems, reynolds, max_iterations, max_batch, device, output_dir, name_of, bfs_step_height=None):
    out = _solve_in_batches(problems, max_iterations, max_batch, device, resident=True)
    fields_list = []
    for pb, Re, (fields, _, status) in zip(problems, reynolds, out):
        if status == L.CASE_DIVERGED:
            raise ValueError(f"Solver failed: NaN/Inf in residuals (Re {Re})")
        if output_dir is not None:
            os.makedirs(output_dir, exist_ok=True)
            save_coarse_fields(os.path.join(output_dir, name_of(Re)), fields, Re, pb.lx, pb.ly, bfs_step_height=bfs_step_height)
        fields_list.append(fields)
    return fields_list


def run_coarse_simulations(reynolds: Sequence[float], lr_dim: int = 10, dt: float = 0.001, scheme: str = "QUICK",
                           convergence_criteria: Optional[Dict[str, float]] = None, max_iterations: int = 100000,
                           output_dir: Optional[str] = None, bc=None, max_batch: int = 64, device: int = 0) -> List[Dict[str, np.ndarray]]:
    """`coarse.run_coarse_simulation` (same arguments and defaults) for a list of Reynolds numbers on the device: one resident
    batch serves up to `max_batch` (at most 64) of them, each case in a workgroup of its own.  Returns the {'u','v','p'} dicts
    of (lr_dim, lr_dim) fields in input order: the `coarse_fields_list` of the warm-started sweeps.  `bc`: one set or one per
    Reynolds number.  These solves follow the device's sweep order (Jacobi momentum, red-black pressure;
    tests/fine_solver_spec.py), not the host's serial sweeps of `srcfd_coarse_solve`: the same fixed point -- the reference's
    stored coarse fields pin both to 6e-8 -- reached along another trajectory, so iteration counts and the last bits differ
    from `coarse.run_coarse_simulation`.  A diverged case raises ValueError, as the host function does."""
    reynolds = list(reynolds)
    bcs = _per_case(bc, len(reynolds))
    pbs = [problem(Re, lr_dim, lr_dim, 1.0, 1.0, dt, scheme, convergence_criteria, b) for Re, b in zip(reynolds, bcs)]
    return _coarse_sweep(pbs, reynolds, max_iterations, max_batch, device, output_dir,
                         lambda Re: f"coarse_Re{Re}_{lr_dim}x{lr_dim}_{max_iterations}_coarse_iterations.h5")


def run_bfs_coarse_simulations(reynolds: Sequence[float], lr_dim: int = 10, dt: float = 0.002, scheme: str = "UPWIND",
                               convergence_criteria: Optional[Dict[str, float]] = None, max_iterations: int = 100000,
                               output_dir: Optional[str] = None, bc=None, step_height: float = 1.0, h: float = 2.0, Ub: float = 1.0,
                               lx: float = 10.0, ly: float = 3.0, relaxation_factors: Optional[Dict[str, float]] = None,
                               max_batch: int = 64, device: int = 0) -> List[Dict[str, np.ndarray]]:
    """`coarse.run_bfs_coarse_simulation` for a list of Reynolds numbers, as `run_coarse_simulations` (the device's sweep order:
    the host solver's fixed point, not its trajectory)."""
    reynolds = list(reynolds)
    bcs = _per_case(bc, len(reynolds))
    pbs = [problem(Re, lr_dim, lr_dim, lx, ly, dt, scheme, convergence_criteria, b, bfs={"step_height": step_height, "h": h, "Ub": Ub},
                   relaxation_factors=relaxation_factors) for Re, b in zip(reynolds, bcs)]
    return _coarse_sweep(pbs, reynolds, max_iterations, max_batch, device, output_dir,
                         lambda Re: f"bfs_coarse_Re{Re}_{lr_dim}x{lr_dim}_{max_iterations}_coarse_iterations.h5", bfs_step_height=step_height)


def _model_files(stats_file, encoder_file, decoder_file):
    for fname, desc in ((stats_file, "Stats file"), (encoder_file, "Encoder model"), (decoder_file, "Decoder model")):
        if not os.path.exists(fname):
            raise FileNotFoundError(f"{desc} not found: {fname}")


def run_ml_accelerated_fine_simulation(coarse_fields: Dict[str, np.ndarray], Re: float, nx: int, ny: int, lr_dim: int = 10,
                                       dt: float = 0.001, scheme: str = "QUICK", convergence_criteria: Optional[Dict[str, float]] = None,
                                       max_iterations_fine: int = 100000, output_name: Optional[str] = None, stats_file: Optional[str] = None,
                                       encoder_file: Optional[str] = None, decoder_file: Optional[str] = None, bc=None,
                                       precision: Optional[str] = None, resident=False, pressure: str = "sweeps") -> tuple:
    """PyCFD_ML_accelerated.py:1024-1123: coarse fields -> SR straight into the device solver state -> fine solve.  The only
    400x400 field that crosses to the host is the result (`solver.Var`, on demand).  `resident`: as FineSolver.set_resident."""
    from . import pipeline
    stats_file = stats_file or f"standardization_stats_{lr_dim}to{nx}.txt"
    encoder_file = encoder_file or f"vanilla_encoder{lr_dim}_to_{nx}.h5"
    decoder_file = decoder_file or f"vanilla_decoder{nx}_from_{lr_dim}.h5"
    output_name = output_name or f"cavity_Re{Re}_{nx}x{ny}"
    _model_files(stats_file, encoder_file, decoder_file)
    model, x, ain, aout, back, _ = pipeline._prepare(coarse_fields, lr_dim, nx, stats_file, encoder_file, decoder_file, False, 1.0, 1.0,
                                                     False, 0.3, precision, pipeline._quiet)
    s = FineSolver(problem(Re, nx, ny, 1.0, 1.0, dt, scheme, convergence_criteria or _DEFAULT_CC, bc), max_iterations_fine, model.device,
                   resident=resident, pressure=pressure)
    pipeline._warn_nonfinite(s.init_from_prediction(model, x, ain, aout, back))
    return _finish(s, Re, output_name, "_accelerated")


def _warm_sweep(coarse_fields_list, problems, prepare, max_iterations, max_batch, output_name, suffix_of, bfs_step_height=None,
                every=1, resident=False, pressure: str = "sweeps"):
    """The batched warm-started solve behind the sweep drop-ins.  `problems` holds `every` consecutive cases per coarse field,
    of which the first is warm-started from it and the others start from zero; prepare(fields) is pipeline._prepare_batch for
    a list of coarse fields.  The prediction of a batch holds the fields of that batch's warm cases only."""
    from . import pipeline
    if max_batch < every:
        raise ValueError(f"max_batch must be at least {every}")
    model = prepare([])[0]   # the handle is cached: this picks the device before any solver exists

    def warm_start(b, a):
        first, n_warm = a // every, b.n_cases // every
        _, x, ain, aout, back = prepare(coarse_fields_list[first:first + n_warm])
        cases = None if every == 1 else [every * i for i in range(n_warm)]
        pipeline._warn_nonfinite(b.init_from_prediction(model, x, ain, aout, back, cases=cases))

    out = _solve_in_batches(problems, max_iterations, max_batch - max_batch % every, model.device, warm_start, resident=resident, pressure=pressure)
    _save_sweep(out, problems, output_name, suffix_of, bfs_step_height)
    return out


def _save_sweep(out, problems, output_name, suffix_of, bfs_step_height=None):
    """Each case's fields to `{output_name}_Re{Re}{suffix_of(i)}.h5` (output_name None: nothing is written)."""
    if output_name is None:
        return
    for i, (fields, _, _) in enumerate(out):
        name = f"{output_name}_Re{problems[i].reynolds:g}{suffix_of(i)}"
        d = os.path.dirname(name)
        if d:
            os.makedirs(d, exist_ok=True)
        save_coarse_fields(f"{name}.h5", fields, problems[i].reynolds, problems[i].lx, problems[i].ly, bfs_step_height=bfs_step_height)


def _paired(out, reynolds):
    """(warm, cold) result pairs of `_warm_sweep(..., every=2)` as the reference's end-of-script comparison
    (PyCFD_ML_accelerated.py:1488-1499, bfs_ml_accelerated.py main), one dict per Reynolds number."""
    res = []
    for i, Re in enumerate(reynolds):
        (f_ml, it_ml, st_ml), (f_n, it_n, st_n) = out[2 * i], out[2 * i + 1]
        res.append({"Re": Re, "ml_iterations": it_ml, "normal_iterations": it_n, "ml_status": st_ml, "normal_status": st_n,
                    "iterations_saved": it_n - it_ml, "ratio": it_n / it_ml if it_ml else float("nan"),
                    "ml_fields": f_ml, "normal_fields": f_n})
    return res


def _ldc_sweep(coarse_fields_list, reynolds, nx, ny, lr_dim, dt, scheme, convergence_criteria, max_iterations_fine, output_name, stats_file,
               encoder_file, decoder_file, bc, precision, max_batch, device, every, resident=False, pressure: str = "sweeps"):
    from . import pipeline
    reynolds, coarse_fields_list = list(reynolds), list(coarse_fields_list)
    if len(coarse_fields_list) != len(reynolds):
        raise ValueError(f"coarse_fields_list must hold one set of coarse fields per Reynolds number ({len(reynolds)}), not {len(coarse_fields_list)}")
    bcs = _per_case(bc, len(reynolds))
    stats_file = stats_file or f"standardization_stats_{lr_dim}to{nx}.txt"
    encoder_file = encoder_file or f"vanilla_encoder{lr_dim}_to_{nx}.h5"
    decoder_file = decoder_file or f"vanilla_decoder{nx}_from_{lr_dim}.h5"
    _model_files(stats_file, encoder_file, decoder_file)
    pbs = [problem(Re, nx, ny, 1.0, 1.0, dt, scheme, convergence_criteria or _DEFAULT_CC, b) for Re, b in zip(reynolds, bcs) for _ in range(every)]
    prepare = lambda fields: pipeline._prepare_batch(fields, lr_dim, nx, stats_file, encoder_file, decoder_file, False, 1.0, 1.0, False, 0.3,
                                                     precision, device)
    return _warm_sweep(coarse_fields_list, pbs, prepare, max_iterations_fine, max_batch, output_name,
                       lambda i: "_accelerated" if i % every == 0 else "_normal", every=every, resident=resident, pressure=pressure)


def run_ml_accelerated_fine_simulations(coarse_fields_list: Sequence[Dict[str, np.ndarray]], reynolds: Sequence[float], nx: int, ny: int,
                                        lr_dim: int = 10, dt: float = 0.001, scheme: str = "QUICK",
                                        convergence_criteria: Optional[Dict[str, float]] = None, max_iterations_fine: int = 100000,
                                        output_name: Optional[str] = None, stats_file: Optional[str] = None,
                                        encoder_file: Optional[str] = None, decoder_file: Optional[str] = None, bc=None,
                                        precision: Optional[str] = None, resident=False, pressure: str = "sweeps", max_batch: int = 8,
                                        device: Optional[int] = None) -> list:
    """`run_ml_accelerated_fine_simulation` for a list of coarse fields and their Reynolds numbers, `max_batch` cases at a time:
    one SR call per batch straight into the batched device solver, then the batched solve.  Returns a list of (fields,
    iterations, status) in input order, as `run_normal_simulations`.  `bc`: one boundary-condition set or one per case.
    `output_name`: None writes nothing; otherwise each case's fields go to `{output_name}_Re{Re}_accelerated.h5`.  `device`:
    None lets the model loader choose.  A case's initial field has the bits of its batch's prediction (see
    FineSolverBatch.init_from_prediction); with max_batch=1 every case equals the single-case function bit for bit.
    `resident`: as FineSolverBatch.set_resident."""
    return _ldc_sweep(coarse_fields_list, reynolds, nx, ny, lr_dim, dt, scheme, convergence_criteria, max_iterations_fine, output_name,
                      stats_file, encoder_file, decoder_file, bc, precision, max_batch, device, 1, resident, pressure)


def compare_ml_and_normal_simulations(coarse_fields_list: Sequence[Dict[str, np.ndarray]], reynolds: Sequence[float], nx: int, ny: int,
                                      lr_dim: int = 10, dt: float = 0.001, scheme: str = "QUICK",
                                      convergence_criteria: Optional[Dict[str, float]] = None, max_iterations_fine: int = 100000,
                                      output_name: Optional[str] = None, stats_file: Optional[str] = None,
                                      encoder_file: Optional[str] = None, decoder_file: Optional[str] = None, bc=None,
                                      precision: Optional[str] = None, resident=False, pressure: str = "sweeps", max_batch: int = 8,
                                      device: Optional[int] = None) -> list:
    """The reference's headline experiment (PyCFD_ML_accelerated.py:1431-1499) for a sweep: every Reynolds number goes into the
    batch twice, case 2i warm-started from its coarse field and case 2i + 1 from zero fields, under the same iteration cap.
    Returns one dict per Reynolds number: Re, ml_iterations, normal_iterations, ml_status, normal_status, iterations_saved
    (normal - ml), ratio (normal / ml) and both results' fields.  Whether iterations are saved depends on the decoder's
    weights; the function only reports the counts."""
    out = _ldc_sweep(coarse_fields_list, reynolds, nx, ny, lr_dim, dt, scheme, convergence_criteria, max_iterations_fine, output_name,
                     stats_file, encoder_file, decoder_file, bc, precision, max_batch, device, 2, resident, pressure)
    return _paired(out, list(reynolds))


# ---------------------------------------------------------------------------------------------- backward-facing step
def _bfs_problem(Re, nx, ny, dt, scheme, convergence_criteria, bc, step_height, h, Ub, lx, ly, relaxation_factors):
    return problem(Re, nx, ny, lx, ly, dt, scheme, convergence_criteria or _DEFAULT_CC, bc,
                   bfs={"step_height": step_height, "h": h, "Ub": Ub}, relaxation_factors=relaxation_factors)


def run_bfs_fine_simulation_with_ml_init(Re: float, nx: int, ny: int, ml_initial_fields: Dict[str, np.ndarray], dt: float = 0.002,
                                         scheme: str = "UPWIND", convergence_criteria: Optional[Dict[str, float]] = None,
                                         max_iterations: int = 100000, output_name: Optional[str] = "bfs_accelerated", bc=None,
                                         step_height: float = 1.0, h: float = 2.0, Ub: float = 1.0, lx: float = 10.0, ly: float = 3.0,
                                         relaxation_factors: Optional[Dict[str, float]] = None, pressure: str = "sweeps") -> tuple:
    """bfs_ml_accelerated.py:1140-1234."""
    s = FineSolver(_bfs_problem(Re, nx, ny, dt, scheme, convergence_criteria, bc, step_height, h, Ub, lx, ly, relaxation_factors),
                   max_iterations, pressure=pressure)
    s.init_fields(ml_initial_fields)
    return _finish(s, Re, output_name, "_accelerated", bfs_step_height=step_height)


def run_bfs_normal_simulation(Re: float, nx: int, ny: int, dt: float = 0.002, scheme: str = "UPWIND",
                              convergence_criteria: Optional[Dict[str, float]] = None, max_iterations: int = 100000,
                              output_name: Optional[str] = "bfs_normal", bc=None, step_height: float = 1.0, h: float = 2.0, Ub: float = 1.0,
                              lx: float = 10.0, ly: float = 3.0, relaxation_factors: Optional[Dict[str, float]] = None,
                              pressure: str = "sweeps") -> tuple:
    """bfs_ml_accelerated.py:1237-1307."""
    s = FineSolver(_bfs_problem(Re, nx, ny, dt, scheme, convergence_criteria, bc, step_height, h, Ub, lx, ly, relaxation_factors),
                   max_iterations, pressure=pressure)
    return _finish(s, Re, output_name, "_normal", bfs_step_height=step_height)


def run_bfs_normal_simulations(reynolds: Sequence[float], nx: int, ny: int, dt: float = 0.002, scheme: str = "UPWIND",
                               convergence_criteria: Optional[Dict[str, float]] = None, max_iterations: int = 100000, bc=None,
                               step_height: float = 1.0, h: float = 2.0, Ub: float = 1.0, lx: float = 10.0, ly: float = 3.0,
                               relaxation_factors: Optional[Dict[str, float]] = None, max_batch: int = 8, device: int = 0,
                               resident=False, pressure: str = "sweeps") -> list:
    """`run_bfs_normal_simulation` for a list of Reynolds numbers, batched as `run_normal_simulations`."""
    reynolds = list(reynolds)
    bcs = _per_case(bc, len(reynolds))
    pbs = [_bfs_problem(Re, nx, ny, dt, scheme, convergence_criteria, b, step_height, h, Ub, lx, ly, relaxation_factors)
           for Re, b in zip(reynolds, bcs)]
    return _solve_in_batches(pbs, max_iterations, max_batch, device, resident=resident, pressure=pressure)


def run_bfs_ml_accelerated_fine_simulation(coarse_fields: Dict[str, np.ndarray], Re: float, nx: int, ny: int, lr_dim: int = 10,
                                           dt: float = 0.002, scheme: str = "UPWIND", convergence_criteria: Optional[Dict[str, float]] = None,
                                           max_iterations_fine: int = 100000, output_name: Optional[str] = None,
                                           stats_file: Optional[str] = None, encoder_file: Optional[str] = None,
                                           decoder_file: Optional[str] = None, bc=None, step_height: float = 1.0, h: float = 2.0,
                                           Ub: float = 1.0, lx: float = 10.0, ly: float = 3.0,
                                           relaxation_factors: Optional[Dict[str, float]] = None, use_aspect_ratio_correction: bool = False,
                                           use_adaptive_normalization: bool = True, blend_factor: float = 0.3,
                                           precision: Optional[str] = None, resident=False, pressure: str = "sweeps") -> tuple:
    """bfs_ml_accelerated.py:1384-1518 (the BFS `ml_super_resolution`: adaptive normalisation, optional aspect-ratio resampling)."""
    from . import pipeline
    stats_file = stats_file or f"standardization_stats_{lr_dim}to{nx}_swish_trained_upto_700_multiBC.txt"
    encoder_file = encoder_file or f"vanilla_encoder{lr_dim}_to_{nx}_swish_trained_upto_700_multiBC.h5"
    decoder_file = decoder_file or f"vanilla_decoder{nx}_from_{lr_dim}_swish_trained_upto_700_multiBC.h5"
    output_name = output_name or f"bfs_Re{Re}_{nx}x{ny}"
    _model_files(stats_file, encoder_file, decoder_file)
    model, x, ain, aout, back, _ = pipeline._prepare(coarse_fields, lr_dim, nx, stats_file, encoder_file, decoder_file,
                                                     use_aspect_ratio_correction, lx, ly, use_adaptive_normalization, blend_factor, precision,
                                                     pipeline._quiet)
    s = FineSolver(_bfs_problem(Re, nx, ny, dt, scheme, convergence_criteria, bc, step_height, h, Ub, lx, ly, relaxation_factors),
                   max_iterations_fine, model.device, resident=resident, pressure=pressure)
    pipeline._warn_nonfinite(s.init_from_prediction(model, x, ain, aout, back))
    return _finish(s, Re, output_name, "_accelerated", bfs_step_height=step_height)


def _bfs_sweep(coarse_fields_list, reynolds, nx, ny, lr_dim, dt, scheme, convergence_criteria, max_iterations_fine, output_name, stats_file,
               encoder_file, decoder_file, bc, step_height, h, Ub, lx, ly, relaxation_factors, use_aspect_ratio_correction,
               use_adaptive_normalization, blend_factor, precision, max_batch, device, every, resident=False, pressure: str = "sweeps"):
    from . import pipeline
    reynolds, coarse_fields_list = list(reynolds), list(coarse_fields_list)
    if len(coarse_fields_list) != len(reynolds):
        raise ValueError(f"coarse_fields_list must hold one set of coarse fields per Reynolds number ({len(reynolds)}), not {len(coarse_fields_list)}")
    bcs = _per_case(bc, len(reynolds))
    stats_file = stats_file or f"standardization_stats_{lr_dim}to{nx}_swish_trained_upto_700_multiBC.txt"
    encoder_file = encoder_file or f"vanilla_encoder{lr_dim}_to_{nx}_swish_trained_upto_700_multiBC.h5"
    decoder_file = decoder_file or f"vanilla_decoder{nx}_from_{lr_dim}_swish_trained_upto_700_multiBC.h5"
    _model_files(stats_file, encoder_file, decoder_file)
    pbs = [_bfs_problem(Re, nx, ny, dt, scheme, convergence_criteria, b, step_height, h, Ub, lx, ly, relaxation_factors)
           for Re, b in zip(reynolds, bcs) for _ in range(every)]
    prepare = lambda fields: pipeline._prepare_batch(fields, lr_dim, nx, stats_file, encoder_file, decoder_file, use_aspect_ratio_correction,
                                                     lx, ly, use_adaptive_normalization, blend_factor, precision, device)
    return _warm_sweep(coarse_fields_list, pbs, prepare, max_iterations_fine, max_batch, output_name,
                       lambda i: "_accelerated" if i % every == 0 else "_normal", bfs_step_height=step_height, every=every,
                       resident=resident, pressure=pressure)


def run_bfs_ml_accelerated_fine_simulations(coarse_fields_list: Sequence[Dict[str, np.ndarray]], reynolds: Sequence[float], nx: int, ny: int,
                                            lr_dim: int = 10, dt: float = 0.002, scheme: str = "UPWIND",
                                            convergence_criteria: Optional[Dict[str, float]] = None, max_iterations_fine: int = 100000,
                                            output_name: Optional[str] = None, stats_file: Optional[str] = None,
                                            encoder_file: Optional[str] = None, decoder_file: Optional[str] = None, bc=None,
                                            step_height: float = 1.0, h: float = 2.0, Ub: float = 1.0, lx: float = 10.0, ly: float = 3.0,
                                            relaxation_factors: Optional[Dict[str, float]] = None, use_aspect_ratio_correction: bool = False,
                                            use_adaptive_normalization: bool = True, blend_factor: float = 0.3,
                                            precision: Optional[str] = None, resident=False, pressure: str = "sweeps", max_batch: int = 8,
                                            device: Optional[int] = None) -> list:
    """`run_bfs_ml_accelerated_fine_simulation` for a list of coarse fields and their Reynolds numbers, batched as
    `run_ml_accelerated_fine_simulations`."""
    return _bfs_sweep(coarse_fields_list, reynolds, nx, ny, lr_dim, dt, scheme, convergence_criteria, max_iterations_fine, output_name,
                      stats_file, encoder_file, decoder_file, bc, step_height, h, Ub, lx, ly, relaxation_factors, use_aspect_ratio_correction,
                      use_adaptive_normalization, blend_factor, precision, max_batch, device, 1, resident, pressure)


def compare_bfs_ml_and_normal_simulations(coarse_fields_list: Sequence[Dict[str, np.ndarray]], reynolds: Sequence[float], nx: int, ny: int,
                                          lr_dim: int = 10, dt: float = 0.002, scheme: str = "UPWIND",
                                          convergence_criteria: Optional[Dict[str, float]] = None, max_iterations_fine: int = 100000,
                                          output_name: Optional[str] = None, stats_file: Optional[str] = None,
                                          encoder_file: Optional[str] = None, decoder_file: Optional[str] = None, bc=None,
                                          step_height: float = 1.0, h: float = 2.0, Ub: float = 1.0, lx: float = 10.0, ly: float = 3.0,
                                          relaxation_factors: Optional[Dict[str, float]] = None, use_aspect_ratio_correction: bool = False,
                                          use_adaptive_normalization: bool = True, blend_factor: float = 0.3,
                                          precision: Optional[str] = None, resident=False, pressure: str = "sweeps", max_batch: int = 8,
                                          device: Optional[int] = None) -> list:
    """`compare_ml_and_normal_simulations` for the backward-facing step (bfs_ml_accelerated.py main)."""
    out = _bfs_sweep(coarse_fields_list, reynolds, nx, ny, lr_dim, dt, scheme, convergence_criteria, max_iterations_fine, output_name,
                     stats_file, encoder_file, decoder_file, bc, step_height, h, Ub, lx, ly, relaxation_factors, use_aspect_ratio_correction,
                     use_adaptive_normalization, blend_factor, precision, max_batch, device, 2, resident, pressure)
    return _paired(out, list(reynolds))


# ---------------------------------------------------------------------------------------------- starts from device fields
def interpolation_matrices(lr_h: int, lr_w: int, nx: int, ny: int, lx: float = 1.0, ly: float = 1.0):
    """(Ry [ny][lr_h], Rx [nx][lr_w]) of the plainly interpolated start: fine = Ry @ coarse @ Rx.T is the interpolating bicubic
    spline of a (lr_h, lr_w) field on the (ny, nx) mesh, with the reference's own node convention, linspace(0, L, n) on both
    sides (resample.interp_matrix)."""
    from . import resample as rs
    return rs.interp_matrix(int(lr_h), float(ly), int(ny), float(ly)), rs.interp_matrix(int(lr_w), float(lx), int(nx), float(lx))


def interpolation_resampler(lr_h: int, lr_w: int, nx: int, ny: int, lx: float = 1.0, ly: float = 1.0, device: int = 0):
    """`interpolation_matrices` as a device `Resampler`."""
    from . import resample as rs
    Ry, Rx = interpolation_matrices(lr_h, lr_w, nx, ny, lx, ly)
    return rs.Resampler(Ry, Rx, int(device))


def _stack_fields(coarse_fields_list) -> np.ndarray:
    """(3 * n, h, w) float64: u, v, p of each coarse-field dict."""
    return np.stack([np.asarray(cf[c], dtype=np.float64) for cf in coarse_fields_list for c in COMPONENTS])


def _interpolated_sweep(coarse_fields_list, reynolds, problems, lr_dim, max_iterations, output_name, max_batch, device, resident,
                        bfs_step_height=None, pressure="sweeps"):
    coarse_fields_list = list(coarse_fields_list)
    if len(coarse_fields_list) != len(reynolds):
        raise ValueError(f"coarse_fields_list must hold one set of coarse fields per Reynolds number ({len(reynolds)}), not {len(coarse_fields_list)}")
    pb = problems[0]
    interp = interpolation_resampler(lr_dim, lr_dim, pb.nx, pb.ny, pb.lx, pb.ly, device)
    try:
        warm_start = lambda b, a: b.init_from_fields(_stack_fields(coarse_fields_list[a:a + b.n_cases]), resampler=interp)
        out = _solve_in_batches(problems, max_iterations, max_batch, device, warm_start, resident=resident, pressure=pressure)
    finally:
        interp.close()
    _save_sweep(out, problems, output_name, lambda i: "_interpolated", bfs_step_height)
    return out


def run_interpolated_fine_simulations(coarse_fields_list: Sequence[Dict[str, np.ndarray]], reynolds: Sequence[float], nx: int, ny: int,
                                      lr_dim: int = 10, dt: float = 0.001, scheme: str = "QUICK",
                                      convergence_criteria: Optional[Dict[str, float]] = None, max_iterations_fine: int = 100000,
                                      output_name: Optional[str] = None, bc=None, resident=False, pressure: str = "sweeps", max_batch: int = 8,
                                      device: int = 0) -> list:
    """The control arm of a warm-start study: `run_ml_accelerated_fine_simulations` with the network replaced by plain bicubic
    interpolation of each coarse field to the mesh (`interpolation_resampler`), on the device.  The arguments are those of that
    function without the model and statistics files and the network's precision; the return value is the same list of (fields,
    iterations, status).  `output_name`: each case's fields go to `{output_name}_Re{Re}_interpolated.h5`."""
    reynolds = list(reynolds)
    bcs = _per_case(bc, len(reynolds))
    pbs = [problem(Re, nx, ny, 1.0, 1.0, dt, scheme, convergence_criteria or _DEFAULT_CC, b) for Re, b in zip(reynolds, bcs)]
    return _interpolated_sweep(coarse_fields_list, reynolds, pbs, lr_dim, max_iterations_fine, output_name, max_batch, device, resident, pressure=pressure)


def run_bfs_interpolated_fine_simulations(coarse_fields_list: Sequence[Dict[str, np.ndarray]], reynolds: Sequence[float], nx: int, ny: int,
                                          lr_dim: int = 10, dt: float = 0.002, scheme: str = "UPWIND",
                                          convergence_criteria: Optional[Dict[str, float]] = None, max_iterations_fine: int = 100000,
                                          output_name: Optional[str] = None, bc=None, step_height: float = 1.0, h: float = 2.0,
                                          Ub: float = 1.0, lx: float = 10.0, ly: float = 3.0,
                                          relaxation_factors: Optional[Dict[str, float]] = None, resident=False, pressure: str = "sweeps", max_batch: int = 8,
                                          device: int = 0) -> list:
    """`run_interpolated_fine_simulations` for the backward-facing step: `run_bfs_ml_accelerated_fine_simulations` without the
    model, its files and its input options."""
    reynolds = list(reynolds)
    bcs = _per_case(bc, len(reynolds))
    pbs = [_bfs_problem(Re, nx, ny, dt, scheme, convergence_criteria, b, step_height, h, Ub, lx, ly, relaxation_factors)
           for Re, b in zip(reynolds, bcs)]
    return _interpolated_sweep(coarse_fields_list, reynolds, pbs, lr_dim, max_iterations_fine, output_name, max_batch, device, resident,
                               bfs_step_height=step_height, pressure=pressure)


ARMS = ("ml", "interp", "zero")


def _warm_start_arms(coarse_fields_list, reynolds, problem_of, arms, lr_dim, files, default_files, prepare_of, max_iterations,
                     output_name, max_batch, device, resident, bfs_step_height=None, pressure="sweeps"):
    """The solve behind `compare_warm_starts` and its BFS form.  problem_of(i): the problem of Reynolds number i; prepare_of(files,
    device): pipeline._prepare_batch for a list of coarse fields."""
    from . import pipeline
    reynolds, coarse_fields_list, arms = list(reynolds), list(coarse_fields_list), tuple(arms)
    if not arms or len(set(arms)) != len(arms) or any(a not in ARMS for a in arms):
        raise ValueError(f"arms must be distinct names out of {ARMS}, not {arms}")
    if len(coarse_fields_list) != len(reynolds):
        raise ValueError(f"coarse_fields_list must hold one set of coarse fields per Reynolds number ({len(reynolds)}), not {len(coarse_fields_list)}")
    if "ml" in arms:
        if all(f is None for f in files):
            arms = tuple(a for a in arms if a != "ml")       # no model files: the arms that need none
            if not arms:
                raise ValueError("the 'ml' arm needs stats_file, encoder_file and decoder_file")
        else:
            files = tuple(f or d for f, d in zip(files, default_files))
            _model_files(*files)
    every = len(arms)
    if max_batch < every:
        raise ValueError(f"max_batch must be at least {every}, the number of arms")
    problems = [problem_of(i) for i in range(len(reynolds)) for _ in arms]
    prepare = model = None
    if "ml" in arms:
        prepare = prepare_of(files, device)
        model = prepare([])[0]   # the handle is cached: this picks the device before any solver exists
        device = model.device
    device = 0 if device is None else int(device)
    pb = problems[0] if problems else None
    interp = interpolation_resampler(lr_dim, lr_dim, pb.nx, pb.ny, pb.lx, pb.ly, device) if "interp" in arms and pb is not None else None

    def warm_start(b, a):
        import torch
        first, n_re = a // every, b.n_cases // every
        coarse = coarse_fields_list[first:first + n_re]
        parts, cases = [], []
        if "ml" in arms:
            # the prediction of these n_re fields goes into the state exactly as the ML sweep puts it there; its float64 copy then
            # joins the other arms' fields, because every init call starts the cases it does not name from zero
            ml_cases = [every * i + arms.index("ml") for i in range(n_re)]
            _, x, ain, aout, back = prepare(coarse)
            pipeline._warn_nonfinite(b.init_from_prediction(model, x, ain, aout, back, cases=ml_cases))
            parts.append(b.fields_device(cases=ml_cases))
            cases += ml_cases
        if "interp" in arms:
            lr = torch.from_numpy(_stack_fields(coarse)).to(torch.device("cuda", device))
            parts.append(interp.apply_device_f64(lr))
            cases += [every * i + arms.index("interp") for i in range(n_re)]
        if cases:
            b.init_from_fields(parts[0] if len(parts) == 1 else torch.cat(parts), cases=cases)

    try:
        out = _solve_in_batches(problems, max_iterations, max_batch - max_batch % every, device, warm_start, resident=resident, pressure=pressure)
    finally:
        if interp is not None:
            interp.close()
    _save_sweep(out, problems, output_name, lambda i: f"_{arms[i % every]}", bfs_step_height)
    res = []
    for i, Re in enumerate(reynolds):
        r = {"Re": Re}
        for k, arm in enumerate(arms):
            fields, it, st = out[every * i + k]
            r[arm] = {"iterations": it, "status": st, "fields": fields}
        r["iterations_saved"] = {arm: r["zero"]["iterations"] - r[arm]["iterations"] for arm in arms if arm != "zero"} if "zero" in arms else {}
        res.append(r)
    return res


def compare_warm_starts(coarse_fields_list: Sequence[Dict[str, np.ndarray]], reynolds: Sequence[float], nx: int, ny: int,
                        arms: Sequence[str] = ARMS, lr_dim: int = 10, dt: float = 0.001, scheme: str = "QUICK",
                        convergence_criteria: Optional[Dict[str, float]] = None, max_iterations_fine: int = 100000,
                        output_name: Optional[str] = None, stats_file: Optional[str] = None, encoder_file: Optional[str] = None,
                        decoder_file: Optional[str] = None, bc=None, precision: Optional[str] = None, resident=False, pressure: str = "sweeps",
                        max_batch: int = 8, device: Optional[int] = None) -> list:
    """`compare_ml_and_normal_simulations` with the control arm: every Reynolds number goes into the batch once per arm -- "ml"
    warm-started from the network, "interp" from the plainly interpolated coarse field (`run_interpolated_fine_simulations`),
    "zero" from zero fields -- under the same iteration cap; `max_batch` is rounded down to a multiple of the number of arms.
    Without any of stats_file, encoder_file and decoder_file the "ml" arm is left out and the others run; with some of them
    given, the missing ones take the defaults of `run_ml_accelerated_fine_simulations` and all three must exist.
    Returns one dict per Reynolds number: Re, one {"iterations", "status", "fields"} per arm under the arm's name, and
    iterations_saved[arm] = zero's iterations - the arm's, for every other arm when "zero" runs.  Each arm has the bits of its
    own sweep function; the "ml" arm's prediction holds one field per Reynolds number of the batch (see
    FineSolverBatch.init_from_prediction).  `output_name`: fields go to `{output_name}_Re{Re}_{arm}.h5`."""
    from . import pipeline
    reynolds = list(reynolds)
    bcs = _per_case(bc, len(reynolds))
    defaults = (f"standardization_stats_{lr_dim}to{nx}.txt", f"vanilla_encoder{lr_dim}_to_{nx}.h5", f"vanilla_decoder{nx}_from_{lr_dim}.h5")
    prepare_of = lambda files, dev: (lambda fields: pipeline._prepare_batch(fields, lr_dim, nx, files[0], files[1], files[2], False, 1.0, 1.0,
                                                                           False, 0.3, precision, dev))
    return _warm_start_arms(coarse_fields_list, reynolds,
                            lambda i: problem(reynolds[i], nx, ny, 1.0, 1.0, dt, scheme, convergence_criteria or _DEFAULT_CC, bcs[i]),
                            arms, lr_dim, (stats_file, encoder_file, decoder_file), defaults, prepare_of, max_iterations_fine, output_name,
                            max_batch, device, resident, pressure=pressure)


def compare_bfs_warm_starts(coarse_fields_list: Sequence[Dict[str, np.ndarray]], reynolds: Sequence[float], nx: int, ny: int,
                            arms: Sequence[str] = ARMS, lr_dim: int = 10, dt: float = 0.002, scheme: str = "UPWIND",
                            convergence_criteria: Optional[Dict[str, float]] = None, max_iterations_fine: int = 100000,
                            output_name: Optional[str] = None, stats_file: Optional[str] = None, encoder_file: Optional[str] = None,
                            decoder_file: Optional[str] = None, bc=None, step_height: float = 1.0, h: float = 2.0, Ub: float = 1.0,
                            lx: float = 10.0, ly: float = 3.0, relaxation_factors: Optional[Dict[str, float]] = None,
                            use_aspect_ratio_correction: bool = False, use_adaptive_normalization: bool = True,
                            blend_factor: float = 0.3, precision: Optional[str] = None, resident=False, pressure: str = "sweeps", max_batch: int = 8,
                            device: Optional[int] = None) -> list:
    """`compare_warm_starts` for the backward-facing step (the arms of `run_bfs_ml_accelerated_fine_simulations`,
    `run_bfs_interpolated_fine_simulations` and `run_bfs_normal_simulations`)."""
    from . import pipeline
    reynolds = list(reynolds)
    bcs = _per_case(bc, len(reynolds))
    tail = "_swish_trained_upto_700_multiBC"
    defaults = (f"standardization_stats_{lr_dim}to{nx}{tail}.txt", f"vanilla_encoder{lr_dim}_to_{nx}{tail}.h5",
                f"vanilla_decoder{nx}_from_{lr_dim}{tail}.h5")
    prepare_of = lambda files, dev: (lambda fields: pipeline._prepare_batch(fields, lr_dim, nx, files[0], files[1], files[2],
                                                                           use_aspect_ratio_correction, lx, ly, use_adaptive_normalization,
                                                                           blend_factor, precision, dev))
    return _warm_start_arms(coarse_fields_list, reynolds,
                            lambda i: _bfs_problem(reynolds[i], nx, ny, dt, scheme, convergence_criteria, bcs[i], step_height, h, Ub, lx, ly,
                                                   relaxation_factors),
                            arms, lr_dim, (stats_file, encoder_file, decoder_file), defaults, prepare_of, max_iterations_fine, output_name,
                            max_batch, device, resident, bfs_step_height=step_height, pressure=pressure)


def run_nested_simulations(reynolds: Sequence[float], meshes: Sequence, dt: float = 0.001, scheme: str = "QUICK",
                           convergence_criteria: Optional[Dict[str, float]] = None, max_iterations=100000, bc=None, max_batch: int = 8,
                           device: int = 0, resident=False, pressure: str = "sweeps") -> list:
    """Grid sequencing (nested iteration) of the lid-driven cavity, the network-free accelerator: `meshes` lists (nx, ny) from
    coarse to fine; level 0 starts from zero fields, and level l from level l - 1's result, interpolated to its mesh
    (`interpolation_resampler`, float64) on the device -- `fields_device` -> `init_from_fields`; no field crosses to the host
    between levels.  `max_iterations`: the cap of every level, or one cap per level.  `resident`: as
    FineSolverBatch.set_resident, per level ("auto" runs the small levels resident).  Returns one dict per Reynolds number: Re,
    fields (the last level's (ny, nx) u, v, p), and iterations and status, one entry per level.  A case that diverges on a
    level passes its non-finite fields on and diverges on the next."""
    reynolds, meshes = list(reynolds), [(int(m[0]), int(m[1])) for m in meshes]
    if not meshes:
        raise ValueError("meshes must list at least one (nx, ny)")
    caps = [int(max_iterations)] * len(meshes) if np.isscalar(max_iterations) else [int(m) for m in max_iterations]
    if len(caps) != len(meshes):
        raise ValueError(f"max_iterations must be one cap or one per level ({len(meshes)}), not {len(caps)}")
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    bcs = _per_case(bc, len(reynolds))
    res = [{"Re": Re, "fields": None, "iterations": [], "status": []} for Re in reynolds]
    for a in range(0, len(reynolds), max_batch):
        z = slice(a, a + max_batch)
        prev, prev_mesh = None, None
        for level, ((nx, ny), cap) in enumerate(zip(meshes, caps)):
            pbs = [problem(Re, nx, ny, 1.0, 1.0, dt, scheme, convergence_criteria or _DEFAULT_CC, b) for Re, b in zip(reynolds[z], bcs[z])]
            b = FineSolverBatch(pbs, cap, device, resident=resident, pressure=pressure)
            try:
                if prev is not None:
                    up = interpolation_resampler(prev_mesh[1], prev_mesh[0], nx, ny, 1.0, 1.0, device)
                    try:
                        b.init_from_fields(prev, resampler=up)
                    finally:
                        up.close()
                b.solve()
                for i, r in enumerate(res[z]):
                    r["iterations"].append(int(b.iterations[i]))
                    r["status"].append(int(b.status[i]))
                if level + 1 < len(meshes):
                    prev, prev_mesh = b.fields_device(), (nx, ny)
                else:
                    for i, r in enumerate(res[z]):
                        r["fields"] = b.fields(i)
            finally:
                b.close()
    return res
