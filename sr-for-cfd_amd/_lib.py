"""ctypes binding of libsrcfd.so (C ABI in include/srcfd.h).

The library is the product: if it is missing or cannot be loaded this module
raises -- there is no Python/CPU fallback for the compute path.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRCFD_LIB") or os.path.join(_HERE, "lib", "libsrcfd.so")  # SRCFD_LIB: A/B builds of the same ABI

OK, ENOENT, EIO, ENOMEM, ENODEV, EINVAL, EKEY, EHIP = 0, -2, -5, -12, -19, -22, -126, -1000

F32, F64, I32, I64, U8, STR, BF16, F16 = 0, 1, 2, 3, 4, 5, 16, 17
PREC_FP32, PREC_BF16, PREC_FP32_NAIVE, PREC_F16, PREC_FP32X3 = 0, 1, 2, 3, 4
TRAIN_OVERWRITE = 1   # srcfd_trainer_forward_backward_ex: grads and sse are written, not added into
TRAIN_SAME_PARAMS = 2  # ... params unchanged since this trainer's previous call: the operand re-packing is skipped
LAYER_CONV2D, LAYER_CONV2D_TRANSPOSE, LAYER_DENSE, LAYER_FLATTEN, LAYER_RESHAPE = 1, 2, 3, 4, 5
ACT_LINEAR, ACT_SWISH, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3, 4
FLAG_NAN_GUARD = 1
CASE_RUNNING, CASE_CONVERGED, CASE_DIVERGED = 0, 1, 2
FINE_MODE_LAUNCHES, FINE_MODE_RESIDENT = 0, 1
PRESSURE_SWEEPS, PRESSURE_DIRECT = 0, 1
PRESSURE_SOLVERS = {"sweeps": PRESSURE_SWEEPS, "direct": PRESSURE_DIRECT}
SCORE_FIELDS = 8   # srcfd_score_fields / srcfd_evalset_score: float32 values per sample, in this order
SCORE_NAMES = ("mae", "mse", "max_abs", "truth_min", "truth_max", "pred_min", "pred_max", "nonfinite")


class SrcfdError(RuntimeError):
    """Any libsrcfd failure that has no closer built-in exception type."""


class NoDeviceError(SrcfdError):
    """No HIP device (SRCFD_ENODEV): the extension cannot compute here."""


class Layer(C.Structure):
    _fields_ = [
        ("kind", C.c_int), ("activation", C.c_int),
        ("kh", C.c_int), ("kw", C.c_int), ("stride", C.c_int), ("same_padding", C.c_int),
        ("cin", C.c_int), ("cout", C.c_int),
        ("reshape", C.c_int * 3),
        ("kernel", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float)),
        ("name", C.c_char_p),
    ]


class CoarseProblem(C.Structure):
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("lx", C.c_double), ("ly", C.c_double),
                ("reynolds", C.c_double), ("rho", C.c_double), ("dt", C.c_double),
                ("scheme", C.c_int), ("max_iterations", C.c_int), ("tolerance", C.c_double * 3),
                ("bc_type", (C.c_int * 4) * 3), ("bc_value", (C.c_double * 4) * 3),
                ("case_type", C.c_int), ("relax", C.c_double * 3),
                ("step_height", C.c_double), ("channel_height", C.c_double), ("bulk_velocity", C.c_double)]


class SolverBC(C.Structure):
    _fields_ = [("type", C.c_int * 4), ("value", C.c_double * 4), ("left_profile", C.POINTER(C.c_double))]


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C sr-for-cfd_amd/csrc` (hipcc, --offload-arch=gfx950). There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    return C.CDLL(LIB_PATH)


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (soname
    libamdhip64.so.7) and links it by the unversioned name; libsrcfd needs `libamdhip64.so.7`.
    Whichever loads first decides whether the second resolves to the same object: torch first is
    fine, libsrcfd first would bring in /opt/rocm's copy and torch then loads a second runtime that
    finds no devices.  So when torch is installed (not necessarily imported), map its copy first."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


lib = _load()

_p = C.c_void_p
_sz = C.c_size_t
_protos = {
    "srcfd_last_error": (C.c_char_p, []),
    "srcfd_version": (C.c_char_p, []),
    "srcfd_device_count": (C.c_int, []),
    "srcfd_model_load_h5": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(_p)]),
    "srcfd_model_create": (C.c_int, [C.POINTER(Layer), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(_p)]),
    "srcfd_model_destroy": (None, [_p]),
    "srcfd_model_input_shape": (C.c_int, [_p, C.POINTER(C.c_int)]),
    "srcfd_model_output_shape": (C.c_int, [_p, C.POINTER(C.c_int)]),
    "srcfd_model_num_layers": (C.c_int, [_p]),
    "srcfd_model_get_layer": (C.c_int, [_p, C.c_int, C.POINTER(Layer), C.c_char_p, _sz]),
    "srcfd_model_macs_per_sample": (C.c_int64, [_p]),
    "srcfd_model_set_precision": (C.c_int, [_p, C.c_int]),
    "srcfd_model_get_precision": (C.c_int, [_p]),
    "srcfd_model_reserve": (C.c_int, [_p, C.c_int]),
    "srcfd_model_has_fused_path": (C.c_int, [_p]),
    "srcfd_model_supports_precision": (C.c_int, [_p, C.c_int]),
    "srcfd_predict": (C.c_int, [_p, _p, C.c_int, _p, _p, _p, C.c_int, C.POINTER(C.c_int64)]),
    "srcfd_predict_device": (C.c_int, [_p, _p, C.c_int, _p, _p, _p, C.c_int, C.c_int, _p, _p]),
    "srcfd_model_workspace": (C.c_int, [_p, C.c_int, C.POINTER(_sz)]),
    "srcfd_model_footprint": (C.c_int, [_p, C.c_int, C.c_int, C.POINTER(_sz)]),
    "srcfd_model_set_profiling": (C.c_int, [_p, C.c_int]),
    "srcfd_model_get_profile": (C.c_int, [_p, C.c_char_p, _sz, C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int]),
    "srcfd_model_debug_activation": (C.c_int, [_p, C.c_int, _p, _sz]),
    "srcfd_model_last_plan": (C.c_int, [_p, C.c_char_p, _sz]),
    "srcfd_model_f32_steps": (C.c_int, [_p, C.c_int, C.c_char_p, _sz]),
    "srcfd_host_alloc": (C.c_int, [_sz, C.POINTER(C.c_void_p)]),
    "srcfd_host_free": (None, [_p]),
    "srcfd_model_save_h5": (C.c_int, [_p, C.c_char_p, C.c_char_p]),
    "srcfd_resampler_create": (C.c_int, [C.c_int, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_p)]),
    "srcfd_resampler_destroy": (None, [_p]),
    "srcfd_resample_device": (C.c_int, [_p, _p, C.c_int, _p, _p]),
    "srcfd_resample_device_f64": (C.c_int, [_p, _p, C.c_int, _p, _p]),
    "srcfd_predict_resampled": (C.c_int, [_p, _p, _p, C.c_int, _p, _p, _p, C.c_int, C.POINTER(C.c_int64)]),
    "srcfd_predict_into_solver_state": (C.c_int, [_p, _p, _p, _p, _p, C.POINTER(SolverBC), _p, C.c_int, C.POINTER(C.c_int64)]),
    "srcfd_trainer_create": (C.c_int, [_p, C.c_int, C.POINTER(_p)]),
    "srcfd_trainer_destroy": (None, [_p]),
    "srcfd_trainer_num_params": (C.c_int64, [_p]),
    "srcfd_trainer_get_params": (C.c_int, [_p, _p]),
    "srcfd_trainer_get_plan": (C.c_int, [_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "srcfd_trainer_last_step": (C.c_int, [_p] + [C.POINTER(C.c_int)] * 5),
    "srcfd_trainer_forward_backward": (C.c_int, [_p, _p, _p, _p, C.c_int, C.c_float, _p, _p, _p]),
    "srcfd_trainer_forward_backward_ex": (C.c_int, [_p, _p, _p, _p, C.c_int, C.c_float, _p, _p, C.c_int, _p]),
    "srcfd_model_save_superres_h5": (C.c_int, [_p, C.c_char_p]),
    "srcfd_model_load_superres_h5": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_p)]),
    "srcfd_prepare_inputs_device": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _p, _p, C.c_int, _p, C.c_int, C.c_double, _p, _p, _p]),
    "srcfd_coarse_solve": (C.c_int, [C.POINTER(CoarseProblem), _p, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "srcfd_fine_solver_create": (C.c_int, [C.POINTER(CoarseProblem), C.c_int, C.POINTER(_p)]),
    "srcfd_fine_solver_destroy": (None, [_p]),
    "srcfd_fine_solver_init": (C.c_int, [_p, _p]),
    "srcfd_fine_solver_init_from_prediction": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.POINTER(C.c_int64)]),
    "srcfd_fine_solver_run": (C.c_int, [_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), _p, C.c_int]),
    "srcfd_fine_solver_get_state": (C.c_int, [_p, _p]),
    "srcfd_fine_solver_counters": (C.c_int, [_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "srcfd_fine_batch_create": (C.c_int, [C.POINTER(CoarseProblem), C.c_int, C.c_int, C.POINTER(_p)]),
    "srcfd_fine_batch_destroy": (None, [_p]),
    "srcfd_fine_batch_init": (C.c_int, [_p, _p]),
    "srcfd_fine_batch_init_from_prediction": (C.c_int, [_p, _p, _p, _p, C.c_int, C.POINTER(C.c_int), _p, _p, C.c_int, C.POINTER(C.c_int64)]),
    "srcfd_fine_batch_init_from_fields_device": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, C.POINTER(C.c_int), _p]),
    "srcfd_fine_batch_get_fields_device": (C.c_int, [_p, C.c_int, C.POINTER(C.c_int), _p, C.c_int, _p]),
    "srcfd_fine_solver_init_from_fields_device": (C.c_int, [_p, _p, _p, C.c_int, _p]),
    "srcfd_fine_solver_get_fields_device": (C.c_int, [_p, _p, C.c_int, _p]),
    "srcfd_fine_batch_run": (C.c_int, [_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _p, _p, C.c_int]),
    "srcfd_fine_batch_get_state": (C.c_int, [_p, C.c_int, _p]),
    "srcfd_fine_batch_counters": (C.c_int, [_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "srcfd_fine_batch_footprint": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "srcfd_fine_resident_supported": (C.c_int, [C.c_int, C.c_int]),
    "srcfd_fine_batch_set_mode": (C.c_int, [_p, C.c_int]),
    "srcfd_fine_solver_set_mode": (C.c_int, [_p, C.c_int]),
    "srcfd_fine_batch_set_pressure_solver": (C.c_int, [_p, C.c_int]),
    "srcfd_fine_solver_set_pressure_solver": (C.c_int, [_p, C.c_int]),
    "srcfd_poisson_basis": (C.c_int, [C.c_int, _p, _p]),
    "srcfd_adam_step": (C.c_int, [_p, _p, _p, _p, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _p]),
    "srcfd_stats_load": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "srcfd_stats_save": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "srcfd_h5_open": (C.c_int, [C.c_char_p, C.POINTER(_p)]),
    "srcfd_h5_close": (None, [_p]),
    "srcfd_h5_list": (C.c_int, [_p, C.c_char_p, C.c_char_p, _sz, C.POINTER(_sz)]),
    "srcfd_h5_kind": (C.c_int, [_p, C.c_char_p]),
    "srcfd_h5_dataset_info": (C.c_int, [_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "srcfd_h5_read": (C.c_int, [_p, C.c_char_p, _p, _sz, C.c_int]),
    "srcfd_h5_attr_string": (C.c_int, [_p, C.c_char_p, C.c_char_p, C.c_char_p, _sz, C.POINTER(_sz)]),
    "srcfd_h5_attr_numeric": (C.c_int, [_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
    "srcfd_h5_attr_names": (C.c_int, [_p, C.c_char_p, C.c_char_p, _sz, C.POINTER(_sz)]),
    "srcfd_h5w_create": (C.c_int, [C.POINTER(_p)]),
    "srcfd_h5w_free": (None, [_p]),
    "srcfd_h5w_group": (C.c_int, [_p, C.c_char_p]),
    "srcfd_h5w_dataset": (C.c_int, [_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), _p]),
    "srcfd_h5w_attr_strings": (C.c_int, [_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]),
    "srcfd_h5w_attr_numeric": (C.c_int, [_p, C.c_char_p, C.c_char_p, C.c_int, _p, C.c_int, C.c_int]),
    "srcfd_h5w_save": (C.c_int, [_p, C.c_char_p]),
    "srcfd_score_plan": (C.c_int, [C.c_int64, C.c_char_p, _sz]),
    "srcfd_score_fields": (C.c_int, [C.c_int, _p, _p, C.c_int, C.c_int64, _p, _p, _p]),
    "srcfd_evalset_create": (C.c_int, [C.c_int, _p, C.c_int64, _p, C.c_int64, C.c_int, _p, _p, _p, C.POINTER(_p)]),
    "srcfd_evalset_score": (C.c_int, [_p, _p, _p]),
    "srcfd_evalset_destroy": (C.c_int, [_p]),
    "srcfd_tiled_plan": (C.c_int, [C.c_int] * 12 + [C.c_char_p, _sz]),
    "srcfd_tiler_create": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_p)]),
    "srcfd_tiled_plan_overlap": (C.c_int, [C.c_int] * 14 + [C.c_char_p, _sz]),
    "srcfd_tiler_create_overlap": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_p)]),
    "srcfd_tiler_destroy": (None, [_p]),
    "srcfd_tiler_set_stream": (C.c_int, [_p, _p]),
    "srcfd_tiler_run": (C.c_int, [_p, _p, _p, _p, _p, C.c_int, _p]),
    "srcfd_tiles_cut_device": (C.c_int, [_p, _p, _p, _p, _p, _p, _p]),
    "srcfd_tiles_stitch_device": (C.c_int, [_p, _p, C.c_int64, _p, C.c_int, C.c_int, _p]),
}
for _name, (_res, _args) in _protos.items():
    _fn = getattr(lib, _name)  # AttributeError here = ABI drift, fail loudly
    _fn.restype = _res
    _fn.argtypes = _args

EXPORTED = tuple(_protos)


def last_error() -> str:
    return (lib.srcfd_last_error() or b"").decode("utf-8", "replace")


def check(rc: int) -> int:
    """Map a status code to the exception the reference's Python would raise
    (SURVEY.md 8b 'errors')."""
    if rc >= 0:
        return rc
    msg = last_error()
    if rc == ENOENT:
        raise FileNotFoundError(msg)
    if rc == EIO:
        raise OSError(msg)
    if rc == EKEY:
        raise KeyError(msg)
    if rc == EINVAL:
        raise ValueError(msg)
    if rc == ENOMEM:
        raise MemoryError(msg)
    if rc == ENODEV:
        raise NoDeviceError(msg)
    raise SrcfdError(f"libsrcfd error {rc}: {msg}")


def enc(path) -> bytes:
    return os.fsencode(path)


def _squeezed(shape) -> tuple:
    return tuple(int(d) for d in shape if int(d) != 1)


def device_ptr(t, what: str, dtype=None, shape=None, device=None, optional: bool = False, exact: bool = False, min_numel: int = 0):
    """The one place a torch CUDA tensor becomes the `void*` of a libsrcfd device entry (include/srcfd.h, "device pointers": every
    device pointer is a dense C-ordered array of its element type, aligned to that element).  Returns the `c_void_p`; raises
    ValueError that names `what` and the offending property when `t`
      * is None and not `optional` (with `optional`, None gives None: the entry's "no such argument");
      * is not a CUDA tensor, or is on a device other than index `device`;
      * has a dtype other than `dtype` (one dtype or a tuple of accepted ones);
      * has the wrong shape or is not contiguous.
    shape = (n, *per_sample): the first dimension is n, the remaining ones equal the per-sample shape once dimensions of size 1 are
    dropped on both sides -- `y.view(n, hr, hr)` for an (hr, hr, 1) output and `y[:n]` are legal, a channel slice or a transposed
    view is not.  exact=True: the shape as it stands.  n == 0 with a zero-row tensor passes as it is: the entry launches nothing
    and the pointer is never followed.  min_numel: for an argument without a shape (a counter), the fewest elements.
    Only attributes are read (is_cuda, device.index, dtype, shape, is_contiguous(), data_ptr()): nothing is enqueued or synchronised."""
    if t is None:
        if optional:
            return None
        raise ValueError(f"{what} is required, got None")
    if not getattr(t, "is_cuda", False):
        raise ValueError(f"{what} must be a CUDA tensor, got {type(t).__name__}" + (f" on {t.device}" if hasattr(t, "device") else ""))
    if device is not None and t.device.index != int(device):
        raise ValueError(f"{what} is on device cuda:{t.device.index}, the handle is on cuda:{int(device)}")
    if dtype is not None:
        accepted = tuple(dtype) if isinstance(dtype, (tuple, list)) else (dtype,)
        if t.dtype not in accepted:
            raise ValueError(f"{what} has dtype {t.dtype}, expected {' or '.join(str(d) for d in accepted)}")
    got = tuple(int(d) for d in t.shape)
    if shape is not None:
        shape = tuple(int(d) for d in shape)
        if exact:
            if got != shape:
                raise ValueError(f"{what} has shape {got}, expected {shape}")
        else:
            if not got or got[0] != shape[0]:
                raise ValueError(f"{what} has shape {got}: its first dimension must be n = {shape[0]} (expected (n, *{shape[1:]}))")
            if shape[0] == 0:
                return C.c_void_p(t.data_ptr())
            if _squeezed(got[1:]) != _squeezed(shape[1:]):
                raise ValueError(f"{what} has per-sample shape {got[1:]}, expected {shape[1:]} (dimensions of size 1 aside)")
    if min_numel:
        numel = 1
        for d in got:
            numel *= d
        if numel < min_numel:
            raise ValueError(f"{what} has {numel} element(s), needs at least {min_numel}")
    if not t.is_contiguous():
        raise ValueError(f"{what} is not contiguous (shape {got}, strides {tuple(t.stride())}): the library reads and writes dense "
                         "C-ordered memory; pass t.contiguous()")
    return C.c_void_p(t.data_ptr())
