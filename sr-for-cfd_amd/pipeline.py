"""Counterpart of the reference's `ml_super_resolution` (the one call the solvers make
between the coarse and the fine solve), on libsrcfd.

    PyCFD_ML_accelerated.py:764-879   ml_super_resolution(coarse_fields, lr_dim, hr_dim,
                                          stats_file, encoder_file, decoder_file)
    bfs_ml_accelerated.py:979-1137    same + use_aspect_ratio_correction, lx, ly,
                                          use_adaptive_normalization=True, blend_factor=0.3

Order of operations is the reference's: float32 cast, [BFS: spline resample to a
square], stats lookup, [BFS: adaptive blend], standardise, predict, de-standardise
with the *training* HR stats, NaN/Inf zero-fill, [BFS: resample back].  Standardise,
the network, de-standardise and the guard run as one device call for the three
components.  The BFS resample back to the rectangle (a bicubic spline fit of a 400x400
field per component in the reference) runs on the device as two float64 matrix products
(resample.py); the 10x10 statistics and the 10x10 pre-resampling stay on the host.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, Optional

import numpy as np

from . import keras_compat as kc
from .stats import load_stats

COMPONENTS = ("u", "v", "p")


def standardize_with_stats(arr, mean, std):
    """PyCFD_ML_accelerated.py:665-668."""
    std = 1e-8 if std == 0 else std
    return (arr - mean) / std


def inverse_standardize(arr, mean, std):
    """PyCFD_ML_accelerated.py:671-673."""
    return arr * std + mean


def reshape_rectangular_to_square(fields, nx_rect, ny_rect, lx, ly):
    """bfs_ml_accelerated.py:59-101 (bicubic RectBivariateSpline onto linspace(0,max(lx,ly))^2)."""
    from scipy import interpolate
    x_rect, y_rect = np.linspace(0, lx, nx_rect), np.linspace(0, ly, ny_rect)
    L = max(lx, ly)
    x_sq, y_sq = np.linspace(0, L, nx_rect), np.linspace(0, L, nx_rect)
    out = {}
    for c in COMPONENTS:
        out[c] = interpolate.RectBivariateSpline(y_rect, x_rect, fields[c], kx=3, ky=3)(y_sq, x_sq)
    return out


def reshape_square_to_rectangular(fields, nx_rect, ny_rect, lx, ly):
    """bfs_ml_accelerated.py:104-145."""
    from scipy import interpolate
    n = fields["u"].shape[0]
    L = max(lx, ly)
    x_sq, y_sq = np.linspace(0, L, n), np.linspace(0, L, n)
    x_rect, y_rect = np.linspace(0, lx, nx_rect), np.linspace(0, ly, ny_rect)
    out = {}
    for c in COMPONENTS:
        out[c] = interpolate.RectBivariateSpline(y_sq, x_sq, fields[c], kx=3, ky=3)(y_rect, x_rect)
    return out


def _case_inputs(coarse_fields, lr_dim, stats_lr, stats_hr, use_aspect_ratio_correction, lx, ly, use_adaptive_normalization, blend_factor,
                 say):
    """The part of `_prepare` that depends on the coarse field (PyCFD...:787-857 / bfs...:1025-1108): the (3,lr,lr,1) float32
    batch, the per-component (mean,std) pairs in and out, and the fields the batch was cast from."""
    fields = coarse_fields
    if use_aspect_ratio_correction and lx != ly:
        # reshape_rectangular_to_square (bfs_ml_accelerated.py:59-101) as two cached 1-D spline matrices: the same
        # interpolating bicubic spline as scipy's RectBivariateSpline to ~1e-15 (tests/test_resample.py), without three
        # FITPACK fits per call
        from . import resample as rs
        Ry, Rx = rs.rect_to_square_matrices(lr_dim, lr_dim, float(lx), float(ly))
        fields = {c: Ry @ np.asarray(coarse_fields[c], np.float64) @ Rx.T for c in COMPONENTS}
    x = np.empty((3, lr_dim, lr_dim, 1), np.float32)
    ain = np.empty((3, 2), np.float32)
    aout = np.empty((3, 2), np.float32)
    for i, c in enumerate(COMPONENTS):
        x[i, :, :, 0] = fields[c]  # == np.asarray(fields[c]).astype(np.float32)
    if use_adaptive_normalization:
        # np.mean / np.std of each component's float32 array (bfs_ml_accelerated.py:1091-1092), as two row reductions over
        # the stacked batch instead of six calls: same pairwise sums, bit-identical (tests/test_dropin.py)
        rows = x.reshape(3, -1)
        input_means, input_stds = rows.mean(axis=1), rows.std(axis=1)
    for i, c in enumerate(COMPONENTS):
        mean_lr, std_lr = stats_lr[c]
        if use_adaptive_normalization:  # bfs_ml_accelerated.py:1093-1097, same expressions
            input_mean, input_std = input_means[i], input_stds[i]
            mean_lr = (1 - blend_factor) * mean_lr + blend_factor * input_mean
            std_lr = (1 - blend_factor) * std_lr + blend_factor * max(input_std, 1e-8)
            if say is not _quiet:
                say(f"  {c.upper()}: adaptive norm (blend={blend_factor:.2f}) mean={float(mean_lr):.6f} std={float(std_lr):.6f}")
        ain[i] = (mean_lr, std_lr)
        aout[i] = stats_hr[c]
    return x, ain, aout, fields


def _prepare_list(coarse_fields_list, lr_dim, hr_dim, stats_file, encoder_file, decoder_file, use_aspect_ratio_correction, lx, ly,
                  use_adaptive_normalization, blend_factor, precision, say, device=None):
    """Everything before `predict` for a list of coarse fields: the model handle, the resampler for the way back (or None),
    and per field what `_case_inputs` returns."""
    stats_lr, stats_hr = load_stats(stats_file, lr_dim, hr_dim)  # FileNotFoundError / KeyError like :819-825
    for f in (encoder_file, decoder_file):  # the callers pre-check this (:1080-1087); load_model would raise too
        if not os.path.exists(f):
            raise FileNotFoundError(f"model file '{f}' not found")
    model = kc._device_handle((os.fspath(encoder_file), os.fspath(decoder_file)), precision or kc._DEFAULT_PRECISION, device)
    per_case = [_case_inputs(cf, lr_dim, stats_lr, stats_hr, use_aspect_ratio_correction, lx, ly, use_adaptive_normalization, blend_factor,
                             say) for cf in coarse_fields_list]
    back = None
    if use_aspect_ratio_correction and lx != ly:
        from . import resample as rs
        back = rs.square_to_rect_resampler(hr_dim, hr_dim, hr_dim, float(lx), float(ly), model.device)
    return model, back, per_case


def _prepare(coarse_fields, lr_dim, hr_dim, stats_file, encoder_file, decoder_file, use_aspect_ratio_correction, lx, ly,
             use_adaptive_normalization, blend_factor, precision, say):
    """Everything before `predict` (PyCFD...:787-857 / bfs...:1025-1108): model handle, the (3,lr,lr,1) float32
    batch, the per-component (mean,std) pairs in and out, and the resampler for the way back (or None)."""
    model, back, ((x, ain, aout, fields),) = _prepare_list([coarse_fields], lr_dim, hr_dim, stats_file, encoder_file, decoder_file,
                                                           use_aspect_ratio_correction, lx, ly, use_adaptive_normalization, blend_factor,
                                                           precision, say)
    return model, x, ain, aout, back, fields


def _prepare_batch(coarse_fields_list, lr_dim, hr_dim, stats_file, encoder_file, decoder_file, use_aspect_ratio_correction, lx, ly,
                   use_adaptive_normalization, blend_factor, precision, device=None):
    """`_prepare` for a list of coarse fields, stacked: x (3n,lr,lr,1), the affine pairs (3n,2), u, v, p of each field in order."""
    model, back, per_case = _prepare_list(coarse_fields_list, lr_dim, hr_dim, stats_file, encoder_file, decoder_file,
                                          use_aspect_ratio_correction, lx, ly, use_adaptive_normalization, blend_factor, precision, _quiet,
                                          device)
    if not per_case:
        return model, np.empty((0, lr_dim, lr_dim, 1), np.float32), np.empty((0, 2), np.float32), np.empty((0, 2), np.float32), back
    x, ain, aout = (np.concatenate([pc[q] for pc in per_case]) for q in range(3))
    return model, x, ain, aout, back


def _quiet(*a, **k):
    pass


def _warn_nonfinite(bad):
    if bad:
        warnings.warn(f"super-resolved fields contained {bad} NaN/Inf values; replaced with zeros "
                      "(PyCFD_ML_accelerated.py:869-876)", RuntimeWarning)


def ml_super_resolution(coarse_fields: Dict[str, np.ndarray], lr_dim: int, hr_dim: int,
                        stats_file: str, encoder_file: str, decoder_file: str,
                        use_aspect_ratio_correction: bool = False, lx: float = 1.0, ly: float = 1.0,
                        use_adaptive_normalization: bool = False, blend_factor: float = 0.3,
                        precision: Optional[str] = None, verbose: bool = False) -> Dict[str, np.ndarray]:
    """Lid-driven-cavity defaults (PyCFD_ML_accelerated.py:764); `ml_super_resolution_bfs`
    has the backward-facing-step defaults.  Returns {'u','v','p'} -> (hr_dim, hr_dim) float32
    (float64 after the BFS back-resampling, as scipy returns it)."""
    say = print if verbose else _quiet
    model, x, ain, aout, back, fields = _prepare(coarse_fields, lr_dim, hr_dim, stats_file, encoder_file, decoder_file,
                                                 use_aspect_ratio_correction, lx, ly, use_adaptive_normalization, blend_factor, precision, say)
    if back is not None:
        y, bad = model.predict_resampled(x, back, in_affine=ain, out_affine=aout, nan_guard=True, return_nonfinite=True)
        y = y[..., None]
    else:
        y, bad = model.predict(x, in_affine=ain, out_affine=aout, nan_guard=True, return_nonfinite=True)
    _warn_nonfinite(bad)
    hr = {c: y[i, :, :, 0] for i, c in enumerate(COMPONENTS)}
    if verbose:  # the range scan costs more than the device work: only when it is printed
        for c in COMPONENTS:
            say(f"  {c.upper()}: {fields[c].shape} -> {hr[c].shape}, range [{hr[c].min():.6f}, {hr[c].max():.6f}]")
    return hr


def bc_arrays(bc):
    """(3,4) int types and (3,4) float values, [left,right,top,bottom] for u, v, p, from the solvers'
    `BoundaryConditions` object (`_get_bc_arrays`, PyCFD_ML_accelerated.py:~350 / bfs_ml_accelerated.py:497-521) or from a
    plain {'u': {'left': ('dirichlet', 0.0), ...}, ...} dict."""
    types = np.zeros((3, 4), np.int32)
    values = np.zeros((3, 4), np.float64)
    for k, c in enumerate(COMPONENTS):
        d = getattr(bc, f"{c}_boundaries", None)
        if d is None:
            d = bc[c]
        for s, side in enumerate(("left", "right", "top", "bottom")):
            e = d[side]
            t, v = (e.type, e.value) if hasattr(e, "type") else e
            types[k, s] = 0 if t == "dirichlet" else 1
            values[k, s] = v
    return types, values


def bfs_inlet_profiles(ny: int, dy: float, step_height: float, h: float, Ub: float) -> Dict[int, np.ndarray]:
    """Row-wise Dirichlet values of the BFS left boundary (bfs_ml_accelerated.py:524-562): wall (0) below the step,
    parabolic U = 6 Ub (y'/h)(1 - y'/h) above it with y' clamped to [0,h]; V = 0 everywhere."""
    y = (np.arange(1, ny + 1) - 0.5) * dy
    yp = np.clip(y - step_height, 0.0, h)
    u = np.where(y < step_height, 0.0, 6.0 * Ub * (yp / h) * (1.0 - (yp / h)))
    return {0: u, 1: np.zeros(ny)}


def ml_super_resolution_into_solver(coarse_fields, lr_dim: int, hr_dim: int, stats_file: str, encoder_file: str, decoder_file: str, bc,
                                    Var: Optional[np.ndarray] = None, left_profiles=None,
                                    use_aspect_ratio_correction: bool = False, lx: float = 1.0, ly: float = 1.0,
                                    use_adaptive_normalization: bool = False, blend_factor: float = 0.3,
                                    precision: Optional[str] = None) -> np.ndarray:
    """`ml_super_resolution` + the hand-off that follows it in the solvers (PyCFD_ML_accelerated.py:936-943,
    bfs_ml_accelerated.py:1211-1218) as one device pass: returns/fills the float64 `Var (3, nx+2, ny+2)` with the SR
    fields transposed into the interior and the ghost cells set from `bc`."""
    model, x, ain, aout, back, _ = _prepare(coarse_fields, lr_dim, hr_dim, stats_file, encoder_file, decoder_file,
                                            use_aspect_ratio_correction, lx, ly, use_adaptive_normalization, blend_factor, precision,
                                            _quiet)
    types, values = bc if isinstance(bc, tuple) else bc_arrays(bc)
    Var, bad = model.predict_into_solver_state(x, types, values, left_profiles=left_profiles, resampler=back, in_affine=ain, out_affine=aout,
                                               nan_guard=True, Var=Var, return_nonfinite=True)
    _warn_nonfinite(bad)
    return Var


def ml_super_resolution_batch(coarse_batch, lr_dim: int, hr_dim: int, stats_file: str, encoder_file: str, decoder_file: str,
                              use_aspect_ratio_correction: bool = False, lx: float = 1.0, ly: float = 1.0,
                              use_adaptive_normalization: bool = False, blend_factor: float = 0.3,
                              precision: Optional[str] = None, return_device: bool = False):
    """`ml_super_resolution` for a LIST of coarse fields in one device pass (the batched form of the BFS / LDC call; the
    reference makes one call per field).  Everything between the float64 coarse fields and the result runs on the GPU:
    the 10x10 aspect-ratio resampling and the adaptive blend of the statistics (`srcfd_prepare_inputs_device`,
    bfs_ml_accelerated.py:59-101, 1086-1097), the network with its fused standardise / de-standardise / NaN guard, and the
    resampling back to the rectangle (bfs_ml_accelerated.py:104-145).  Returns a list of {'u','v','p'} dicts like the
    per-field call (float32 (hr,hr); float64 after the BFS back-resampling), or with return_device=True the
    (N, 3, hr, hr) CUDA tensor."""
    import ctypes as C
    import torch
    from . import _lib as L
    from . import resample as rs
    n_f = len(coarse_batch)
    stats_lr, stats_hr = load_stats(stats_file, lr_dim, hr_dim)
    for f in (encoder_file, decoder_file):
        if not os.path.exists(f):
            raise FileNotFoundError(f"model file '{f}' not found")
    model = kc._device_handle((os.fspath(encoder_file), os.fspath(decoder_file)), precision or kc._DEFAULT_PRECISION)
    dev = torch.device("cuda", model.device)
    with torch.cuda.device(dev):     # the preparation kernel is launched on this device's current stream
        return _super_resolution_batch_on_device(coarse_batch, n_f, model, dev, stats_lr, stats_hr, lr_dim, hr_dim, use_aspect_ratio_correction,
                                                 lx, ly, use_adaptive_normalization, blend_factor, return_device)


def _super_resolution_batch_on_device(coarse_batch, n_f, model, dev, stats_lr, stats_hr, lr_dim, hr_dim, use_aspect_ratio_correction, lx, ly,
                                      use_adaptive_normalization, blend_factor, return_device):
    import ctypes as C
    import torch
    from . import _lib as L
    from . import resample as rs
    st = torch.cuda.current_stream(dev)
    h, w = np.asarray(coarse_batch[0]["u"]).shape
    fields = np.stack([np.stack([np.asarray(cf[c], np.float64) for c in COMPONENTS]) for cf in coarse_batch]).reshape(3 * n_f, h, w)
    f_dev = torch.from_numpy(np.ascontiguousarray(fields)).to(dev)
    train = torch.from_numpy(np.tile(np.array([stats_lr[c] for c in COMPONENTS], np.float64), (n_f, 1))).to(dev)
    aout = torch.from_numpy(np.tile(np.array([stats_hr[c] for c in COMPONENTS], np.float32), (n_f, 1))).to(dev)
    resample = use_aspect_ratio_correction and lx != ly
    Ry = Rx = None
    if resample:
        ry, rx = rs.rect_to_square_matrices(w, h, float(lx), float(ly))
        Ry, Rx = torch.from_numpy(np.array(ry)).to(dev), torch.from_numpy(np.array(rx)).to(dev)
    side = lr_dim if resample else h
    x = torch.empty((3 * n_f, side, side, 1), dtype=torch.float32, device=dev)
    ain = torch.empty((3 * n_f, 2), dtype=torch.float32, device=dev)
    y = torch.empty((3 * n_f, hr_dim, hr_dim, 1), dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    # every tensor of both device calls is checked before the first of them is enqueued: an lr_dim / hr_dim that is not the model's
    # is refused here, not found by the forward after the preparation kernel ran (or, for hr_dim, by a store past the end of y)
    model._device_args(x, y, ain, aout, bad, names=(f"x ({side}, {side}, 1), from lr_dim = {lr_dim} and the fields' size,",
                                                    f"y ({hr_dim}, {hr_dim}, 1), from hr_dim = {hr_dim},"))
    f64 = torch.float64
    p = lambda t, what, shape: L.device_ptr(t, what, f64, shape, model.device, optional=True, exact=True)
    L.check(L.lib.srcfd_prepare_inputs_device(p(f_dev, "fields", (3 * n_f, h, w)), 3 * n_f, h, w, p(Ry, "Ry", (lr_dim, h)), p(Rx, "Rx", (lr_dim, w)),
                                              lr_dim, p(train, "train_stats", (3 * n_f, 2)), int(bool(use_adaptive_normalization)), float(blend_factor),
                                              L.device_ptr(x, "x", torch.float32, (3 * n_f, side, side), model.device),
                                              L.device_ptr(ain, "in_affine", torch.float32, (3 * n_f, 2), model.device, exact=True),
                                              C.c_void_p(st.cuda_stream)))
    model.predict_device(x, y, in_affine=ain, out_affine=aout, nan_guard=True, nonfinite=bad)
    if resample:
        back = rs.square_to_rect_resampler(hr_dim, hr_dim, hr_dim, float(lx), float(ly), model.device)
        out = back.apply_device(y.view(3 * n_f, hr_dim, hr_dim))
    else:
        out = y.view(3 * n_f, hr_dim, hr_dim)
    _warn_nonfinite(int(bad.item()))
    out = out.view(n_f, 3, out.shape[-2], out.shape[-1])
    if return_device:
        return out
    host = out.cpu().numpy()
    return [{c: host[i, k] for k, c in enumerate(COMPONENTS)} for i in range(n_f)]


def ml_super_resolution_bfs(coarse_fields, lr_dim, hr_dim, stats_file, encoder_file, decoder_file,
                            use_aspect_ratio_correction: bool = False, lx: float = 1.0, ly: float = 1.0,
                            use_adaptive_normalization: bool = True, blend_factor: float = 0.3, **kw):
    """bfs_ml_accelerated.py:979-985 defaults."""
    return ml_super_resolution(coarse_fields, lr_dim, hr_dim, stats_file, encoder_file, decoder_file,
                               use_aspect_ratio_correction, lx, ly, use_adaptive_normalization, blend_factor, **kw)


def inject_into_solver_state(hr_fields: Dict[str, np.ndarray], Var: np.ndarray) -> None:
    """The consumer side of the boundary (PyCFD_ML_accelerated.py:936-938): write the SR
    fields, transposed, into the interior of the solver's float64 `Var[k, 1:-1, 1:-1]`."""
    for k, c in enumerate(COMPONENTS):
        Var[k, 1:-1, 1:-1] = hr_fields[c].T


def _tile_counts(H: int, W: int, lr_dim: int, oy: int, ox: int):
    """(TY, TX) of an (H, W) field cut into lr x lr tiles that share oy rows / ox columns with their neighbours; ValueError for an
    overlap outside 0 <= 2*o <= lr and for a size that is not T*(lr - o) + o, naming the two nearest sizes that are."""
    counts = []
    for axis, size, o in (("height", H, oy), ("width", W, ox)):
        if o < 0 or 2 * o > lr_dim:
            raise ValueError(f"overlap {o} on the {axis}: an overlap is at least 0 and at most half a tile (2*overlap <= lr_dim = {lr_dim}), "
                             "so that a point lies in at most two tiles per axis")
        step = lr_dim - o
        t = max((size - o) // step, 1)
        if t * step + o != size:
            raise ValueError(f"field {axis} {size} is not T*(lr_dim - overlap) + overlap for lr_dim {lr_dim}, overlap {o}; "
                             f"the nearest sizes that fit are {t * step + o} and {(t + 1) * step + o}")
        counts.append(t)
    return counts[0], counts[1]


def _blend_axis(y, T, S, O, w):
    """Stitches T tiles along one axis with the ramp across the overlaps.  y (..., T, ..., S + O) with the tile index at axis 0
    and the blended axis last; returns (..., T*S + O) without the tile axis.  float32, every operation rounded: a + w*(b - a)."""
    out = np.empty(y.shape[1:-1] + (T * S + O,), np.float32)
    for t in range(T):
        lo = O if t else 0
        hi = S if t < T - 1 else S + O
        out[..., t * S + lo:t * S + hi] = y[t][..., lo:hi]          # one source: the tile's bits
        if t:
            a, b = y[t - 1][..., S:S + O], y[t][..., :O]
            out[..., t * S:t * S + O] = a + w * (b - a)
    return out


def _stitch_overlapped(y, ty, tx, C, oy, ox, lr_dim):
    """The overlapped stitch of the samples y (n, hh, hw[, 1]) in sample order s = (ty*TX + tx)*C + c: along x inside every tile
    row first, then along y (the order matters at the corners)."""
    hh, hw = int(y.shape[1]), int(y.shape[2])
    if hh % lr_dim or hw % lr_dim:
        raise ValueError(f"an overlap needs an output that is a whole multiple of the input; the model maps {lr_dim} x {lr_dim} -> {hh} x {hw}")
    sy, sx = hh // lr_dim, hw // lr_dim
    Sy, Oy, Sx, Ox = (lr_dim - oy) * sy, oy * sy, (lr_dim - ox) * sx, ox * sx
    wy = ((np.arange(Oy, dtype=np.float64) + 0.5) / max(Oy, 1)).astype(np.float32)
    wx = ((np.arange(Ox, dtype=np.float64) + 0.5) / max(Ox, 1)).astype(np.float32)
    t = np.asarray(y, np.float32).reshape(ty, tx, C, hh, hw)
    rows = _blend_axis(t.transpose(1, 0, 2, 3, 4), tx, Sx, Ox, wx)                    # (TY, C, hh, W)
    full = _blend_axis(rows.transpose(0, 1, 3, 2), ty, Sy, Oy, wy)                    # (C, W, H): y last
    return np.ascontiguousarray(full.transpose(2, 1, 0))


def tiled_super_resolution(field: np.ndarray, model, lr_dim: int = 10, in_affine=None, out_affine=None, distributed: bool = False,
                           overlap=0) -> np.ndarray:
    """BASELINE config 5: a (T*lr, T*lr, C) coarse field is cut into T x T
    lr x lr tiles, each component of each tile super-resolved independently with the same
    weights, and the 400x400 results stitched to (T*400, T*400, C).  The reference defines
    no tiling; overlap=0, the default, cuts disjoint tiles and copies them.

    overlap (an int or (oy, ox), coarse cells, 0 <= 2*o <= lr): neighbouring tiles share o cells, the field is
    (TY*(lr-oy) + oy, TX*(lr-ox) + ox, C) and the model's output must be a whole multiple s of its input.  Per axis, with the fine
    stride S = (lr-o)*s and the fine overlap O = o*s: output row R belongs to tile t1 = min(R // S, T-1) at row r1 = R - t1*S; if
    t1 >= 1 and r1 < O it is a + w*(b - a) of tile t1-1 at row r1 + S (a) and tile t1 at row r1 (b) with w = float32((r1 + 0.5) / O),
    three float32 operations each rounded; otherwise it is copied.  x is blended first inside each tile row, then y; a pixel outside
    every overlap zone has its tile's bits.  This function is the specification `tiled_super_resolution_device` is held to.

    distributed=True (inside an initialised `torch.distributed` group, one process per GPU): every rank
    super-resolves its contiguous block of the T*T*C tile samples (shard.shard_range) and the blocks are
    exchanged with one all_gather, so each rank returns the whole stitched field.  The tiles are independent:
    there is no other collective."""
    from .engine import overlap_pair
    H, W, C = field.shape
    oy, ox = overlap_pair(overlap)
    if (oy, ox) == (0, 0):
        ty, tx = H // lr_dim, W // lr_dim
        if ty * lr_dim != H or tx * lr_dim != W:
            raise ValueError("field size must be a multiple of the tile size")
        tiles = field.reshape(ty, lr_dim, tx, lr_dim, C).transpose(0, 2, 4, 1, 3).reshape(ty * tx * C, lr_dim, lr_dim, 1)
    else:
        ty, tx = _tile_counts(H, W, lr_dim, oy, ox)
        ly, lx = lr_dim - oy, lr_dim - ox
        tiles = np.stack([field[a * ly:a * ly + lr_dim, b * lx:b * lx + lr_dim, c] for a in range(ty) for b in range(tx) for c in range(C)])[..., None]
    tiles = np.ascontiguousarray(tiles, dtype=np.float32)
    n = tiles.shape[0]
    ai = np.tile(np.asarray(in_affine, np.float32), (ty * tx, 1)) if in_affine is not None else None
    ao = np.tile(np.asarray(out_affine, np.float32), (ty * tx, 1)) if out_affine is not None else None
    if not distributed:
        y = model.predict(tiles, in_affine=ai, out_affine=ao)
    else:
        import torch
        import torch.distributed as dist
        from .shard import shard_range
        rank, world = dist.get_rank(), dist.get_world_size()
        lo, hi = shard_range(n, rank, world)
        y_loc = model.predict(tiles[lo:hi], in_affine=None if ai is None else ai[lo:hi], out_affine=None if ao is None else ao[lo:hi])
        hr = y_loc.shape[1] if hi > lo else None
        # blocks differ by at most one sample: pad to the largest, gather, cut
        per = -(-n // world)
        shape = torch.tensor([0 if hr is None else hr], dtype=torch.int64)
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
        shape = shape.to(dev)
        dist.all_reduce(shape, op=dist.ReduceOp.MAX)
        hr = int(shape.item())
        buf = torch.zeros((per, hr, hr, 1), dtype=torch.float32, device=dev)
        if hi > lo:
            buf[:hi - lo] = torch.from_numpy(np.ascontiguousarray(y_loc)).to(dev)
        parts = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(parts, buf)
        y = np.concatenate([parts[r][:shard_range(n, r, world)[1] - shard_range(n, r, world)[0]].cpu().numpy() for r in range(world)])
    if (oy, ox) != (0, 0):
        return _stitch_overlapped(y, ty, tx, C, oy, ox, lr_dim)
    hr = y.shape[1]
    return y.reshape(ty, tx, C, hr, hr).transpose(0, 3, 1, 4, 2).reshape(ty * hr, tx * hr, C)


def tile_source_index(n: int, world: int) -> np.ndarray:
    """Sharded tiling: the row of the gathered (world * per, hh, hw) buffer that holds tile sample s, per = ceil(n / world).  Rank r
    predicts the samples shard_range(n, r, world) into rows r * per onward, so the map is the identity only when n divides evenly."""
    from .shard import shard_range
    per = -(-n // world)
    idx = np.empty(n, np.int32)
    for r in range(world):
        lo, hi = shard_range(n, r, world)
        idx[lo:hi] = r * per + np.arange(hi - lo, dtype=np.int32)
    return idx


def _tiler_for(model, ty, tx, C, max_chunk, overlap=(0, 0)):
    """One Tiler per (model, TY, TX, C, max_chunk[, overlap]), kept on the model object: it lives and dies with the handle it borrows.
    Without an overlap the key is the four figures alone."""
    from .engine import Tiler
    cache = model.__dict__.setdefault("_tilers", {})
    key = (ty, tx, C, max_chunk) if tuple(overlap) == (0, 0) else (ty, tx, C, max_chunk, tuple(overlap))
    if key not in cache:
        cache[key] = Tiler(model, ty, tx, C, max_chunk, overlap)
    return cache[key]


def tiled_super_resolution_device(field, model, lr_dim: int = 10, in_affine=None, out_affine=None, out=None, stream=None,
                                  max_chunk: Optional[int] = None, distributed: bool = False, overlap=0):
    """`tiled_super_resolution` with the cut, the network and the stitch on the model's device (csrc/tiles.hip): the same tiles in
    the same sample order, and a result with the same bits.

    field: a float32 CUDA tensor (T_y*lr, T_x*lr, C) -- the stitched (T_y*hr, T_x*hr, C) tensor is returned (`out` when given) and
    nothing is synchronised: the work is enqueued on `stream` (a torch stream; None: the current one) -- or a numpy array, which
    is uploaded; the result then comes back as a numpy array (page-locked, from the result pool of `predict`).
    in_affine / out_affine: per-component (C, 2) (mean, std) pairs, numpy or CUDA tensors.  max_chunk: at most that many samples per
    network call (rounded down to whole tiles); None: the model's own largest unchunked call.
    model: an `SRModel`.  An object that only has `.predict` is what the host function takes.
    overlap: as in `tiled_super_resolution` -- strided tiles and the blending stitch (tiles_blend), bit for bit the host function's
    result; every chunk predicts into its planes of an intermediate of all samples and one stitch follows the last.

    distributed=True (inside an initialised `torch.distributed` group, one process per GPU): every rank cuts all tiles, predicts
    its `shard.shard_range` block into its rows of one (world * per, hr, hr) device buffer, the blocks are exchanged with one
    all_gather_into_tensor of device tensors (backend "gloo": the collective's payload alone goes through the host), and every
    rank stitches the whole field once through `tile_source_index`."""
    import torch
    from .engine import SRModel, _result_pool
    if not isinstance(model, SRModel):
        raise TypeError(f"tiled_super_resolution_device runs on an SRModel's device; {type(model).__name__} is not one -- an object "
                        "with only .predict is what pipeline.tiled_super_resolution takes")
    dev = torch.device("cuda", model.device)
    from_numpy = not isinstance(field, torch.Tensor)
    st = stream if stream is not None else torch.cuda.current_stream(dev)

    def on_device(a, shape=None):
        if a is None:
            return None
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        a = a.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        return a if shape is None else a.reshape(shape)

    with torch.cuda.device(dev), torch.cuda.stream(st):
        f = on_device(field)
        if f.dim() != 3:
            raise ValueError("field must have shape (H, W, C)")
        H, W, C = (int(v) for v in f.shape)
        ih, iw, _ = model.input_shape
        if (ih, iw) != (lr_dim, lr_dim):
            raise ValueError(f"the model takes {ih} x {iw} tiles, lr_dim is {lr_dim}")
        from .engine import overlap_pair
        oy, ox = overlap_pair(overlap)
        if (oy, ox) == (0, 0):
            ty, tx = H // lr_dim, W // lr_dim
            if ty * lr_dim != H or tx * lr_dim != W:
                raise ValueError("field size must be a multiple of the tile size")
        else:
            ty, tx = _tile_counts(H, W, lr_dim, oy, ox)
            oh, ow, _ = model.output_shape
            if oh % lr_dim or ow % lr_dim:
                raise ValueError(f"an overlap needs an output that is a whole multiple of the input; the model maps {lr_dim} x {lr_dim} -> {oh} x {ow}")
        tiler = _tiler_for(model, ty, tx, C, max_chunk, (oy, ox))
        ain, aout = on_device(in_affine, (C, 2)), on_device(out_affine, (C, 2))
        res = out if out is not None else torch.empty(tiler.out_shape, dtype=torch.float32, device=dev)
        if not distributed:
            tiler.run(f, res, in_affine=ain, out_affine=aout, stream=st)
        else:
            import torch.distributed as dist
            from .shard import shard_range
            rank, world = dist.get_rank(), dist.get_world_size()
            n = tiler.n
            per = -(-n // world)
            lo, hi = shard_range(n, rank, world)
            x, ain_n, aout_n = tiler.cut(f, ain, aout, stream=st)
            y = torch.empty((world * per, tiler.hh, tiler.hw, 1), dtype=torch.float32, device=dev)
            mine = y[rank * per:(rank + 1) * per]
            if hi > lo:
                model.predict_device(x[lo:hi], mine[:hi - lo], in_affine=None if ain_n is None else ain_n[lo:hi],
                                     out_affine=None if aout_n is None else aout_n[lo:hi], stream=st)
            if world > 1:
                if dist.get_backend() == "nccl":
                    dist.all_gather_into_tensor(y, mine)
                else:   # the collective's payload through the host, nothing else
                    block = mine.cpu()
                    parts = [torch.empty_like(block) for _ in range(world)]
                    dist.all_gather(parts, block)
                    y.copy_(torch.cat(parts), non_blocking=False)
            if world not in tiler._index:
                tiler._index[world] = torch.from_numpy(tile_source_index(n, world)).to(dev)
            tiler.stitch(y, res, 0, n, src_index=tiler._index[world], stream=st)
        if not from_numpy:
            return res
        host = _result_pool.empty(tiler.out_shape)
        torch.from_numpy(host).copy_(res)     # synchronises with the stream
        return host
