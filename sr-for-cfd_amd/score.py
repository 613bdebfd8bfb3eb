"""Scoring of predictions against targets on the device (include/srcfd.h, "scoring"; csrc/score.hip).

`score_fields` and `EvalSet.score` return, per sample, what the notebook's `evaluate_for_re` (sr-ae-conv.ipynb:c323-369)
reduces with numpy -- MAE, MSE, the largest error, the ranges of truth and prediction -- with numpy's float32 bits, without the
predicted fields leaving the device.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, Optional

import numpy as np

from . import _lib as L


def score_plan(elems: int) -> dict:
    """Test hook (srcfd_score_plan): the summation order for a field of `elems` elements, the tables the kernel reads."""
    buf = C.create_string_buffer(1 << 15)
    L.check(L.lib.srcfd_score_plan(int(elems), buf, len(buf)))
    return json.loads(buf.value.decode())


def _as_dict(metrics: np.ndarray) -> Dict[str, np.ndarray]:
    return {name: np.ascontiguousarray(metrics[:, k]) for k, name in enumerate(L.SCORE_NAMES)}


def _affine(a, n: int, what: str) -> Optional[np.ndarray]:
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != (n, 2):
        raise ValueError(f"{what} must have shape ({n}, 2): (mean, std) per sample")
    return a


def _ptr(a: Optional[np.ndarray]):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def score_fields(pred, truth, pred_affine=None, truth_affine=None, device: int = 0) -> Dict[str, np.ndarray]:
    """Per sample of pred / truth (n, ...) float32: {'mae', 'mse', 'max_abs', 'truth_min', 'truth_max', 'pred_min', 'pred_max',
    'nonfinite'} as float32 arrays of length n, each with the bits of the numpy expression on
    p = pred * std + mean, t = truth * std + mean (affines (n, 2) = (mean, std), or None: the values as they are):
    np.mean(np.abs(t - p)), np.mean((t - p)**2), np.max(np.abs(t - p)), np.min(t), np.max(t), np.min(p), np.max(p) and the number
    of non-finite t - p."""
    pred = np.ascontiguousarray(pred, dtype=np.float32)
    truth = np.ascontiguousarray(truth, dtype=np.float32)
    if pred.shape != truth.shape or pred.ndim < 1:
        raise ValueError(f"pred {pred.shape} and truth {truth.shape} must have one shape (n, ...)")
    n = pred.shape[0]
    elems = int(np.prod(pred.shape[1:], dtype=np.int64))
    pa, ta = _affine(pred_affine, n, "pred_affine"), _affine(truth_affine, n, "truth_affine")
    metrics = np.empty((n, L.SCORE_FIELDS), np.float32)
    if n == 0:
        return _as_dict(metrics)
    L.check(L.lib.srcfd_score_fields(int(device), _ptr(pred), _ptr(truth), n, elems, _ptr(pa), _ptr(ta), _ptr(metrics)))
    return _as_dict(metrics)


def nmae_percent(mae, truth_min, truth_max) -> np.ndarray:
    """`evaluate_for_re`'s range-normalised MAE (train_main.py): float(mae) / (float(max - min) + 1e-8) * 100 per sample, float64."""
    mae, lo, hi = (np.asarray(a, np.float32) for a in (mae, truth_min, truth_max))
    return np.array([float(m) / (float(np.float32(h) - np.float32(l)) + 1e-8) * 100 for m, l, h in zip(mae, lo, hi)], np.float64)


class EvalSet:
    """A held-out set resident on one device (srcfd_evalset): x_lr (n, h, w, c) inputs and x_hr (n, oh, ow, oc) targets, with
    optional (n, 2) (mean, std) pairs -- in_affine standardises the input inside the forward, pred_affine / truth_affine
    inverse-standardise prediction and truth inside the scorer (the notebook's order).  `score(model)` predicts the set with the
    model's current precision and returns the metrics of `score_fields` plus 'nmae_percent'; only n x 8 floats come back.
    `history` collects what `train.fit(validation=...)` appends."""

    def __init__(self, x_lr, x_hr, in_affine=None, pred_affine=None, truth_affine=None, device: int = 0):
        x = np.ascontiguousarray(x_lr, dtype=np.float32)
        y = np.ascontiguousarray(x_hr, dtype=np.float32)
        if x.ndim < 2 or y.ndim < 2 or x.shape[0] != y.shape[0]:
            raise ValueError(f"x_lr {x.shape} and x_hr {y.shape} must be (n, ...) arrays of one length")
        self._h = None
        self.n = int(x.shape[0])
        self.device = int(device)
        self.in_shape, self.out_shape = tuple(x.shape[1:]), tuple(y.shape[1:])
        self.history = []
        ia, pa, ta = (_affine(a, self.n, w) for a, w in ((in_affine, "in_affine"), (pred_affine, "pred_affine"), (truth_affine, "truth_affine")))
        h = C.c_void_p()
        L.check(L.lib.srcfd_evalset_create(self.device, _ptr(x), int(np.prod(self.in_shape, dtype=np.int64)), _ptr(y),
                                           int(np.prod(self.out_shape, dtype=np.int64)), self.n, _ptr(ia), _ptr(pa), _ptr(ta), C.byref(h)))
        self._h = h

    def score(self, model) -> Dict[str, np.ndarray]:
        if not self._h:
            raise ValueError("EvalSet is closed")
        if not getattr(model, "_h", None):
            raise ValueError("model is closed")
        metrics = np.empty((self.n, L.SCORE_FIELDS), np.float32)
        L.check(L.lib.srcfd_evalset_score(self._h, model._h, _ptr(metrics)))
        out = _as_dict(metrics)
        out["nmae_percent"] = nmae_percent(out["mae"], out["truth_min"], out["truth_max"])
        return out

    def close(self):
        if getattr(self, "_h", None):
            L.lib.srcfd_evalset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
