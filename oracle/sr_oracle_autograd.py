"""Gradient oracle: the SR network in differentiable torch CPU ops (float64) + reference Adam.

TEST INFRASTRUCTURE ONLY (same import rule as sr_oracle.py).  Restates
sr-ae-conv.ipynb:c306-320 (`train_step`: loss = reduce_mean(mse), tape.gradient) and Keras'
Adam update rule; PARITY UNPINNED for the same reasons as the forward oracle.  `loss_and_grads_specs` does the same for
any layer graph `SRModel.from_layers` builds (the training tests' reference on every layer shape the trainer accepts).
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .sr_oracle import DECODER_LAYERS, ENCODER_LAYERS, same_padding


def flat_order(enc_w, dec_w) -> List[str]:
    """Keras trainable_weights order: per layer kernel then bias, encoder then decoder."""
    names = []
    for l in list(ENCODER_LAYERS if enc_w is not None else ()) + list(DECODER_LAYERS if dec_w is not None else ()):
        names += [f"{l}/kernel", f"{l}/bias"]
    return names


def loss_and_grads(x: np.ndarray, y: np.ndarray, enc_w: Dict[str, np.ndarray], dec_w: Dict[str, np.ndarray]) -> Tuple[float, np.ndarray]:
    w = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in {**enc_w, **dec_w}.items()}
    t = torch.tensor(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    _, pt, pb = same_padding(t.shape[2], 3, 2)
    _, pl, pr = same_padding(t.shape[3], 3, 2)
    h = F.silu(F.conv2d(F.pad(t, (pl, pr, pt, pb)), w["conv2d/kernel"].permute(3, 2, 0, 1).contiguous(), w["conv2d/bias"], stride=2))
    h = F.silu(F.conv2d(h, w["conv2d_1/kernel"].permute(3, 2, 0, 1).contiguous(), w["conv2d_1/bias"], padding=1))
    h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)
    h = F.silu(h @ w["dense/kernel"] + w["dense/bias"])
    z = h @ w["latent_vector/kernel"] + w["latent_vector/bias"]
    h = F.silu(z @ w["dense_1/kernel"] + w["dense_1/bias"]).reshape(-1, 12, 12, 256).permute(0, 3, 1, 2)
    for name in DECODER_LAYERS[1:6]:
        h = F.silu(F.conv_transpose2d(h, w[f"{name}/kernel"].permute(3, 2, 0, 1).contiguous(), w[f"{name}/bias"], stride=2))
    pred = F.conv2d(h, w["output_image_400/kernel"].permute(3, 2, 0, 1).contiguous(), w["output_image_400/bias"], padding=1).permute(0, 2, 3, 1)
    loss = torch.mean((torch.tensor(np.asarray(y, np.float64)) - pred) ** 2)
    loss.backward()
    flat = np.concatenate([w[k].grad.numpy().reshape(-1) for k in flat_order(enc_w, dec_w)])
    return float(loss.item()), flat


def _act_t(h, act):
    if act in ("swish", "silu"):
        return F.silu(h)
    if act in ("linear", None):
        return h
    if act == "relu":
        return torch.relu(h)
    if act == "sigmoid":
        return torch.sigmoid(h)
    if act == "tanh":
        return torch.tanh(h)
    raise ValueError(f"unsupported activation {act!r}")


def _forward_specs(specs, params, x, dtype, pre=None):
    """NHWC x -> NHWC prediction through the spec graph; params: {index: (kernel, bias)} torch leaves.  pre: a list that
    receives every weighted layer's pre-activation (gradient retained)."""
    def act(z, s):
        if pre is not None:
            z.retain_grad()
            pre.append(z)
        return _act_t(z, s.get("act", "linear"))

    h = torch.as_tensor(np.asarray(x), dtype=dtype).permute(0, 3, 1, 2)   # NCHW while spatial, (n, features) once flat
    for i, s in enumerate(specs):
        kind = s["kind"]
        if kind == "flatten":
            h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)                  # NHWC order
        elif kind == "reshape":
            oh, ow, oc = s["shape"]
            h = h.reshape(h.shape[0], oh, ow, oc).permute(0, 3, 1, 2)
        elif kind == "dense":
            w, b = params[i]
            h = act(h @ w + b, s)
        elif kind == "conv2d":
            w, b = params[i]
            st = int(s.get("stride", 1))
            kh, kw = w.shape[0], w.shape[1]
            if s.get("same", False):
                _, pt, pb = same_padding(h.shape[2], kh, st)
                _, pl, pr = same_padding(h.shape[3], kw, st)
                h = F.pad(h, (pl, pr, pt, pb))
            h = act(F.conv2d(h, w.permute(3, 2, 0, 1).contiguous(), b, stride=st), s)
        elif kind == "conv2d_transpose":
            if s.get("same", False):
                raise ValueError("the oracle restates VALID transposed convolutions only")
            w, b = params[i]                                                    # (kh, kw, Cout, Cin): no-flip scatter
            h = act(F.conv_transpose2d(h, w.permute(3, 2, 0, 1).contiguous(), b, stride=int(s.get("stride", 1))), s)
        else:
            raise ValueError(f"unsupported layer kind {kind!r}")
    return h.permute(0, 2, 3, 1) if h.dim() == 4 else h


def forward_specs(specs, x, dtype=torch.float64) -> np.ndarray:
    """The prediction of the spec graph (NHWC, or (n, features) when it ends flat), in `dtype` on the CPU."""
    params = {i: (torch.as_tensor(np.asarray(s["w"]), dtype=dtype), torch.as_tensor(np.asarray(s["b"]), dtype=dtype))
              for i, s in enumerate(specs) if "w" in s}
    with torch.no_grad():
        return _forward_specs(specs, params, x, dtype).numpy()


def loss_and_grads_specs(specs, in_shape, x: np.ndarray, y: np.ndarray, dtype=torch.float64, bias_cond: bool = False):
    """Loss and flat gradient of any layer graph `SRModel.from_layers` takes (the same spec dicts), in the trainer's parameter
    order: per layer with weights, kernel then bias.  Semantics as the forward oracle (sr_oracle.py): TF-SAME padding with the
    extra pixel at the bottom / right, Conv2DTranspose as a no-flip scatter of (kh, kw, Cout, Cin) kernels with output
    (H - 1) s + k, NHWC flatten / reshape; loss = mean over all output elements of (y - pred)^2.  dtype=torch.float32 runs the
    same graph in float32 on the CPU (the scale of the device tolerances).  Returns (loss, float64 gradient); bias_cond=True
    adds, per weighted layer, the condition number of its bias gradient as a sum over every output pixel of the pre-activation
    gradient dZ: || sum_px |dZ| ||_2 / || sum_px dZ ||_2 over the channels (how much any float32 evaluation of that sum
    amplifies the rounding of its terms)."""
    x = np.asarray(x)
    assert tuple(x.shape[1:]) == tuple(in_shape), (x.shape, in_shape)
    params = {i: (torch.tensor(np.asarray(s["w"]), dtype=dtype, requires_grad=True), torch.tensor(np.asarray(s["b"]), dtype=dtype, requires_grad=True))
              for i, s in enumerate(specs) if "w" in s}
    pre = [] if bias_cond else None
    pred = _forward_specs(specs, params, x, dtype, pre)
    yt = torch.as_tensor(np.asarray(y), dtype=dtype).reshape(pred.shape)
    loss = torch.mean((yt - pred) ** 2)
    loss.backward()
    flat = np.concatenate([t.grad.numpy().astype(np.float64).reshape(-1) for i in sorted(params) for t in params[i]])
    if not bias_cond:
        return float(loss.item()), flat
    conds = []
    for z in pre:
        g = z.grad.double().transpose(0, 1).reshape(z.shape[1], -1)      # channel-major: NCHW and (n, features) alike
        conds.append(float(torch.linalg.norm(g.abs().sum(1)) / max(float(torch.linalg.norm(g.sum(1))), 1e-300)))
    return float(loss.item()), flat, conds


def param_sizes_specs(specs) -> List[Tuple[str, int]]:
    """(name, size) of every flat-gradient tensor of a spec graph, in the trainer's order."""
    out = []
    for i, s in enumerate(specs):
        if "w" in s:
            nm = s.get("name") or f"layer{i}"
            out += [(f"{nm}/kernel", int(np.asarray(s["w"]).size)), (f"{nm}/bias", int(np.asarray(s["b"]).size))]
    return out


def adam_reference(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """Keras Adam, float64."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    alpha = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    return p - alpha * m / (np.sqrt(v) + eps), m, v
