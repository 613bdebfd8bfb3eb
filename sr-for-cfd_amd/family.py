"""The model family of the training notebook: `build_encoder_{10,20,50,80,100,400}` and
`build_decoder_{10,20,50,80,100,400}` (sr-ae-conv.ipynb), as tables.

Every encoder is a stack of 3x3 SAME `Conv2D`s (swish), `Flatten`, `Dense(128, swish)` and the linear
`latent_vector`; every decoder is `Dense(h*w*c, swish)`, `Reshape((h, w, c))`, a stack of stride-2
`Conv2DTranspose`s (swish) and the linear 3x3 SAME `Conv2D` `output_image_{hr}`.  Layer names are Keras'
automatic ones when the encoder is built first and the decoder second, as the notebook's main block does:
`conv2d`, `conv2d_1`, ..., `dense`, `latent_vector`, then `dense_1`, `reshape`, `conv2d_transpose`,
`conv2d_transpose_1`, ..., `output_image_{hr}`.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

LATENT_DIM = 50
DIMS = (10, 20, 50, 80, 100, 400)

# lr_dim -> [(filters, stride)] of the 3x3 SAME convolutions
ENCODER_CONVS = {
    10: [(64, 2), (128, 1)],
    20: [(64, 2), (128, 2)],
    50: [(64, 2), (128, 2), (256, 2), (512, 2)],
    80: [(32, 2), (64, 2), (128, 2), (256, 2)],
    100: [(32, 2), (64, 2), (128, 2), (256, 2), (512, 2)],
    400: [(16, 2), (32, 2), (64, 2), (128, 2), (256, 2)],
}
# hr_dim -> (reshape target (h, w, c), [(filters, kernel, padding 'same')] of the stride-2 transposed convolutions)
DECODER_CONVTS = {
    10: ((5, 5, 128), [(64, 3, True)]),
    20: ((5, 5, 128), [(64, 3, True), (32, 3, True)]),
    50: ((3, 3, 512), [(256, 3, True), (128, 3, True), (64, 3, False), (32, 2, False)]),
    80: ((5, 5, 256), [(128, 3, True), (64, 3, True), (32, 3, True), (16, 3, True)]),
    100: ((3, 3, 512), [(256, 3, True), (128, 3, True), (64, 3, False), (32, 2, False), (16, 2, False)]),
    400: ((12, 12, 256), [(128, 3, False), (64, 2, False), (32, 2, False), (16, 2, False), (8, 2, False)]),
}
# what `Trainer` takes: build_dgrad refuses a strided Conv2D behind the first layer, which every encoder but encoder_10 has
TRAINABLE_ENCODERS = (10,)


def _check(table, dim, what):
    if dim not in table:
        raise ValueError(f"no {what}_{dim} in the family; defined: {sorted(table)}")


def _numbered(base: str, i: int) -> str:
    return base if i == 0 else f"{base}_{i}"


def convt_out(size: int, k: int, stride: int, same: bool) -> int:
    """Keras Conv2DTranspose output size of one axis."""
    return size * stride if same else (size - 1) * stride + k


def encoder_shapes(lr_dim: int = 10, latent_dim: int = LATENT_DIM) -> Dict[str, tuple]:
    """{layer name: kernel shape} of encoder_{lr_dim}, in layer order."""
    _check(ENCODER_CONVS, lr_dim, "encoder")
    shapes, side, cin = {}, lr_dim, 1
    for i, (f, s) in enumerate(ENCODER_CONVS[lr_dim]):
        shapes[_numbered("conv2d", i)] = (3, 3, cin, f)
        side, cin = -(-side // s), f
    shapes["dense"] = (side * side * cin, 128)
    shapes["latent_vector"] = (128, latent_dim)
    return shapes


def decoder_shapes(hr_dim: int = 400, latent_dim: int = LATENT_DIM) -> Dict[str, tuple]:
    """{layer name: kernel shape} of decoder_{hr_dim}, in layer order; Conv2DTranspose kernels are (kh, kw, Cout, Cin)."""
    _check(DECODER_CONVTS, hr_dim, "decoder")
    (h, w, c), convts = DECODER_CONVTS[hr_dim]
    shapes = {"dense_1": (latent_dim, h * w * c)}
    for i, (f, k, _) in enumerate(convts):
        shapes[_numbered("conv2d_transpose", i)] = (k, k, f, c)
        c = f
    shapes[f"output_image_{hr_dim}"] = (3, 3, c, 1)
    return shapes


def layer_names(lr_dim: Optional[int], hr_dim: Optional[int]) -> List[str]:
    """Keras' automatic layer names, encoder first, then decoder (Flatten / Reshape included)."""
    names: List[str] = []
    if lr_dim is not None:
        convs = [n for n in encoder_shapes(lr_dim) if n.startswith("conv2d")]
        names += convs + ["flatten", "dense", "latent_vector"]
    if hr_dim is not None:
        sh = list(decoder_shapes(hr_dim))
        names += [sh[0], "reshape"] + sh[1:]
    return names


def _shapes_of(w: Dict[str, np.ndarray]) -> Dict[str, tuple]:
    return {k[:-len("/kernel")]: tuple(v.shape) for k, v in w.items() if k.endswith("/kernel")}


def encoder_dim_of(enc_w: Dict[str, np.ndarray]) -> int:
    """Which encoder a weight dict belongs to: the one with as many convolutions, the same filter counts and the same
    `dense` input width.  encoder_10 and encoder_20 have the same shapes (they differ in one stride): the answer is then 10,
    pass `lr_dim=20` where the other one is meant."""
    got = _shapes_of(enc_w)
    convs = {n: s for n, s in got.items() if n.startswith("conv2d") and not n.startswith("conv2d_transpose")}
    for lr in DIMS:
        want = encoder_shapes(lr)
        if all(got.get(n) == s for n, s in want.items() if n != "latent_vector") and len(convs) == len(want) - 2:
            return lr
    raise ValueError("weights match no encoder of the family")


def decoder_dim_of(dec_w: Dict[str, np.ndarray]) -> int:
    """Which decoder a weight dict belongs to: the `output_image_{hr}` layer names it."""
    for k in dec_w:
        if k.startswith("output_image_") and k.endswith("/kernel"):
            hr = int(k[len("output_image_"):-len("/kernel")])
            _check(DECODER_CONVTS, hr, "decoder")
            return hr
    raise ValueError("weights hold no output_image_* layer")


def encoder_specs(enc_w: Dict[str, np.ndarray], lr_dim: Optional[int] = None) -> List[dict]:
    """Layer specs (`SRModel.from_layers`) of encoder_{lr_dim} from a `{'<layer>/kernel', '<layer>/bias'}` dict."""
    lr = encoder_dim_of(enc_w) if lr_dim is None else lr_dim
    _check(ENCODER_CONVS, lr, "encoder")
    specs = []
    for i, (_, s) in enumerate(ENCODER_CONVS[lr]):
        n = _numbered("conv2d", i)
        specs.append(dict(kind="conv2d", name=n, k=3, stride=s, same=True, act="swish", w=enc_w[f"{n}/kernel"], b=enc_w[f"{n}/bias"]))
    specs += [
        dict(kind="flatten", name="flatten"),
        dict(kind="dense", name="dense", act="swish", w=enc_w["dense/kernel"], b=enc_w["dense/bias"]),
        dict(kind="dense", name="latent_vector", act="linear", w=enc_w["latent_vector/kernel"], b=enc_w["latent_vector/bias"]),
    ]
    return specs


def decoder_specs(dec_w: Dict[str, np.ndarray], hr_dim: Optional[int] = None) -> List[dict]:
    """Layer specs of decoder_{hr_dim} from a weight dict."""
    hr = decoder_dim_of(dec_w) if hr_dim is None else hr_dim
    _check(DECODER_CONVTS, hr, "decoder")
    shape, convts = DECODER_CONVTS[hr]
    specs = [dict(kind="dense", name="dense_1", act="swish", w=dec_w["dense_1/kernel"], b=dec_w["dense_1/bias"]),
             dict(kind="reshape", name="reshape", shape=shape)]
    for i, (_, k, same) in enumerate(convts):
        n = _numbered("conv2d_transpose", i)
        specs.append(dict(kind="conv2d_transpose", name=n, k=k, stride=2, same=same, act="swish", w=dec_w[f"{n}/kernel"], b=dec_w[f"{n}/bias"]))
    n = f"output_image_{hr}"
    specs.append(dict(kind="conv2d", name=n, k=3, stride=1, same=True, act="linear", w=dec_w[f"{n}/kernel"], b=dec_w[f"{n}/bias"]))
    return specs


def layers_from_weights(enc_w: Optional[Dict[str, np.ndarray]], dec_w: Optional[Dict[str, np.ndarray]],
                        lr_dim: Optional[int] = None, hr_dim: Optional[int] = None) -> List[dict]:
    specs: List[dict] = []
    if enc_w is not None:
        specs += encoder_specs(enc_w, lr_dim)
    if dec_w is not None:
        specs += decoder_specs(dec_w, hr_dim)
    return specs


def input_shape(enc_w: Optional[Dict[str, np.ndarray]], dec_w: Optional[Dict[str, np.ndarray]], lr_dim: Optional[int] = None) -> Tuple[int, int, int]:
    """Input (h, w, c) of the graph `layers_from_weights` describes."""
    if enc_w is not None:
        lr = encoder_dim_of(enc_w) if lr_dim is None else lr_dim
        return (lr, lr, 1)
    return (1, 1, int(dec_w["dense_1/kernel"].shape[0]))


def _bias_len(name: str, shape: tuple) -> int:
    return shape[2] if name.startswith("conv2d_transpose") else shape[-1]


def glorot_uniform(rng, shape) -> np.ndarray:
    """Keras `glorot_uniform` + `compute_fans`: the last two axes are (fan_in, fan_out) units, also for the
    (kh,kw,Cout,Cin) kernels of Conv2DTranspose; limit = sqrt(6 / (fan_in + fan_out))."""
    rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    limit = math.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
    return rng.uniform(-limit, limit, size=shape).astype(np.float32)


def keras_default_init(lr_dim: int = 10, hr_dim: int = 400, seed: int = 0):
    """Fresh encoder_{lr_dim} / decoder_{hr_dim} weights as the notebook's builders create them: glorot_uniform kernels,
    zero biases.  One generator, encoder first.  -> (enc_w, dec_w)."""
    rng = np.random.default_rng(seed)
    out = []
    for shapes in (encoder_shapes(lr_dim), decoder_shapes(hr_dim)):
        w = {}
        for name, shape in shapes.items():
            w[f"{name}/kernel"] = glorot_uniform(rng, shape)
            w[f"{name}/bias"] = np.zeros(_bias_len(name, shape), np.float32)
        out.append(w)
    return out[0], out[1]


def synthetic_decoder_weights(hr_dim: int = 400, seed: int = 1, bias_scale: float = 0.1) -> Dict[str, np.ndarray]:
    """Seeded stand-in for a trained decoder_{hr_dim}: variance-preserving uniform kernels (variance 2.4 / fan_eff, where
    fan_eff counts the taps of a stride-2 transposed convolution that reach one output pixel: k*k / 4) keep the activations
    O(1) through the swish layers, as trained weights do; small normal biases."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in decoder_shapes(hr_dim).items():
        tr = name.startswith("conv2d_transpose")
        if len(shape) == 2:
            fan_in = shape[0]
        else:
            rf = shape[0] * shape[1]
            fan_in = rf * (shape[3] if tr else shape[2])
        fan_eff = fan_in / 4.0 if (tr and shape[0] == 2) else (fan_in / 2.25 if tr else fan_in)
        limit = math.sqrt(3.0 * 2.4 / fan_eff)
        w[f"{name}/kernel"] = rng.uniform(-limit, limit, size=shape).astype(np.float32)
        w[f"{name}/bias"] = (bias_scale * rng.standard_normal(_bias_len(name, shape))).astype(np.float32)
    return w


def synthetic_encoder_weights(lr_dim: int = 10, seed: int = 2, bias_scale: float = 0.1) -> Dict[str, np.ndarray]:
    """Seeded stand-in for a trained encoder_{lr_dim} (no trained file exists for any encoder but encoder_10)."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in encoder_shapes(lr_dim).items():
        fan_in = int(np.prod(shape[:-1]))
        limit = math.sqrt(3.0 * 2.4 / fan_in)
        w[f"{name}/kernel"] = rng.uniform(-limit, limit, size=shape).astype(np.float32)
        w[f"{name}/bias"] = (bias_scale * rng.standard_normal(shape[-1])).astype(np.float32)
    return w


def output_dim(hr_dim: int) -> int:
    """Side of decoder_{hr_dim}'s output, computed from its layers (equals hr_dim for every member)."""
    _check(DECODER_CONVTS, hr_dim, "decoder")
    (h, _, _), convts = DECODER_CONVTS[hr_dim]
    for _, k, same in convts:
        h = convt_out(h, k, 2, same)
    return h
