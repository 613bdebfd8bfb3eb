"""Seeded weights: stand-ins for the absent decoder_400 file, and Keras' default initialisation for training.

The reference's trained decoder files are absent from its checkout
(.MISSING_LARGE_BLOBS:29-34), so benchmarks and the smoke test run
random-init weights of the same architecture (sr-ae-conv.ipynb:c277-287).
Variance-preserving uniform init (variance 2.4 / fan_eff) keeps activations
O(1) through the six swish layers, as trained weights do.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import family

DECODER_SHAPES = family.decoder_shapes(400)
ENCODER_SHAPES = family.encoder_shapes(10)


def synthetic_decoder_weights(seed: int = 1, bias_scale: float = 0.1) -> Dict[str, np.ndarray]:
    """decoder_400; any other member of the family: `family.synthetic_decoder_weights(hr_dim, seed)`."""
    return family.synthetic_decoder_weights(400, seed, bias_scale)


def keras_default_init(seed: int = 0):
    """Fresh encoder_10 / decoder_400 weights as `build_encoder_10` / `build_decoder_400` create them
    (sr-ae-conv.ipynb:c162-169, c277-287): glorot_uniform kernels, zero biases.  -> (enc_w, dec_w).
    Any other pair: `family.keras_default_init(lr_dim, hr_dim, seed)`."""
    return family.keras_default_init(10, 400, seed)
