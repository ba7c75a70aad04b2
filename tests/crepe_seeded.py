"""Seeded CREPE weights for the encoder fixtures (tools/make_encoder_goldens.py) and their tests.  The pretrained CREPE weights
belong to their authors and are not in this repository; the fixtures pin the architecture and arithmetic with these instead.

Rule: numpy.default_rng(seed) draws every state-dict entry in key order -- conv / classifier weights normal with std
gain / sqrt(fan_in), biases and BatchNorm shifts / running means normal with std 0.1, BatchNorm scales normal about 1 with
std 0.5 (some negative: the ReLU -> BN -> pool order matters), running variances uniform in [0.5, 2), the batch counters 0.
The classifier's gain and bias offset make the top-1 bin decisive on most frames (the tool asserts it)."""
import numpy as np
import torch

CLASSIFIER_GAIN = 2.0
CLASSIFIER_OFFSET = -2.0


def seeded_crepe_state(shapes, seed):
    """shapes: [(key, shape)] of a CREPE state dict in order -> {key: tensor} (float32; num_batches_tracked int64)."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape in shapes:
        shape = tuple(shape)
        name = key.rsplit(".", 1)[-1]
        if name == "num_batches_tracked":
            out[key] = torch.zeros(shape, dtype=torch.int64)
            continue
        if name == "weight" and len(shape) >= 2:
            gain = CLASSIFIER_GAIN if "classifier" in key else 1.6
            v = rng.standard_normal(shape) * gain / np.sqrt(np.prod(shape[1:]))
        elif name == "weight":                                   # BatchNorm scale
            v = 1.0 + 0.5 * rng.standard_normal(shape)
        elif name == "running_var":
            v = rng.uniform(0.5, 2.0, shape)
        else:                                                     # biases, BatchNorm shifts, running means
            v = 0.1 * rng.standard_normal(shape)
            if key.startswith("classifier") or ".classifier" in key:
                v = v + CLASSIFIER_OFFSET
        out[key] = torch.from_numpy(v.astype(np.float32))
    return out


def crepe_shapes(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


def top1_margin(probabilities):
    """top-1 minus top-2 probability per frame ([.., 360] numpy); NaN rows give NaN."""
    s = np.sort(probabilities, axis=-1)
    return s[..., -1] - s[..., -2]
