"""Deterministic synthetic weights / inputs (no checkpoints or datasets are reachable offline).

Every parameter is filled from a pure-numpy generator keyed by the parameter's NAME and shape, so
the reference modules (in tests/golden/make_golden.py), the oracle and the HIP path all see
bit-identical weights without any weight file being committed.  Layers that the
reference zero-initialises (pyunet.py:236-238,801; attention.py:276-280) are filled like any other
layer, otherwise the U-Net output would be identically zero.
"""
import zlib

import numpy as np

__all__ = ["fill_tensor", "fill_state_dict", "seeded_normal"]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode("utf-8")))


# Residual-branch outputs: the last layer of every block that is ADDED to the stream (pyunet.py:236-238 out_layers conv, attention.py:276-280
# proj_out; taming model.py:99-137 conv2 / nin_shortcut, :160-166 attention proj_out).  The "heavy" profile scales them up so that the raw
# residual stream reaches 10^3 .. 10^4 -- the range a trained checkpoint can push the UN-NORMALISED operand producers into.
# (NOT the 1x1 skip / nin_shortcut convs: they act on the RAW stream, a gain there compounds from block to block -- 300^k)
_BRANCH_OUT = ("out_layers.3.weight", "proj_out.weight", "conv2.weight")
HEAVY_STREAM_GAIN = 6.0


def _fill_heavy(name, shape, rng, leaf):
    """Second deterministic filler (r05, r04 verdict item 5): what a TRAINED checkpoint looks like to the arithmetic, not what an
    initialiser produces -- heavy-tailed weights (Student-t, 3 degrees of freedom, unit variance) with a log-normal gain per output
    channel, GroupNorm / LayerNorm scales spread over [0.2, 3], biases of 0.5 sigma, and residual-branch outputs scaled by
    HEAVY_STREAM_GAIN so that the stream itself (every block input is normalised, so the gains do not compound: the stream is a
    random walk of ~sqrt(blocks) x gain) runs in the thousands."""
    if "embedding.weight" in name or name.endswith("emb.weight") or "stage_emb" in name:
        return (rng.standard_normal(shape) * (0.5 if "stage_emb" in name else 1.0)).astype(np.float32)
    if leaf in ("in_proj_weight", "text_projection") and len(shape) == 2:
        return (rng.standard_t(3, shape) / np.sqrt(3.0) / np.sqrt(shape[1] if leaf == "in_proj_weight" else shape[0])).astype(np.float32)
    if leaf == "weight" and len(shape) >= 2:
        fan_in = int(np.prod(shape[1:]))
        w = rng.standard_t(3, shape) / np.sqrt(3.0)
        gain = np.exp(0.5 * rng.standard_normal(shape[0])).reshape((-1,) + (1,) * (len(shape) - 1))
        w = w * gain / np.sqrt(fan_in)
        if name.endswith(_BRANCH_OUT):
            w = w * HEAVY_STREAM_GAIN
        return w.astype(np.float32)
    if leaf == "weight":  # norm scales
        return rng.uniform(0.2, 3.0, shape).astype(np.float32)
    if leaf == "bias":
        b = 0.5 * rng.standard_normal(shape)
        if name.endswith(tuple(n.replace(".weight", ".bias") for n in _BRANCH_OUT)):
            b = b * HEAVY_STREAM_GAIN
        return b.astype(np.float32)
    if leaf in ("g", "scale"):
        return rng.uniform(0.2, 3.0, shape).astype(np.float32)
    return (0.5 * rng.standard_normal(shape)).astype(np.float32)


def _fill_lpips(name, shape, rng, leaf):
    """Third filler: the LPIPS module (frido_amd.models.LPIPS / taming's own, same names).  Thirteen conv + ReLU layers in a row with no
    normalisation between them need He scale to keep the features O(1) down to relu5_3 -- std = sqrt(2 / fan_in), fan_in = 9 Cin --
    with small biases, 0.05 N(0, 1); the 1 x 1 projections linK.model.N.weight are non-negative like the trained ones, uniform in [0, 1)."""
    if any(part[:3] == "lin" and part[3:].isdigit() for part in name.split(".")):
        return rng.uniform(0.0, 1.0, shape).astype(np.float32)
    if leaf == "weight":
        return (rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:])))).astype(np.float32)
    return (0.05 * rng.standard_normal(shape)).astype(np.float32)


PATCHGAN_GAIN = 2.0      # on He scale: the logits of a filled discriminator then spread over several units, both hinges clip


def _fill_patchgan(name, shape, rng, leaf):
    """Fourth filler: the PatchGAN discriminator (frido_amd.models.NLayerDiscriminator / taming's own, same state_dict names; buffers
    too).  Conv weights PATCHGAN_GAIN x He scale so that a good share of the logits lies beyond +-1 (where relu(1 - l) and relu(1 + l)
    clip: a swapped sign then shows); per-channel DISTINCT norm statistics: running_var in [0.5, 2), running_mean 0.3 N(0, 1), BatchNorm
    weight in [0.5, 1.5), ActNorm scale in [0.5, 1.5) and loc 0.3 N(0, 1); biases 0.1 N(0, 1)."""
    if leaf == "weight" and len(shape) == 4:
        return (rng.standard_normal(shape) * PATCHGAN_GAIN * np.sqrt(2.0 / int(np.prod(shape[1:])))).astype(np.float32)
    if leaf in ("running_var", "weight", "scale"):
        return rng.uniform(0.5, 1.5 if leaf != "running_var" else 2.0, shape).astype(np.float32)
    if leaf in ("running_mean", "loc"):
        return (0.3 * rng.standard_normal(shape)).astype(np.float32)
    return (0.1 * rng.standard_normal(shape)).astype(np.float32)


INCEPTION_GAIN = 1.0     # on He scale; with the BatchNorm ranges below the 94 post-ReLU outputs stay O(1) from the stem to Mixed_7c


def _fill_inception(name, shape, rng, leaf):
    """Fifth filler: the Inception-v3 of the Fréchet distance (frido_amd.models.FIDInceptionV3, torchvision's names; buffers too).  94
    conv + BatchNorm + ReLU layers: conv weights INCEPTION_GAIN x He scale, sqrt(2 / fan_in), so that a layer hands on the second
    moment it received; per-channel DISTINCT BatchNorm statistics whose ratio gamma^2 / var averages about 1: running_var in
    [0.5, 1.5) (positive), weight in [0.75, 1.25), running_mean and bias 0.1 N(0, 1) -- about half of every output survives its ReLU
    and no output dies or saturates on the way down (tests/test_fid_host.py asserts it).  fc (run by FIDInceptionV3.logits only) gets fan-in scale."""
    if leaf == "weight" and len(shape) == 4:
        return (rng.standard_normal(shape) * INCEPTION_GAIN * np.sqrt(2.0 / int(np.prod(shape[1:])))).astype(np.float32)
    if leaf == "weight" and len(shape) == 2:
        return (rng.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
    if leaf == "running_var":
        return rng.uniform(0.5, 1.5, shape).astype(np.float32)
    if leaf == "weight":
        return rng.uniform(0.75, 1.25, shape).astype(np.float32)
    return (0.1 * rng.standard_normal(shape)).astype(np.float32)


_CACHE = None      # {(name, shape, profile): array} when enable_cache() was called (the GPU suite: tests/conftest.py)


def enable_cache():
    """Memoise fill_tensor for the life of the process.  The filler is a pure function of (name, shape, profile) and costs ~20 s per
    full-size model on one core; the GPU suite builds the same models dozens of times.  Callers only ever COPY the arrays."""
    global _CACHE
    if _CACHE is None:
        _CACHE = {}


def fill_tensor(name, shape, profile=None):
    """float32 array for parameter `name` (a state_dict key) of `shape`.  profile None: the fan-in-scaled N(0, sigma) filler every
    fixture of rounds 1-4 uses; "heavy": the trained-checkpoint-like dynamic range of _fill_heavy; "lpips": _fill_lpips, for the LPIPS module only;
    "patchgan": _fill_patchgan, for the discriminator only; "inception": _fill_inception, for FIDInceptionV3 only."""
    shape = tuple(int(s) for s in shape)
    if _CACHE is not None:
        key = (name, shape, profile)
        if key not in _CACHE:
            arr = _fill_tensor(name, shape, profile)
            _CACHE[key] = arr
        return _CACHE[key]
    return _fill_tensor(name, shape, profile)


def _fill_tensor(name, shape, profile):
    rng = _rng(name if profile is None else f"{profile}:{name}")
    leaf = name.rsplit(".", 1)[-1]
    if len(shape) == 0:
        return np.asarray(1.0, dtype=np.float32)
    if profile == "heavy":
        return _fill_heavy(name, shape, rng, leaf)
    if profile == "lpips":
        return _fill_lpips(name, shape, rng, leaf)
    if profile == "patchgan":
        return _fill_patchgan(name, shape, rng, leaf)
    if profile == "inception":
        return _fill_inception(name, shape, rng, leaf)
    if profile is not None:
        raise ValueError(f"unknown filler profile {profile!r}")
    if "embedding.weight" in name or name.endswith("emb.weight") or "stage_emb" in name:
        # VQ codebooks / token / stage embeddings: O(1) entries so that codes are well separated
        return (rng.standard_normal(shape) * (0.5 if "stage_emb" in name else 1.0)).astype(np.float32)
    if leaf in ("in_proj_weight", "text_projection") and len(shape) == 2:      # OpenAI CLIP's bare matrices: fan-in scaling too
        return (rng.standard_normal(shape) / np.sqrt(shape[1] if leaf == "in_proj_weight" else shape[0])).astype(np.float32)
    if leaf == "weight" and len(shape) >= 2:
        fan_in = int(np.prod(shape[1:]))
        return (rng.standard_normal(shape) / np.sqrt(fan_in)).astype(np.float32)
    if leaf == "weight":  # norm scales
        return (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
    if leaf == "bias":
        return (0.1 * rng.standard_normal(shape)).astype(np.float32)
    if leaf in ("g", "scale"):
        return (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
    return (0.1 * rng.standard_normal(shape)).astype(np.float32)


def fill_state_dict(shapes, skip=()):
    """shapes: mapping name -> shape.  Returns name -> float32 ndarray."""
    out = {}
    for name, shape in shapes.items():
        if any(name.startswith(s) or s in name for s in skip):
            continue
        out[name] = fill_tensor(name, shape)
    return out


def seeded_normal(tag, shape):
    """Standard-normal float32 input tensor keyed by a string tag (test/bench inputs)."""
    return _rng("input:" + tag).standard_normal(tuple(shape)).astype(np.float32)


def fill_module(module, prefix="", profile=None):
    """Fill every parameter of an nn.Module in place from the deterministic filler (keyed by prefix+name)."""
    import torch
    with torch.no_grad():
        for name, p in module.named_parameters():
            p.copy_(torch.from_numpy(fill_tensor(prefix + name, p.shape, profile)).to(p.device))
    if hasattr(module, "invalidate"):
        module.invalidate()
    return module
