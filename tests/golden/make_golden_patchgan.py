#!/usr/bin/env python3
"""Generate the PatchGAN / tokenizer-loss fixture (tests/golden/patchgan_ref.npz) by IMPORTING THE REFERENCE on CPU.

Runs only where the reference checkout exists; the fixture it writes is data (expected outputs) and is committed.  Weights and images
are never stored: both sides regenerate them -- the discriminator's state_dict with frido_amd.synth.fill_tensor(profile="patchgan"),
LPIPS's with profile="lpips", both keyed by state_dict name, the images from the seeds of tests/patchgan_ref.py.

    python tests/golden/make_golden_patchgan.py

Reference entry points exercised, in eval mode under no_grad:
  taming/modules/discriminator/model.py:17-67       NLayerDiscriminator (state_dict key set of both norm kinds, forward)
  taming/modules/util.py:10-69                      ActNorm (eval-mode forward)
  taming/modules/losses/vqperceptual.py:36-150      VQLPIPSWithDiscriminator (constructor, forward for both optimizer_idx)
Nothing is downloaded: torchvision.models.vgg16 is OUR stub (the 31-layer configuration-D nn.Sequential, uninitialised), `requests`,
`tqdm` (imported by taming/util.py) and `cv2` (vqperceptual.py) are empty stubs, and LPIPS.load_from_pretrained -- the download of
vgg.pth -- is made a no-op before the loss is instantiated.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import lpips_ref as L  # noqa: E402
import patchgan_ref as R  # noqa: E402
from frido_amd.synth import fill_tensor  # noqa: E402  (resolved now, before the reference's packages take over the path)
sys.path.remove(REPO)

_spec = importlib.util.spec_from_file_location("_ref_harness", os.path.join(REPO, "oracle", "_ref_harness.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

VGG16_D = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def _vgg16_stub(pretrained=False, **kw):
    """What lpips.py:79 reads of torchvision.models.vgg16: `.features`, configuration D."""
    layers, cin = [], 3
    for v in VGG16_D:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    net = nn.Module()
    net.features = nn.Sequential(*layers)
    return net


def reference_modules():
    """(taming.modules.discriminator.model, taming.modules.losses.vqperceptual) of the reference, stubs installed."""
    H.install()
    tv = sys.modules["torchvision"]
    tv.models = H._stub("torchvision.models", vgg16=_vgg16_stub)
    H._stub("requests")
    H._stub("cv2")
    H._stub("tqdm", tqdm=lambda it=None, **k: it)
    lp = H.import_ref("taming.modules.losses.lpips")
    lp.LPIPS.load_from_pretrained = lambda self, name="vgg_lpips": None
    return H.import_ref("taming.modules.discriminator.model"), H.import_ref("taming.modules.losses.vqperceptual")


def _fill(module, prefix, profile):
    """Every floating-point entry of the module's state_dict from the filler, keyed by prefix + name."""
    sd = module.state_dict()
    module.load_state_dict({k: (torch.from_numpy(fill_tensor(prefix + k, v.shape, profile).copy()) if v.is_floating_point() else v)
                            for k, v in sd.items()}, strict=True)
    return module


def main():
    dm, vq = reference_modules()
    arrs = {}
    for act in (False, True):
        sd = dm.NLayerDiscriminator(use_actnorm=act).state_dict()
        arrs[f"keys_actnorm_{int(act)}"] = np.array(list(sd))
        arrs[f"shapes_actnorm_{int(act)}"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
        arrs[f"dtypes_actnorm_{int(act)}"] = np.array([str(v.dtype) for v in sd.values()])
    for ci, (shape, ndf, nl, act) in enumerate(R.NET_CASES):
        net = _fill(dm.NLayerDiscriminator(input_nc=3, ndf=ndf, n_layers=nl, use_actnorm=act), R.PREFIX, "patchgan").eval()
        x, y = R.images(*shape, R.case_seed(ci))
        with torch.no_grad():
            lr, lf = net(x), net(y)
            hidden, h = [], x
            for m in net.main:
                h = m(h)
                if isinstance(m, nn.LeakyReLU):
                    hidden.append(h.clone())
        arrs[f"logits_real_{ci}"], arrs[f"logits_fake_{ci}"] = lr.numpy(), lf.numpy()
        for k, f in enumerate(hidden):
            arrs[f"hidden_{ci}_{k}"] = f.flatten()[R.sample_index(f.numel(), k, ci)].numpy()
        print(ci, shape, ndf, nl, act, "logits", tuple(lr.shape), "clip shares", R.clip_shares(lr, lf))
    x, y = R.images(*R.LOSS_SHAPE, R.LOSS_SEED)
    for li, (disc_loss, act) in enumerate(R.LOSS_CASES):
        loss = vq.VQLPIPSWithDiscriminator(disc_loss=disc_loss, use_actnorm=act, **R.LOSS_KW).eval()
        if li == 0:
            sd = loss.state_dict()
            arrs["loss_keys"] = np.array(list(sd))
            arrs["loss_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
        _fill(loss.discriminator, R.PREFIX, "patchgan")
        with torch.no_grad():
            for name, p in loss.perceptual_loss.named_parameters():
                p.copy_(torch.from_numpy(fill_tensor(L.PREFIX + name, p.shape, "lpips")))
        last_layer = nn.Parameter(torch.zeros(1))      # what msvqgan.py:230 passes is a weight; without a graph autograd.grad raises -> d_weight = 0
        for step in R.LOSS_STEPS:
            with torch.no_grad():
                l0, log0 = loss(torch.tensor(R.CODEBOOK_LOSS), x, y, 0, step, last_layer=last_layer, split="val")
                l1, log1 = loss(torch.tensor(R.CODEBOOK_LOSS), x, y, 1, step, last_layer=last_layer, split="val")
            assert list(log0) == ["val/" + k for k in R.LOG0_KEYS] and list(log1) == ["val/" + k for k in R.LOG1_KEYS], (list(log0), list(log1))
            tag = f"{li}_{step}"
            arrs[f"loss0_{tag}"], arrs[f"loss1_{tag}"] = np.float64(float(l0)), np.float64(float(l1))
            arrs[f"log0_{tag}"] = np.array([float(log0["val/" + k]) for k in R.LOG0_KEYS], dtype=np.float64)
            arrs[f"log1_{tag}"] = np.array([float(log1["val/" + k]) for k in R.LOG1_KEYS], dtype=np.float64)
            print(disc_loss, act, "step", step, "loss0", float(l0), "loss1", float(l1), {k: float(v) for k, v in log1.items()})
        with torch.no_grad():
            lr, lf = loss.discriminator(x), loss.discriminator(y)
        arrs[f"loss_logits_real_{li}"], arrs[f"loss_logits_fake_{li}"] = lr.numpy(), lf.numpy()
    arrs["net_shapes"] = np.array([c[0] for c in R.NET_CASES])
    path = os.path.join(HERE, "patchgan_ref.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
