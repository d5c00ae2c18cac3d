#!/usr/bin/env python3
"""Generate the LPIPS fixture (tests/golden/lpips_ref.npz) by IMPORTING THE REFERENCE on CPU.

Runs only where the reference checkout exists; the fixture it writes is data (expected outputs) and is committed.  Weights and images
are never stored: both sides regenerate them -- the weights with frido_amd.synth.fill_tensor(profile="lpips") keyed by state_dict name,
the images from the seeds of tests/lpips_ref.py.

    python tests/golden/make_golden_lpips.py

Reference entry points exercised:
  taming/modules/losses/lpips.py:11-25     LPIPS.__init__ (state_dict key set, both values of use_dropout)
  taming/modules/losses/lpips.py:41-54     LPIPS.forward
  taming/modules/losses/lpips.py:76-113    vgg16 (the five slices of torchvision's vgg16.features)
Nothing is downloaded: torchvision.models.vgg16 is OUR stub (an object whose `.features` is the standard 31-layer configuration-D
nn.Sequential, uninitialised), `requests`, `tqdm` (imported by taming/util.py) and `cv2` (vqperceptual.py) are empty stubs, and LPIPS.load_from_pretrained -- the
download of vgg.pth -- is made a no-op before the class is instantiated.
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
import lpips_ref as R  # noqa: E402  (imports frido_amd.synth lazily, inside its functions)
from frido_amd.synth import fill_tensor  # noqa: E402,F401  (resolved now, before the reference's packages take over the path)
sys.path.remove(REPO)

_spec = importlib.util.spec_from_file_location("_ref_harness", os.path.join(REPO, "oracle", "_ref_harness.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

VGG16_D = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def _vgg16_stub(pretrained=False, **kw):
    """What lpips.py:79 reads of torchvision.models.vgg16: `.features`, configuration D (conv3x3 + ReLU, 'M' = MaxPool2d(2, 2))."""
    layers, cin = [], 3
    for v in VGG16_D:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    net = nn.Module()
    net.features = nn.Sequential(*layers)
    assert len(net.features) == 31
    return net


def reference_lpips(use_dropout=True):
    H.install()
    tv = sys.modules["torchvision"]
    tv.models = H._stub("torchvision.models", vgg16=_vgg16_stub)
    H._stub("requests")
    H._stub("cv2")      # imported by taming/modules/losses/vqperceptual.py, which the package's __init__ pulls in; never called here
    H._stub("tqdm", tqdm=lambda it=None, **k: it)
    mod = H.import_ref("taming.modules.losses.lpips")
    mod.LPIPS.load_from_pretrained = lambda self, name="vgg_lpips": None
    return mod.LPIPS(use_dropout=use_dropout).eval()


def main():
    net = reference_lpips(True)
    arrs = {}
    for ud in (True, False):
        sd = reference_lpips(ud).state_dict()
        arrs[f"keys_dropout_{int(ud)}"] = np.array(list(sd))
        arrs[f"shapes_dropout_{int(ud)}"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.copy_(torch.from_numpy(fill_tensor(R.PREFIX + name, p.shape, "lpips")))
    for ci, case in enumerate(R.CASES):
        x, y = R.images(*case, R.case_seed(case))
        with torch.no_grad():
            fx, fy = net.net(net.scaling_layer(x)), net.net(net.scaling_layer(y))
            lins = [net.lin0, net.lin1, net.lin2, net.lin3, net.lin4]
            per = []
            for k in range(5):      # lpips.py:46-50 with the reference's own helpers, layer by layer
                m = sys.modules["taming.modules.losses.lpips"]
                d = (m.normalize_tensor(fx[k]) - m.normalize_tensor(fy[k])) ** 2
                per.append(m.spatial_average(lins[k].model(d), keepdim=True).flatten())
            out = net(x, y)
        assert out.shape == (case[0], 1, 1, 1)
        arrs[f"out_{ci}"] = out.flatten().numpy()
        arrs[f"per_layer_{ci}"] = torch.stack(per, dim=1).numpy()
        for k in range(5):
            idx = R.sample_index(fx[k].numel(), k, case)
            arrs[f"feat_x_{ci}_{k}"] = fx[k].flatten()[idx].numpy()
            arrs[f"feat_y_{ci}_{k}"] = fy[k].flatten()[idx].numpy()
        print(case, "out", out.flatten().tolist(), "per layer", torch.stack(per, dim=1)[0].tolist())
    arrs["cases"] = np.array(R.CASES)
    path = os.path.join(HERE, "lpips_ref.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
