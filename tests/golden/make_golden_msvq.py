#!/usr/bin/env python3
"""Generate the MSFPNVQModel fixtures (tests/golden/msvq_*.npz, shipped_msvq_cfgs.json) by IMPORTING THE REFERENCE on CPU.

Runs only where the reference checkout exists; the fixtures it writes are data (inputs + expected outputs) and are committed.
Weights are never stored: both sides regenerate them with frido_amd.synth.fill_tensor keyed by state_dict name.

    python tests/golden/make_golden_msvq.py [names...]

Reference entry points exercised:
  taming/models/msvqgan.py:16-96      MSFPNVQModel.__init__ (state_dict key set)
  taming/models/msvqgan.py:116-159    encode (quantised latent [fine .. coarse], emb_loss, codes), decode
  taming/models/msvqgan.py:166-186    forward (reconstruction, the two aux decodes)
  taming/models/msvqgan.py:266-309    log_images (key set, per-scale reconstructions)
The reference's loss module (LPIPS + discriminator) is never instantiated: lossconfig is torch.nn.Identity, like the other generators.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from frido_amd.synth import fill_tensor, seeded_normal  # noqa: E402
sys.path.remove(REPO)
import importlib.util  # noqa: E402

_spec = importlib.util.spec_from_file_location("_ref_harness", os.path.join(REPO, "oracle", "_ref_harness.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

sys.path.insert(0, HERE)
from golden_cfg import VQ_SMALL  # noqa: E402

MIN_GAP = 1e-3      # an input is kept only if every VQ decision's first / second nearest squared distances differ by more than this (relative)
B = 2


def fill_module(mod, prefix=""):
    with torch.no_grad():
        for name, p in mod.named_parameters():
            p.copy_(torch.from_numpy(fill_tensor(prefix + name, p.shape)))
    return mod


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def build(**over):
    m = H.import_ref("taming.models.msvqgan")
    net = m.MSFPNVQModel(**dict(VQ_SMALL, lossconfig={"target": "torch.nn.Identity"}, **over))
    return fill_module(net, "first_stage_model.").eval()      # the prefix of the VQModelInterface fixtures: the same weights


def encode_watched(net, x):
    """encode(x) plus, per scale (coarse first), the quantiser's input z and the relative gap between the nearest and the second nearest
    code of every pixel (float64 distances)."""
    seen, hooks = [], []
    for q in net.ms_quantize:
        hooks.append(q.register_forward_hook(lambda mod, i, o, seen=seen: seen.append((mod, i[0].detach()))))
    quant, emb_loss, info = net.encode(x)
    for h in hooks:
        h.remove()
    gaps, zs = [], []
    for mod, z in seen:
        zf = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).double()
        d = ((zf[:, None, :] - mod.embedding.weight.detach().double()[None]) ** 2).sum(-1)
        d2, _ = d.sort(dim=1)
        gaps.append(((d2[:, 1] - d2[:, 0]) / d2[:, 1]).numpy())
        zs.append(z)
    return quant, emb_loss, info, zs, gaps


def pick_input(net):
    """The first seeded image all of whose VQ decisions are MIN_GAP clear -- 'codes equal' is then a fair demand of an fp32-class path."""
    for k in range(64):
        tag = "msvq:img" if k == 0 else f"msvq:img:{k}"
        x = torch.from_numpy(np.tanh(seeded_normal(tag, (B, 3, 64, 64))))
        out = encode_watched(net, x)
        worst = min(float(g.min()) for g in out[4])
        print(f"  {tag}: smallest first/second distance gap {worst:.3g}")
        if worst > MIN_GAP:
            return tag, x, out
    raise SystemExit("no seeded input with clear VQ decisions")


def gen_small():
    net = build()
    tag, x, (quant, emb_loss, info, zs, gaps) = pick_input(net)
    n = len(VQ_SMALL["embed_dim"])
    out = {"img": x.numpy(), "img_tag": np.array(tag), "quant": quant.numpy(), "emb_loss": emb_loss.numpy(),
           "keys": np.array(sorted(net.state_dict().keys()))}
    # per scale (coarse first): codes, the decision margins, the quantiser's input and rms(z_q - z)
    e = VQ_SMALL["embed_dim"]
    for s in range(n):
        out[f"idx_{s}"] = info[2][s].numpy()
        out[f"margin_{s}"] = gaps[s]
        out[f"h_{s}"] = zs[s].numpy()
        c0 = sum(e[s + 1:])                                  # [fine .. coarse]: scale s sits after the finer ones
        up = quant.shape[-1] // zs[s].shape[-1]
        zq = quant[:, c0:c0 + e[s], ::up, ::up]
        out[f"rms_{s}"] = np.float64(((zq - zs[s]).double() ** 2).mean().sqrt())
    dec, diff, _ = net(x)
    assert torch.equal(diff, emb_loss)
    out["dec"] = dec.numpy()
    net.use_aux_loss = True
    dec2, (aux, aux2), _, _ = net(x)
    assert torch.equal(dec2, dec)
    out["dec_aux"], out["dec_aux2"] = aux.numpy(), aux2.numpy()
    batch = {"image": x.permute(0, 2, 3, 1).contiguous(), "file_name": ["a", "b"]}
    log = net.log_images(batch)
    out["log_keys_aux"] = np.array(sorted(log.keys()))
    net.use_aux_loss = False
    log = net.log_images(batch)
    out["log_keys"] = np.array(sorted(log.keys()))
    log_nf = net.log_images({"image": batch["image"]})
    out["log_keys_nofile"] = np.array(sorted(log_nf.keys()))
    for k, v in log.items():
        if k.startswith("reconstructions_"):
            out["log_" + k] = v.numpy()
    assert torch.equal(log["reconstructions"], dec)
    save("msvq_small", **out)


def gen_small_nl():
    """legacy=False (the loss terms in the other order, quantize.py:289-291), sane_index_shape=True (codes as [B, h, w]), beta 0.4; the image
    of msvq_small."""
    g = np.load(os.path.join(HERE, "msvq_small.npz"))
    net = build(legacy=False, sane_index_shape=True, quant_beta=0.4)
    x = torch.from_numpy(g["img"])
    quant, emb_loss, info = net.encode(x)
    assert np.array_equal(quant.numpy(), g["quant"])
    out = {"emb_loss": emb_loss.numpy(), "quant_beta": np.float64(0.4)}
    for s, idx in enumerate(info[2]):
        out[f"idx_{s}"] = idx.numpy()
    save("msvq_small_nl", **out)


def gen_shipped_cfgs():
    """The `model:` tree of every configs/msvqgan/*.yaml the reference ships, as JSON (data: the host test feeds each one to
    instantiate_from_config)."""
    import glob
    import json
    import yaml
    root = os.path.join(H.REF_ROOT, "configs")
    out = {os.path.relpath(f, root): yaml.safe_load(open(f))["model"] for f in sorted(glob.glob(os.path.join(root, "msvqgan", "*.yaml")))}
    with open(os.path.join(HERE, "shipped_msvq_cfgs.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("shipped_msvq_cfgs.json:", len(out), "configs")


GENS = {"msvq_small": gen_small, "msvq_small_nl": gen_small_nl, "shipped_msvq_cfgs": gen_shipped_cfgs}

if __name__ == "__main__":
    torch.set_grad_enabled(False)
    for name in (sys.argv[1:] or list(GENS)):
        print(f"[{name}]")
        GENS[name]()
