#!/usr/bin/env python3
"""Time of one evaluation of the diffusion objective (FridoDiffusion.forward, two stages) on the config-2 denoiser at B = 16, next to the
same quantity composed by hand from the public calls that existed before it, and the denoiser-only floor.  Writes profiles/loss_eval.txt
(--out).

    python tools/loss_step_bench.py [--out FILE] [--arms new,composed,floor] [--calls 20] [--rounds 5]

Arms (interleaved in ONE process, A B C A B C ...; host clock around `calls` back-to-back evaluations that end in a device synchronise):
  new       model(x, c, t=t, noise="philox"): q_sample, both denoiser programs and the loss of both stages as one replayed graph
  new-tape  the same with a device noise tensor (noise=): the graph that reads the tape, plus its upload
  composed  per stage: torch.randn_like, model.q_sample (torch), model.apply_model (two layout changes, eager programs, a fresh tensor),
            the torch reduction and the stage row -- only calls that the parent of this feature has, so this arm also runs there
  floor     two eager PyUNetModel.forward calls on a prepared x_noisy (no noise, no loss)
Parity: the new path against the composed path on the same t and the same noise tensor, per stage row entry.
"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from frido_amd import synth  # noqa: E402


def composed(model, x, c, t, noises=None):
    """forward() written with q_sample + apply_model + torch reductions: (total, per-stage rows [S][3] = simple, vlb, loss)."""
    total, rows = torch.zeros((), device=x.device), []
    lvlb = getattr(model, "lvlb_weights", None)
    for s in range(model.num_resulotion):
        noise = torch.randn_like(x) if noises is None else noises[s]
        c0, c1 = sum(model.embed_dim_list[:s]), sum(model.embed_dim_list[:s + 1])
        x_noisy = model.q_sample(x_start=x, t=t, ch_start=c0, ch_end=c1, noise=noise, mix_tau=0.1)
        eps = model.apply_model(x_noisy, t, c, stage=s)
        ls = (noise[:, c0:c1] - eps).abs().mean([1, 2, 3])
        simple = ls.mean()                                   # logvar = 0: loss = l_simple_weight * mean(ls) + elbo_weight * vlb
        vlb = (lvlb[t] * ls).mean() if lvlb is not None else simple * 0
        loss = 1.0 * simple + 0.0 * vlb
        rows.append(torch.stack([simple, vlb, loss]))
        total = total + loss * 0.5
    return total, torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--arms", default="new,new-tape,composed,floor")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda")
    model = bench.build_model("bf16x3", dev)
    model.model.conditioning_key = "crossattn"      # ('__is_unconditional__' resets the wrapper's key; the context tensor is fed directly)
    model.cond_stage_trainable = False              # (... so forward() must not look for a cond stage to encode it)
    unet = model.model.diffusion_model
    B, Cn, hw = args.batch, unet.in_channels, unet.image_size
    x = torch.from_numpy(synth.seeded_normal("bench:loss:x", (B, Cn, hw, hw))).to(dev)
    c = torch.from_numpy(synth.seeded_normal("bench:ctx", (B, 26, 640))).to(dev)
    gen = torch.Generator().manual_seed(3)
    ts = [torch.randint(0, model.num_timesteps, (B,), generator=gen) for _ in range(8)]
    ts_dev = [t.to(dev) for t in ts]
    noise = torch.randn(B, Cn, hw, hw, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    xn = [model.q_sample(x, ts_dev[0], ch_start=sum(model.embed_dim_list[:s]), ch_end=sum(model.embed_dim_list[:s + 1]), noise=noise)
          for s in range(2)]

    arms = {
        "new": lambda i: model(x, c, t=ts_dev[i % 8], noise="philox", seed=i)[0],
        "new-tape": lambda i: model(x, c, t=ts_dev[i % 8], noise=noise)[0],
        "composed": lambda i: composed(model, x, c, ts_dev[i % 8])[0],
        "floor": lambda i: [unet(xn[s], ts_dev[i % 8], context=c, stage=s) for s in range(2)][-1],
    }
    arms = {k: arms[k] for k in args.arms.split(",")}
    lines = [f"f8f4 denoiser (UNET_F8F4, bf16x3), B = {B}, latent ({Cn}, {hw}, {hw}), 26 context tokens, loss l1, noise_mix_ratio 0.1, two stages, "
             f"{torch.cuda.get_device_name(0)}",
             f"ms per evaluation: host clock around {args.calls} back-to-back calls ending in one device synchronise, {args.rounds} interleaved rounds"]
    for fn in arms.values():           # warm: plans, graphs, tuner state
        for i in range(3):
            out = fn(i)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    ms = {k: [] for k in arms}
    for r in range(args.rounds):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.calls):
                fn(i)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.calls)
    for name, v in ms.items():
        lines.append(f"{name:9s} ms per evaluation, per round: {', '.join(f'{q:.3f}' for q in v)}   median {statistics.median(v):.3f}  "
                     f"spread {max(v) - min(v):.3f}")
    med = {k: statistics.median(v) for k, v in ms.items()}
    if "new" in med and "composed" in med:
        lines.append(f"new - composed = {med['new'] - med['composed']:+.3f} ms ({100 * (med['new'] / med['composed'] - 1):+.2f} %)")
    if "new" in med and "floor" in med:
        lines.append(f"new - floor = {med['new'] - med['floor']:+.3f} ms ({100 * (med['new'] / med['floor'] - 1):+.2f} % over two eager denoiser forwards)")
    if "composed" in med and "floor" in med:
        lines.append(f"composed - floor = {med['composed'] - med['floor']:+.3f} ms ({100 * (med['composed'] / med['floor'] - 1):+.2f} %)")
    if "new-tape" in arms and "composed" in arms:      # parity on the same t and noise
        _, d = model(x, c, t=ts_dev[0], noise=noise)
        tot_c, rows = composed(model, x, c, ts_dev[0], noises=[noise, noise])
        for s in range(2):
            got = [d[f"val/loss_simple_stage{s}"] / 0.5, d[f"val/loss_vlb_stage{s}"] / 0.5]
            lines.append(f"parity stage {s}: loss_simple {float(got[0]):.7g} (composed {float(rows[s][0]):.7g}, rel {abs(float(got[0]) / float(rows[s][0]) - 1):.2e}); "
                         f"loss_vlb {float(got[1]):.7g} (composed {float(rows[s][1]):.7g}, rel {abs(float(got[1]) / float(rows[s][1]) - 1):.2e})")
        tot = model(x, c, t=ts_dev[0], noise=noise)[0]
        lines.append(f"parity total: {float(tot):.7g} (composed {float(tot_c):.7g}, rel {abs(float(tot) / float(tot_c) - 1):.2e})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
