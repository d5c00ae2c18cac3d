#!/usr/bin/env python3
"""Per-step time of the ancestral (DDPM) loop next to DDIM eta = 1 on the config-2 model (f8f4, B = 16, 6 x 64 x 64 latent, 26 context
tokens), interleaved in ONE process, and the update kernels' own time and achieved bytes/s.  Writes profiles/ancestral_step.txt (--out).

    python tools/ancestral_step_bench.py [--out FILE] [--steps 40] [--rounds 3]

Step time: host clock around a whole sampling call that ends in a device synchronise, divided by its step bodies (two stages) (both loops replay
captured graphs in 20-step units; Philox noise, nothing logged).  Kernel time: one HIP event pair around 200 back-to-back launches of the
update on the engine's own buffers.  Bytes: what the update must move, from shapes -- x and eps read, x' and x0 written.
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
from frido_amd.engine import Prog  # noqa: E402
from frido_amd.samplers import DDIMSampler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda")
    model = bench.build_model("bf16x3", dev)
    unet = model.model.diffusion_model
    B, S = args.batch, args.steps
    shape = (unet.in_channels, unet.image_size, unet.image_size)
    c = torch.from_numpy(synth.seeded_normal("bench:ctx", (B, 26, 640))).to(dev)
    calls = {
        "ddim_eta1": lambda k: DDIMSampler(model).sample(S=S, batch_size=B, shape=shape, conditioning=c, num_stage=2, eta=1.0, verbose=False,
                                                        noise="philox", seed=k, log_every_t=10 ** 9)[0],
        "ancestral": lambda k: model.p_sample_loop(c, (B,) + shape, timesteps=S, verbose=False, noise="philox", seed=k, log_every_t=10 ** 9),
    }
    lines = [f"config-2 model (UNET_F8F4, bf16x3), B = {B}, latent {shape}, 26 context tokens, {S} steps x 2 stages per call, Philox noise, "
             f"{torch.cuda.get_device_name(0)}"]
    for name, fn in calls.items():      # warm-up: plans, graph captures
        z = fn(0)
        torch.cuda.synchronize()
        assert torch.isfinite(z).all(), name
    # step bodies per stage and call, from the engines: make_ddim_timesteps gives 1000 // S-spaced steps, S + 1 or more of them when S does
    # not divide the schedule
    nsteps = {("ancestral" if e.kind == "ddpm" else "ddim_eta1"): e.n_steps for e in unet.runtime()._sampler_engines.values()}
    lines.append(f"step bodies per stage: {nsteps}")
    ms = {k: [] for k in calls}
    for r in range(args.rounds):        # interleaved: A B A B ...
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(r + 1)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / (2 * nsteps[name]))
    for name, v in ms.items():
        lines.append(f"{name:10s} ms per replayed step, per round: {', '.join(f'{x:.3f}' for x in v)}   median {statistics.median(v):.3f}  "
                     f"spread {max(v) - min(v):.3f}")
    a, d = statistics.median(ms["ancestral"]), statistics.median(ms["ddim_eta1"])
    lines.append(f"ancestral / ddim_eta1 = {a / d:.4f}  (difference {a - d:+.3f} ms; run-to-run spread above)")
    # the update kernels alone, on the engines' buffers
    engines = unet.runtime()._sampler_engines
    for key, eng in engines.items():
        s = 1
        kw, label = eng._update_op(s)[1], "ancestral_step_kernel" if eng.kind == "ddpm" else "sampler_step_kernel (ddim, eta 1)"
        n = 200
        p = Prog(dev, 2)
        for _ in range(n):
            p.emit("FRIDO_OP_SAMPLER_STEP", **kw)
        eng.step.zero_()
        st = torch.cuda.current_stream()
        p.run(st.cuda_stream)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(5):
            e0.record(st)
            p.run(st.cuda_stream)
            e1.record(st)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / n)
        HW, C, nch = eng.H * eng.W, eng.C, eng.embed[s]
        nbytes = B * HW * (C + nch + 2 * C) * 4          # both kernels: x and eps read, x' and x0 written (all C channels)
        us = statistics.median(ts)
        lines.append(f"{label}: {us:.2f} us per launch (median of 5 x {n} back-to-back launches; min {min(ts):.2f}, max {max(ts):.2f}); must move "
                     f"{nbytes / 1e6:.2f} MB -> {nbytes / us / 1e6:.2f} TB/s achieved (state of {B * HW * C * 4 / 1e6:.2f} MB stays in the 256-MB "
                     f"last-level cache between launches: a cache figure, not an HBM one)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
