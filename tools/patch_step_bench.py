#!/usr/bin/env python3
"""Per-step time of patch-wise DDIM sampling (split_input_params) next to the whole-latent engine doing identical denoiser work, interleaved
in ONE process, plus the two new kernels' own time and achieved bytes/s and both engines' peak memory.  Writes profiles/patch_sampling.txt
(--out).

    python tools/patch_step_bench.py [--out FILE] [--steps 20] [--rounds 3]

Patch mode: the f8f4 denoiser at B = 1 on a 6 x 128 x 128 latent, ks 64, stride 32 -> L = 9 crops of 64 x 64 per model evaluation.
Whole latent: the same library's engine at B = 9, 6 x 64 x 64 -- the same 9 denoiser forwards per step on the same GEMM shapes.
Step time: host clock around a whole sampling call that ends in a device synchronise, divided by its step bodies (two stages); both replay
captured graphs in 20-step units, Philox noise, nothing logged.  Kernel time: one HIP event pair around 200 back-to-back launches on the
engine's own buffers.  Bytes: what the kernel must move, from shapes.  Memory: torch's peak allocated bytes over one sampling call per
engine on a fresh denoiser runtime (packed weights, activation pool, plans, K / V^T caches), after a throw-away call of both arms, each
measured with the other engine dropped; the first arm is measured again at the end to show what the order does.
"""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from frido_amd import patching, synth  # noqa: E402
from frido_amd.samplers import DDIMSampler  # noqa: E402

SPLIT = dict(ks=(64, 64), stride=(32, 32), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_min_weight=0.01, clip_max_weight=0.5,
             clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)


def timed_launches(fn, n=200, reps=5):
    st = torch.cuda.current_stream()
    for _ in range(n):
        fn(st.cuda_stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(st)
        for _ in range(n):
            fn(st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / n)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda")
    model = bench.build_model("bf16x3", dev)
    unet = model.model.diffusion_model
    S, Cn = args.steps, unet.in_channels
    geo = patching.geometry(SPLIT, 128, 128, patching.MODEL, dev)
    L = geo.L
    c1 = torch.from_numpy(synth.seeded_normal("bench:ctx", (1, 26, 640))).to(dev)
    cL = c1.repeat(L, 1, 1).contiguous()

    def patch(k):
        model.split_input_params = dict(SPLIT)
        try:
            return DDIMSampler(model).sample(S=S, batch_size=1, shape=(Cn, 128, 128), conditioning=c1, num_stage=2, eta=1.0, verbose=False,
                                             noise="philox", seed=k, log_every_t=10 ** 9)[0]
        finally:
            del model.split_input_params

    def whole(k):
        return DDIMSampler(model).sample(S=S, batch_size=L, shape=(Cn, 64, 64), conditioning=cL, num_stage=2, eta=1.0, verbose=False,
                                         noise="philox", seed=k, log_every_t=10 ** 9)[0]
    calls = {"patch B=1 128x128 L=9": patch, "whole B=9 64x64": whole}
    lines = [f"f8f4 denoiser (UNET_F8F4, bf16x3), 26 context tokens, DDIM eta 1, {S} steps x 2 stages per call, Philox noise, "
             f"{torch.cuda.get_device_name(0)}",
             f"patch mode: latent (1, {Cn}, 128, 128), ks 64, stride 32 -> L = {L} crops; whole latent: ({L}, {Cn}, 64, 64)"]
    for fn in calls.values():           # throw-away first calls: process-wide one-time allocations (split-K workspaces, tuner state) happen here
        fn(0)
    torch.cuda.synchronize()
    peak = []
    for name in list(calls) + [next(iter(calls))]:      # each arm with only its own engine alive; the first arm again at the end (order check)
        unet.invalidate()
        gc.collect()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        z = calls[name](0)
        torch.cuda.synchronize()
        assert torch.isfinite(z).all(), name
        peak.append((name, torch.cuda.max_memory_allocated() - base, base))
    for name, v, base in peak:
        lines.append(f"{name:24s} peak device memory over one call on a fresh runtime (packed weights, plans, pool, caches), above the "
                     f"{base / 2 ** 20:.0f} MiB allocated before it: {v / 2 ** 20:.0f} MiB")
    for name, fn in calls.items():      # both engines alive for the interleaved timing
        fn(0)
    torch.cuda.synchronize()
    engines = list(unet.runtime()._sampler_engines.values())
    nsteps = engines[0].n_steps
    assert all(e.n_steps == nsteps for e in engines)
    ms = {k: [] for k in calls}
    for r in range(args.rounds):        # interleaved: A B A B ...
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(r + 1)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / (2 * nsteps))
    for name, v in ms.items():
        lines.append(f"{name:24s} ms per replayed step ({nsteps} per stage), per round: {', '.join(f'{x:.3f}' for x in v)}   "
                     f"median {statistics.median(v):.3f}  spread {max(v) - min(v):.3f}")
    p, w = (statistics.median(ms[k]) for k in calls)
    lines.append(f"patch - whole = {p - w:+.3f} ms per step ({100 * (p / w - 1):+.2f} %)")
    # the two kernels alone, on the patch engine's buffers (stage 1: 3 eps channels)
    eng = next(e for e in engines if e.geo is not None)
    s = 1
    nch = eng.embed[s]
    ops = eng._eval_ops(s)
    unf, fold = ops[0][1], ops[-1][1]
    tu = timed_launches(lambda st: patching.launch_unfold(unf, st))
    tf = timed_launches(lambda st: patching.launch_fold(fold, st))
    bu = 2 * L * 64 * 64 * Cn * 4                                          # every crop element read once and written once
    bf = (L * 64 * 64 * nch + 128 * 128 * nch) * 4 + 128 * 128 * 4 + geo.max_cover * 128 * 128 * 4      # crops read, eps written, norm, <= 4 weights per pixel
    for label, ts, nb in (("unfold_kernel (x -> 9 crops, 6 channels)", tu, bu), ("fold_kernel (9 crop eps -> eps, 3 channels)", tf, bf)):
        us = statistics.median(ts)
        lines.append(f"{label}: {us:.2f} us per launch (median of 5 x 200 back-to-back launches; min {min(ts):.2f}, max {max(ts):.2f}); must move "
                     f"{nb / 1e6:.2f} MB -> {nb / us / 1e6:.3f} TB/s achieved (the tensors stay in the last-level cache between launches: a cache "
                     "figure, not an HBM one; at this size a launch is mostly launch latency)")
    lines.append(f"expected gap per step = unfold + fold = {(statistics.median(tu) + statistics.median(tf)) / 1e3:.4f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
