#!/usr/bin/env python3
"""Per-step time of the DDIM inversion step body next to the plain DDIM step body on the config-2 model (f8f4, B = 16, 6 x 64 x 64 latent,
26 context tokens): the same denoiser runtime (weights, tiles), one process, the two calls alternating, median of three rounds.  Writes
profiles/invert_sampling.txt (--out).

    python tools/invert_step_bench.py [--out FILE] [--steps 40] [--rounds 3] [--no-routes]

  ddim    DDIMSampler.sample at eta 0: [evaluation, sampler step, +1] per step, a hand-off between the stages
  invert  DDIMSampler.invert(t_start = S): [evaluation, frido_invert_step, +1] per step, every stage from z0

Step time: host clock around a whole call that ends in a device synchronise, divided by its step bodies (two stages); both loops replay
captured graphs in 20-step units, nothing logged in between.  Kernel time: one HIP event pair around 200 back-to-back launches of the update
on the engine's own buffers.  Expectation: the two step times agree within the run-to-run spread -- the update is a rounding error beside a
denoiser forward; no threshold, the numbers are written down.  Unless --no-routes is given, the figures tests/test_invert_gpu.py prints
(kernel against float64, engine against its composed loop, the round trip) are taken from a run of those tests in a child process and
appended.
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from frido_amd import _lib, synth  # noqa: E402
from frido_amd.samplers import DDIMSampler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-routes", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda")
    model = bench.build_model("bf16x3", dev)
    unet = model.model.diffusion_model
    B, S = args.batch, args.steps
    shape = (unet.in_channels, unet.image_size, unet.image_size)
    c = torch.from_numpy(synth.seeded_normal("bench:ctx", (B, 26, 640))).to(dev)
    z0 = torch.from_numpy(synth.seeded_normal("bench:z0", (B,) + shape)).to(dev)
    smp = DDIMSampler(model)
    calls = {
        "ddim": lambda k: smp.sample(S=S, batch_size=B, shape=shape, conditioning=c, num_stage=2, eta=0.0, verbose=False, noise="philox", seed=k,
                                     log_every_t=10 ** 9)[0],
        "invert": lambda k: smp.invert(S, z0, c, t_start=S, num_stage=2, verbose=False, log_every_t=10 ** 9)[0],
    }
    lines = [f"config-2 model (UNET_F8F4, bf16x3), B = {B}, latent {shape}, 26 context tokens, S = k = {S} x 2 stages per call, no guidance, "
             f"{torch.cuda.get_device_name(0)}"]
    for name, fn in calls.items():      # warm-up: plans, graph captures
        z = fn(0)
        torch.cuda.synchronize()
        assert torch.isfinite(z).all(), name
    eng, = (e for e in unet.runtime()._sampler_engines.values() if e.kind == "invert")
    lines.append(f"inversion engine, step bodies captured: {sorted(str(k) for k in eng.graphs)}")
    ms = {k: [] for k in calls}
    for r in range(args.rounds):        # alternating: A B A B ...
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(r + 1)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / (2 * S))
    for name, v in ms.items():
        lines.append(f"{name:7s} ms per replayed step body, per round: {', '.join(f'{x:.3f}' for x in v)}   median {statistics.median(v):.3f}  "
                     f"spread {max(v) - min(v):.3f}")
    d, a = statistics.median(ms["ddim"]), statistics.median(ms["invert"])
    lines.append(f"invert / ddim per step body = {a / d:.4f}  (difference {a - d:+.3f} ms; run-to-run spread above)")
    # the update alone, on the engine's buffers (stage 1: window [3, 6) of 6 channels)
    s, n = 1, 200
    st = torch.cuda.current_stream()
    nch = eng.embed[s]
    L = _lib.lib(eng.planes)
    eng.step.zero_()
    kind, fields = eng._update_op(s)
    desc = _lib.make_op(kind, **fields)[1]
    nbytes = B * eng.H * eng.W * 3 * nch * 4       # reads x and eps, writes x, on the window
    run = lambda: [_lib.check(L.frido_invert_step(C.byref(desc), st.cuda_stream), "frido_invert_step") for _ in range(n)]
    run()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):
        ev0.record(st)
        run()
        ev1.record(st)
        ev1.synchronize()
        ts.append(ev0.elapsed_time(ev1) * 1e3 / n)
    us = statistics.median(ts)
    lines.append(f"ddim_invert_step_kernel: {us:.2f} us per launch (median of 5 x {n} back-to-back launches; min {min(ts):.2f}, max {max(ts):.2f}); "
                 f"must move {nbytes / 1e6:.2f} MB -> {nbytes / us / 1e6:.2f} TB/s (the state stays in the last-level cache between launches: a "
                 "cache figure, not an HBM one)")
    if not args.no_routes:
        lines.append("comparisons on the small test model (tests/test_invert_gpu.py):")
        out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", os.path.join(REPO, "tests", "test_invert_gpu.py"), "-k",
                              "composed_from_apply_model or round_trip or (kernel_matches and f16)"], capture_output=True, text=True, cwd=REPO)
        lines += ["  " + ln.strip().lstrip(".") for ln in out.stdout.splitlines() if " vs " in ln or "round trip" in ln or "error / bound" in ln]
        lines.append("  " + (out.stdout.strip().splitlines() or ["(no output)"])[-1])
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
