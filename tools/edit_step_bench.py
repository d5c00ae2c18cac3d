#!/usr/bin/env python3
"""Per-step time of the editing step bodies next to the plain DDIM step body on the config-2 model (f8f4, B = 16, 6 x 64 x 64 latent, 26
context tokens): the same denoiser runtime and the SAME engine (weights, plans, tiles), one process, the three calls alternating, median of
three rounds.  Writes profiles/edit_sampling.txt (--out).

    python tools/edit_step_bench.py [--out FILE] [--steps 40] [--rounds 3] [--no-routes]

  ddim          DDIMSampler.sample: the plain body [evaluation, update, +1] -- the code path of the commit before editing existed
  edit_img2img  DDIMSampler.edit(t_start = S, init "z0"), no mask: the same plain body after one start blend per stage ("without the blend")
  edit_masked   the same with a keep mask: [blend, evaluation, update, +1] per step, one clean blend per stage at the end

Step time: host clock around a whole call that ends in a device synchronise, divided by its step bodies (two stages); all loops replay
captured graphs in 20-step units, Philox noise, eta = 1, nothing logged in between.  Kernel time: one HIP event pair around 200 back-to-back
launches of the blend on the engine's own buffers.  No threshold: the blend is memory-bound and tiny next to a denoiser forward; the numbers
are written down.  Unless --no-routes is given, the figures of tests/test_edit_gpu.py's composed-loop and reference comparisons are taken
from a run of those tests in a child process and appended.
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
    mask = torch.zeros(B, 1, shape[1], shape[2], device=dev)
    mask[..., : shape[2] // 2] = 1.0
    common = dict(conditioning=c, num_stage=2, eta=1.0, verbose=False, noise="philox", log_every_t=10 ** 9)
    smp = DDIMSampler(model)
    calls = {
        "ddim": lambda k: smp.sample(S=S, batch_size=B, shape=shape, seed=k, **common)[0],
        "edit_img2img": lambda k: smp.edit(S, z0, t_start=S, seed=k, **common)[0],
        "edit_masked": lambda k: smp.edit(S, z0, t_start=S, keep_mask=mask, seed=k, **common)[0],
    }
    lines = [f"config-2 model (UNET_F8F4, bf16x3), B = {B}, latent {shape}, 26 context tokens, S = k = {S} x 2 stages per call, eta 1, Philox, "
             f"{torch.cuda.get_device_name(0)}"]
    for name, fn in calls.items():      # warm-up: plans, graph captures
        z = fn(0)
        torch.cuda.synchronize()
        assert torch.isfinite(z).all(), name
    eng, = unet.runtime()._sampler_engines.values()        # one engine serves all three
    lines.append(f"one engine, step bodies captured: {sorted(str(k) for k in eng.graphs)}")
    ms = {k: [] for k in calls}
    for r in range(args.rounds):        # alternating: A B C A B C ...
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(r + 1)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / (2 * S))
    for name, v in ms.items():
        lines.append(f"{name:13s} ms per replayed step body, per round: {', '.join(f'{x:.3f}' for x in v)}   median {statistics.median(v):.3f}  "
                     f"spread {max(v) - min(v):.3f}")
    d = statistics.median(ms["ddim"])
    for name in ("edit_img2img", "edit_masked"):
        a = statistics.median(ms[name])
        lines.append(f"{name} / ddim per step body = {a / d:.4f}  (difference {a - d:+.3f} ms; run-to-run spread above)")
    # the blend alone, on the engine's buffers (stage 1: window [3, 6) of 6 channels)
    s, n = 1, 200
    st = torch.cuda.current_stream()
    HW, a0, e0 = eng.H * eng.W, sum(eng.embed[:s]), sum(eng.embed[:s + 1])
    L = _lib.lib(eng.planes)
    eng.step.zero_()
    blend = lambda **kw: _lib.make_op("FRIDO_OP_KEEP_BLEND", **eng._blend_op(s, (a0, e0), True, **kw)[1])[1]
    for label, desc, nbytes in (("masked Philox blend", blend(), B * HW * (3 * (e0 - a0) + 1) * 4),
                                ("clean blend (reimpose)", blend(clean=True), B * HW * (3 * (e0 - a0) + 1) * 4)):
        run = lambda: [_lib.check(L.frido_keep_blend(C.byref(desc), st.cuda_stream), "frido_keep_blend") for _ in range(n)]
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
        lines.append(f"keep_blend_kernel, {label}: {us:.2f} us per launch (median of 5 x {n} back-to-back launches; min {min(ts):.2f}, max {max(ts):.2f}); "
                     f"must move {nbytes / 1e6:.2f} MB -> {nbytes / us / 1e6:.2f} TB/s (the state stays in the last-level cache between launches: a "
                     "cache figure, not an HBM one)")
    if not args.no_routes:
        lines.append("comparisons on the small test model (tests/test_edit_gpu.py, max-relative latent distance):")
        out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", os.path.join(REPO, "tests", "test_edit_gpu.py"), "-k",
                              "composed_from_apply_model or references_own"], capture_output=True, text=True, cwd=REPO)
        lines += ["  " + ln.strip().lstrip(".") for ln in out.stdout.splitlines() if " vs " in ln]
        lines.append("  " + (out.stdout.strip().splitlines() or ["(no output)"])[-1])
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
