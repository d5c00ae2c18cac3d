#!/usr/bin/env python3
"""Per-step time of the DPM-Solver++(2M) step body next to the DDIM eta = 0 step body on the config-2 model (f8f4, B = 16, 6 x 64 x 64 latent,
26 context tokens): the same denoiser runtime (weights, plans' pool, tiles), one process, the two samplers alternating, median of three
rounds.  Writes profiles/dpm_sampling.txt (--out).

    python tools/dpm_step_bench.py [--out FILE] [--steps 40] [--rounds 3] [--no-routes]

Step time: host clock around a whole sampling call that ends in a device synchronise, divided by its step bodies (two stages); both loops
replay captured graphs in 20-step units, Philox x_T, nothing logged in between.  Kernel time: one HIP event pair around 200 back-to-back
launches of each update on its engine's own buffers.  Bytes: what each update must move, from shapes.
Unless --no-routes is given, the two route figures of tests/test_dpm_gpu.py (engine vs the loop composed from apply_model, for the solver
and for DDIM eta = 0 on the small test model) are taken from a run of those tests in a child process and appended.
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
from frido_amd.engine import Prog  # noqa: E402
from frido_amd.samplers import DDIMSampler, DPMSolverSampler  # noqa: E402


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
    common = dict(S=S, batch_size=B, shape=shape, conditioning=c, num_stage=2, verbose=False, noise="philox", log_every_t=10 ** 9)
    calls = {
        "ddim_eta0": lambda k: DDIMSampler(model).sample(eta=0.0, seed=k, **common)[0],
        "dpm_2m": lambda k: DPMSolverSampler(model).sample(seed=k, **common)[0],
    }
    lines = [f"config-2 model (UNET_F8F4, bf16x3), B = {B}, latent {shape}, 26 context tokens, S = {S} x 2 stages per call, Philox x_T, "
             f"{torch.cuda.get_device_name(0)}"]
    for name, fn in calls.items():      # warm-up: plans, graph captures
        z = fn(0)
        torch.cuda.synchronize()
        assert torch.isfinite(z).all(), name
    engines = {("dpm_2m" if e.kind == "dpm" else "ddim_eta0"): e for e in unet.runtime()._sampler_engines.values()}
    nsteps = {k: e.n_steps for k, e in engines.items()}
    lines.append(f"step bodies per stage: {nsteps} (DPM: logSNR grid, duplicates removed)")
    ms = {k: [] for k in calls}
    for r in range(args.rounds):        # alternating: A B A B ...
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(r + 1)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / (2 * nsteps[name]))
    for name, v in ms.items():
        lines.append(f"{name:10s} ms per replayed step body, per round: {', '.join(f'{x:.3f}' for x in v)}   median {statistics.median(v):.3f}  "
                     f"spread {max(v) - min(v):.3f}")
    a, d = statistics.median(ms["dpm_2m"]), statistics.median(ms["ddim_eta0"])
    lines.append(f"dpm_2m / ddim_eta0 per step body = {a / d:.4f}  (difference {a - d:+.3f} ms; run-to-run spread above)")
    if a > 1.02 * d:
        lines.append("the DPM body is more than 2 % slower than the DDIM body: see the update kernels' own times below -- the update reads the "
                     "x0 history and writes it back on top of what the DDIM update moves")
    # the update kernels alone, on the engines' buffers
    s, n = 1, 200
    st = torch.cuda.current_stream()
    scratch = torch.empty_like(next(iter(engines.values())).x)      # x' goes here: the state the launches read stays what the last run left
    for name, eng in engines.items():
        HW, Cn, nch = eng.H * eng.W, eng.C, eng.embed[s]
        if name == "dpm_2m":
            kind, fields = eng._update_op(s)
            desc = _lib.make_op(kind, **fields)[1]
            desc.x_out = scratch.data_ptr()
            L = _lib.lib(eng.planes)
            run = lambda: [_lib.check(L.frido_dpm_step(C.byref(desc), st.cuda_stream), "frido_dpm_step") for _ in range(n)]
            # x (start + nch channels) and eps read, x', x0 and the history written, the history read on second-order rows
            nbytes, label = B * HW * ((s + 1) * nch + nch + 2 * (s + 1) * nch + 2 * nch) * 4, "dpm_step_kernel (second-order row)"
            eng.step.fill_(1)
        else:
            p = Prog(dev, 2)
            for _ in range(n):
                p.emit("FRIDO_OP_SAMPLER_STEP", **dict(eng._update_op(s)[1], x_out=scratch.data_ptr()))
            run = lambda p=p: p.run(st.cuda_stream)
            nbytes, label = B * HW * ((s + 1) * nch + nch + 2 * (s + 1) * nch) * 4, "sampler_step_kernel (ddim, eta 0)"
            eng.step.zero_()
        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(5):
            e0.record(st)
            run()
            e1.record(st)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / n)
        us = statistics.median(ts)
        lines.append(f"{label}: {us:.2f} us per launch (median of 5 x {n} back-to-back launches; min {min(ts):.2f}, max {max(ts):.2f}); must move "
                     f"{nbytes / 1e6:.2f} MB -> {nbytes / us / 1e6:.2f} TB/s achieved (the state stays in the last-level cache between launches: "
                     "a cache figure, not an HBM one)")
    if not args.no_routes:
        lines.append("route comparison on the small test model (tests/test_dpm_gpu.py, max-relative latent distance, engine vs the loop composed "
                     "from apply_model per step + the update restated in torch; bounds: 1e-3 and 4 x the DDIM figure):")
        out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", os.path.join(REPO, "tests", "test_dpm_gpu.py"), "-k",
                              "composed_from_apply_model or is_ddim_eta0"], capture_output=True, text=True, cwd=REPO)
        lines += ["  " + ln.strip().lstrip(".") for ln in out.stdout.splitlines() if "scale " in ln and "vs" in ln]
        lines.append("  " + (out.stdout.strip().splitlines() or ["(no output)"])[-1])
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
