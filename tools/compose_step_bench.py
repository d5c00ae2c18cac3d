#!/usr/bin/env python3
"""Per-step time of composed guidance next to classifier-free guidance on the config-2 model (f8f4, B = 16, 6 x 64 x 64 latent, 26 context
tokens): the same denoiser runtime (weights, tiles), one process, the calls alternating, median of three rounds.  Writes
profiles/compose_sampling.txt (--out).

    python tools/compose_step_bench.py [--out FILE] [--steps 40] [--rounds 3] [--no-trace] [--no-routes]

  cfg           DDIMSampler.sample(scale 1.5, uncond) at eta 0: [evaluation of 2 B, sampler step mixing the halves, +1] per step -- the old path
  n1            the same guidance through the composed route: [evaluation of 2 B, frido_guidance_compose, sampler step on slot 0, +1].  No
                public call takes this route (one conditioning without rescale IS the old path; a tiny guidance_rescale is other
                arithmetic), so the engine is built here with SamplerEngine(compose_always=True)
  n1_rescale    guidance_rescale = 0.7 alone (the rescaled kernel)
  n2 / n3       1 / 2 extra conditionings (compose=), evaluation of 3 B / 4 B; with _rescale: guidance_rescale = 0.7 on top

Step time: host clock around a whole call that ends in a device synchronise, divided by its step bodies (two stages); every loop replays
captured graphs in 20-step units, nothing logged in between.  Each composed step is set against the old-path step of the same run scaled
by xrep / 2 (the evaluation is linear in the batch at best): the difference is what the route costs beyond its larger batch, next to the
run-to-run spread.  Kernel times: HIP events around back-to-back launches on the engine's own buffers, and -- unless --no-trace -- a
kernel-trace run of their own (this script again under `rocprofv3 --kernel-trace`, --kernels-only).  Expectation to confirm or refute: the
extra launch costs microseconds next to a denoiser forward of milliseconds; no threshold, the numbers are written down.  Unless
--no-routes is given, the figures tests/test_compose_gpu.py prints are taken from a run of those tests in a child process and appended.
"""
import argparse
import csv
import ctypes as C
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from frido_amd import _lib, samplers, synth  # noqa: E402
from frido_amd.runtime import SamplerEngine  # noqa: E402
from frido_amd.samplers import DDIMSampler  # noqa: E402

SCALE, PHI, EXTRA_W = 1.5, 0.7, (-0.75, 0.5)
KERNELS = ("guidance_compose_kernel", "guidance_rescale_kernel")


def kernel_launches(B, HW, nch, n, launches, dev):
    """`launches` back-to-back launches of each form on buffers shaped like stage 1's of an engine with n conditionings.  Returns
    {kernel: us per launch} from one HIP event pair per form (median of 5)."""
    L = _lib.lib()
    st = torch.cuda.current_stream()
    eps = torch.from_numpy(synth.seeded_normal("bench:guide:eps", (n + 1, B * HW * nch))).to(dev)
    out = torch.empty(B * HW * nch, device=dev)
    w = torch.tensor([SCALE] + list(EXTRA_W[:n - 1]) + [PHI], dtype=torch.float32, device=dev)
    us = {}
    for rescale, name in enumerate(KERNELS):
        d = _lib.STRUCTS["FridoGuidanceCompose"](eps=eps.data_ptr(), out=out.data_ptr(), weights=w.data_ptr(), n=n, B=B, per_sample=HW * nch,
                                                 rescale=rescale)
        run = lambda: [_lib.check(L.frido_guidance_compose(C.byref(d), st.cuda_stream), "frido_guidance_compose") for _ in range(launches)]
        run()
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(5):
            ev0.record(st)
            run()
            ev1.record(st)
            ev1.synchronize()
            ts.append(ev0.elapsed_time(ev1) * 1e3 / launches)
        us[name] = (statistics.median(ts), min(ts), max(ts))
    return us


def traced_kernel_times(args):
    """The two kernels' own durations from a kernel-trace run of their own: {kernel: (median us, launches)}, or a string saying why not."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--kernels-only",
               "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return f"the traced run gave no kernel trace (exit {r.returncode})"
        dur = {k: [] for k in KERNELS}
        for path in files:
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    for k in KERNELS:
                        if k in row.get("Kernel_Name", ""):
                            dur[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        return {k: (statistics.median(v), len(v)) for k, v in dur.items() if v} or "the trace holds neither kernel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-routes", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="only launch the two kernels (the traced child run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda")
    B, S = args.batch, args.steps
    if args.kernels_only:       # stage 1 of the config-2 latent: 64 x 64 pixels, 3 channels
        for n in (1, 3):
            kernel_launches(B, 64 * 64, 3, n, 50, dev)
        torch.cuda.synchronize()
        return
    samplers.ENGINE_CACHE_SIZE = 16     # seven engines alternate here: none may be evicted and rebuilt inside a timed call
    model = bench.build_model("bf16x3", dev)
    unet = model.model.diffusion_model
    shape = (unet.in_channels, unet.image_size, unet.image_size)
    ctx = lambda tag: torch.from_numpy(synth.seeded_normal(f"bench:{tag}", (B, 26, 640))).to(dev)
    c, uc, extra = ctx("ctx"), ctx("uctx"), [ctx("ctx1"), ctx("ctx2")]
    smp = DDIMSampler(model)
    kw = dict(S=S, batch_size=B, shape=shape, conditioning=c, num_stage=2, eta=0.0, verbose=False, noise="philox", log_every_t=10 ** 9,
              unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)
    forced = SamplerEngine(unet.runtime().builder_for(0), unet.cfg, B=B, C=shape[0], H=shape[1], W=shape[2], nctx=26, S=S, eta=0.0, kind="ddim",
                           alphas_cumprod=model.alphas_cumprod.detach().float().cpu().numpy(), embed_dim=model.embed_dim_list, cfg_scale=SCALE,
                           num_stage=2, ncond=1, rescale=False, compose_always=True)
    comp = lambda n: [(extra[i], EXTRA_W[i]) for i in range(n - 1)]
    calls = {
        "cfg": (2, lambda k: smp.sample(seed=k, **kw)[0]),
        "n1": (2, lambda k: forced.run([c], uc, noise="philox", seed=k, log_every_t=10 ** 9, weights=[SCALE], phi=0.0)[0]),
        "n1_rescale": (2, lambda k: smp.sample(seed=k, guidance_rescale=PHI, **kw)[0]),
        "n2": (3, lambda k: smp.sample(seed=k, compose=comp(2), **kw)[0]),
        "n2_rescale": (3, lambda k: smp.sample(seed=k, compose=comp(2), guidance_rescale=PHI, **kw)[0]),
        "n3": (4, lambda k: smp.sample(seed=k, compose=comp(3), **kw)[0]),
        "n3_rescale": (4, lambda k: smp.sample(seed=k, compose=comp(3), guidance_rescale=PHI, **kw)[0]),
    }
    lines = [f"config-2 model (UNET_F8F4, bf16x3), B = {B}, latent {shape}, 26 context tokens, S = {S} x 2 stages per call, DDIM eta 0, scale "
             f"{SCALE}, extra weights {EXTRA_W}, phi {PHI}, {torch.cuda.get_device_name(0)}"]
    first = {}
    for name, (_, fn) in calls.items():      # warm-up: plans, graph captures
        first[name] = fn(0)
        torch.cuda.synchronize()
        assert torch.isfinite(first[name]).all(), name
    lines.append(f"n1 (composed route) vs cfg (old path), same seed: max |difference| / max = "
                 f"{float((first['n1'] - first['cfg']).abs().max() / first['cfg'].abs().max()):.3e}")
    ms = {k: [] for k in calls}
    for r in range(args.rounds):        # alternating: A B C ... A B C ...
        for name, (_, fn) in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(r + 1)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / (2 * S))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for name, v in ms.items():
        xrep = calls[name][0]
        line = (f"{name:11s} xrep {xrep}  ms per replayed step body, per round: {', '.join(f'{x:.3f}' for x in v)}   median {med[name]:.3f}  "
                f"spread {max(v) - min(v):.3f}")
        if name != "cfg":
            want = med["cfg"] * xrep / 2
            line += f"   cfg x {xrep}/2 = {want:.3f}: difference {med[name] - want:+.3f} ms ({100 * (med[name] / want - 1):+.2f} %)"
        lines.append(line)
    for n in (1, 3):
        for name, (us, lo, hi) in kernel_launches(B, shape[1] * shape[2], model.embed_dim_list[1], n, 200, dev).items():
            nbytes = B * shape[1] * shape[2] * model.embed_dim_list[1] * 4 * ((n + 2) + (2 if "rescale" in name else 0))
            lines.append(f"{name} n = {n}: {us:.2f} us per launch (HIP events, median of 5 x 200 back-to-back launches; min {lo:.2f}, max {hi:.2f}); "
                         f"moves {nbytes / 1e6:.2f} MB -> {nbytes / us / 1e6:.2f} TB/s (the slots stay in the last-level cache between launches: a "
                         "cache figure, not an HBM one)")
    if not args.no_trace:
        tr = traced_kernel_times(args)
        lines.append("kernel-trace run of their own (n = 1 and n = 3 launches together): " + (tr if isinstance(tr, str) else "; ".join(
            f"{k} median {v[0]:.2f} us over {v[1]} launches" for k, v in tr.items())))
    if not args.no_routes:
        lines.append("comparisons on the small test model (tests/test_compose_gpu.py):")
        out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", os.path.join(REPO, "tests", "test_compose_gpu.py"), "-k",
                              "rescaled_form or composed_from_apply_model or summed_scale or class_labels"],
                             capture_output=True, text=True, cwd=REPO)
        lines += ["  " + ln.strip().lstrip(".") for ln in out.stdout.splitlines() if " vs " in ln or "error / bound" in ln]
        lines.append("  " + (out.stdout.strip().splitlines() or ["(no output)"])[-1])
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
