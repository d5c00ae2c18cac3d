"""Times frido_amd.models.LPIPS on the MI355X and writes the report profiles/lpips.txt is: milliseconds per batch of image pairs, the
split between the four kernels of csrc/lpips.hip and the five slice programs, the launch count, the same network in torch fp32 eager
beside it, and -- with --test-log -- the errors tests/test_lpips_gpu.py printed in the same run.  Weights are the deterministic
filler's (no trained VGG16 / vgg.pth ships here): times do not depend on them.

    python -m pytest tests/test_lpips_gpu.py -m gpu -s > lpips_tests.log
    python tools/lpips_bench.py [--batch 16] [--size 256] [--reps 30] [--test-log lpips_tests.log] > profiles/lpips.txt

Every time is the median of `reps` device-event intervals after 3 warm calls; needs the GPU (there is no CPU path to time)."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HEAD = """LPIPS (frido_amd/lpips.py LpipsPlan + csrc/lpips.hip) on one MI355X: what was run, what was seen, what was not run.

What was run
  1. python -m pytest tests/test_lpips_gpu.py -m gpu -s      (the errors it printed are listed at the end)
  2. python tools/lpips_bench.py --test-log <that log>       (batch {B} of {S} x {S} pairs: the tower runs at batch {B2}; output below)
Both in one process each, on a shared box, profiler off.  Times are medians of {reps} device-event intervals after 3 warm calls
(min / max beside them); weights are the deterministic filler's ("lpips" profile), inputs uniform in [-1, 1].  GEMM tiles: {tiles}.

What was NOT run
  - Other batch sizes and image sizes, the bf16-pair build and precision="bf16": not timed (the bf16-pair build's errors are below).
  - No rocprofv3 trace: the split below is event-timed launches on an otherwise idle stream, not per-kernel times inside the graph;
    the GB/s figures divide the bytes a launch must move by that time and claim no share of the HBM peak.
  - No trained weights exist here: nothing below says anything about the quality of the metric.
  - One run on one box: the spread between boxes and between runs was not measured.  There is no pass mark on these times.

Reading it: the thirteen 3 x 3 convolutions are MFMA GEMMs in the three-pass fp32-class arithmetic and carry the time; the four new
kernels move each byte once.  The torch fp32 eager line is the same network (F.conv2d / relu / max_pool2d, then the normalisation,
projection and means as torch expressions) on the same card in the same process, for scale: it runs other arithmetic (MIOpen fp32)
and is no parity reference.
"""


def timed(fn, reps, warm=3):
    """Median / min / max device milliseconds of fn() (events on the current stream)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def fmt(t, nbytes=None):
    s = f"{t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    return s + (f"  {nbytes / t[0] / 1e6:7.0f} GB/s over {nbytes / 1e6:.1f} MB" if nbytes else "")


def eager_lpips(sd, lin_names, x, y):
    """The same network in torch fp32 eager: lpips.py:41-54 on the module's own weights."""
    from frido_amd.lpips import VGG_SLICES

    def feats(h):
        h = (h - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
        outs = []
        for si, convs in enumerate(VGG_SLICES):
            if si > 0:
                h = F.max_pool2d(h, 2, 2)
            for idx, _ in convs:
                h = F.relu(F.conv2d(h, sd[f"net.slice{si + 1}.{idx}.weight"], sd[f"net.slice{si + 1}.{idx}.bias"], padding=1))
            outs.append(h)
        return outs
    val = None
    for k, (a, b) in enumerate(zip(feats(x), feats(y))):
        a = a / (torch.sqrt((a ** 2).sum(1, keepdim=True)) + 1e-10)
        b = b / (torch.sqrt((b ** 2).sum(1, keepdim=True)) + 1e-10)
        r = F.conv2d((a - b) ** 2, sd[lin_names[k]]).mean([2, 3], keepdim=True)
        val = r if val is None else val + r
    return val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--test-log", default=None, help="output of `pytest tests/test_lpips_gpu.py -m gpu -s`: its error lines are appended")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/lpips_bench.py: no HIP device; nothing was measured")
    from frido_amd import lpips, tune
    from frido_amd.engine import current_stream_ptr
    from frido_amd.models import LPIPS
    from frido_amd.synth import fill_module

    B, S = args.batch, args.size
    tiles = ("the pinned cache where it holds the shape" if tune.cache_is_pinned_for_this_library() else
             "tuned live at plan time (frido_amd/tune.py: the committed tile cache is keyed to the library build from before csrc/lpips.hip "
             "joined it, so no pinned tile applied; it holds no entry of these shapes either)")
    print(HEAD.format(B=B, S=S, B2=2 * B, reps=args.reps, tiles=tiles))
    print("---- tools/lpips_bench.py ----")
    print(f"# LPIPS on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; batch {B} pairs of {S} x {S}, precision bf16x3 (fp16-pair planes), "
          f"median of {args.reps} event-timed calls after 3 warm ones")
    x = torch.rand(B, 3, S, S, device="cuda") * 2 - 1
    y = (0.7 * x + 0.3 * (torch.rand(B, 3, S, S, device="cuda") * 2 - 1)).clamp(-1, 1)
    t0 = time.perf_counter()
    m = fill_module(LPIPS(), "lpips.", "lpips").cuda()
    out = m(x, y)
    torch.cuda.synchronize()
    plan = next(iter(m._plans.values()))[0]
    n_ops = sum(len(p.ops) for p in plan.progs)
    n_kern = len(plan.steps) - len(plan.progs)
    print(f"first call, with filling the weights, planning and the capture: {time.perf_counter() - t0:.1f} s; launches per call: {n_kern} kernels of "
          f"csrc/lpips.hip (1 scale, 4 pools, 5 layers, 1 finish) + {n_ops} program ops in 5 slice programs, replayed as one graph")
    sp = current_stream_ptr(x.device)
    print(f"forward(x, y), as a user calls it (two copies in, graph, copy out): {fmt(timed(lambda: m(x, y), args.reps))}")
    print(f"  graph replay alone:                                               {fmt(timed(lambda: plan.graph.launch(sp), args.reps))}")
    total_k, total_p = 0.0, 0.0
    pool_i = layer_i = prog_i = 0
    for name, what in plan.steps:
        if name == "prog":
            hw = plan.planes_hw[prog_i]
            t = timed(lambda: what.run(sp), args.reps)
            total_p += t[0]
            print(f"  slice {prog_i + 1} program ({len(what.ops)} ops, {hw[0]} x {hw[1]} planes), op by op (no graph): {fmt(t)}")
            prog_i += 1
            continue
        if name == "frido_lpips_scale":
            nbytes, label = 2 * (2 * B * S * S * 3 * 4), "frido_lpips_scale"
        elif name == "frido_maxpool2":
            nbytes, label = what.B * what.C * 4 * (what.H * what.W + (what.H // 2) * (what.W // 2)), f"frido_maxpool2 after slice {pool_i + 1} (C = {what.C})"
            pool_i += 1
        elif name == "frido_lpips_layer":
            nbytes, label = 2 * what.B * what.HW * what.C * 4, f"frido_lpips_layer {layer_i} (C = {what.C}, {what.nblk} workgroups per sample)"
            layer_i += 1
        else:
            nbytes, label = None, "frido_lpips_finish"
        t = timed(lambda: lpips.launch(name, what, sp), args.reps)
        total_k += t[0]
        print(f"  {label + ':':66s}{fmt(t, nbytes)}")
    print(f"  sum of the medians: the {n_kern} kernels {total_k:.3f} ms, the 5 slice programs {total_p:.3f} ms")
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = eager_lpips(sd, m.lin_names(), x, y)
        t = timed(lambda: eager_lpips(sd, m.lin_names(), x, y), args.reps)
    print(f"torch fp32 eager, the same network and weights (two towers at batch {B}):    {fmt(t)}")
    print(f"  largest relative difference between the two results (other arithmetic, no parity claim): "
          f"{float(((out - ref) / ref).abs().max()):.2e}")
    if args.test_log:
        print("\n---- errors printed by tests/test_lpips_gpu.py (one run of the file, same box) ----")
        for line in open(args.test_log):
            line = line.strip().lstrip(".")
            if line.startswith(("lpips", "reconstruction_metrics")) or " passed" in line or " failed" in line:
                print(line)
        print("scale: max abs error against float64 | bound = 2 x the float32 evaluation of the same formula on the host (and the host's bits).")
        print("layer: relative error of the per-layer values and of the total against float64; bound = 2 x the largest float32-vs-float64 difference of")
        print("the host evaluation over all cases of the file.  tower: feature maps relative to each layer's max |f|, bound = 8 x the float32 restatement's")
        print("own difference; per-layer values and total relative, bound = 8 x E32 (the restatement's largest relative float32-vs-float64 difference")
        print("over all cases, samples and layers); the bf16-pair build gets 10 x the default build's bounds.")


if __name__ == "__main__":
    main()
