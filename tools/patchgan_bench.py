"""Times frido_amd.models.VQLPIPSWithDiscriminator.evaluate and its NLayerDiscriminator on the MI355X and writes the report
profiles/patchgan.txt is: milliseconds per evaluate call, the split of the discriminator's graph between the five kernels of
csrc/patchgan.hip and the middle convolutions' slice programs, the GB/s of the stem and the affines on the large planes, the same
discriminator in torch fp32 eager beside it, and -- with --test-log -- the errors tests/test_patchgan_gpu.py printed in the same run.
Weights are the deterministic filler's (no trained discriminator ships here): times do not depend on them, and the values mean
nothing about image quality.

    python -m pytest tests/test_patchgan_gpu.py -m gpu -s > patchgan_tests.log
    python tools/patchgan_bench.py [--batch 16] [--size 256] [--reps 30] [--test-log patchgan_tests.log] > profiles/patchgan.txt

Every time is the median of `reps` device-event intervals after 3 warm calls; needs the GPU (there is no CPU path to time)."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HEAD = """PatchGAN discriminator + the tokenizer's loss (frido_amd/patchgan.py PatchGanPlan + csrc/patchgan.hip) on one MI355X: what was run, what
was seen, what was not run.

What was run
  1. python -m pytest tests/test_patchgan_gpu.py -m gpu -s   (the errors it printed are listed at the end)
  2. python tools/patchgan_bench.py --test-log <that log>    (batch {B} of {S} x {S} pairs, the default net ndf 64 / 3 layers / BatchNorm:
                                                              the discriminator runs at batch {B2}; output below)
Both in one process each, on a shared box, profiler off.  Times are medians of {reps} device-event intervals after 3 warm calls
(min / max beside them); weights are the deterministic filler's, inputs uniform in [-1, 1].  GEMM tiles: {tiles}.

What was NOT run
  - Other batch sizes, image sizes and nets, the bf16-pair build and precision="bf16": not timed (the bf16-pair build's errors are below).
  - No rocprofv3 trace: the split below is event-timed launches on an otherwise idle stream, not per-kernel times inside the graph;
    the GB/s figures divide the bytes a launch must move (each input and output once) by that time and claim no share of the HBM peak.
  - No trained weights exist here: with filler weights the logits, g_loss and disc_loss say nothing about image quality.
  - One run on one box: the spread between boxes and between runs was not measured.  There is no pass mark on these times.

Reading it: the three middle 4 x 4 convolutions (K = 1024, 2048, 4096) are MFMA GEMMs in the three-pass fp32-class arithmetic and carry
most of the discriminator's time.  The affines run at the rate of the caches their planes still sit in.  The stem is the slowest of the new
launches and is NOT bound by memory: for its four output pixels a thread issues 48 LDS reads, 192 (cached) source loads and 768 FMAs
for four 16-byte stores (with one pixel per thread, 48 LDS reads each, it took 0.38 ms).  The head reads every input row 16 times through
the caches.
The torch fp32 eager line is the same discriminator (F.conv2d / F.batch_norm / F.leaky_relu on both images, then the hinge and the means
as torch expressions) on the same card in the same process, for scale: it runs other arithmetic (MIOpen fp32) and is no parity reference.
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


def eager_disc(sd, table, x):
    """The same discriminator in torch fp32 eager on the module's own weights (eval-mode BatchNorm2d)."""
    h = x
    for ci, ni, _, _, stride in table:
        h = F.conv2d(h, sd[f"main.{ci}.weight"], sd.get(f"main.{ci}.bias"), stride=stride, padding=1)
        if ni is not None:
            h = F.batch_norm(h, sd[f"main.{ni}.running_mean"], sd[f"main.{ni}.running_var"], sd[f"main.{ni}.weight"], sd[f"main.{ni}.bias"],
                             False, 0.0, 1e-5)
        if ci != table[-1][0]:
            h = F.leaky_relu(h, 0.2)
    return h


def eager_terms(sd, table, x, y):
    lr, lf = eager_disc(sd, table, x), eager_disc(sd, table, y)
    return torch.stack([lr.mean(), lf.mean(), -lf.mean(), 0.5 * (F.relu(1. - lr).mean() + F.relu(1. + lf).mean()),
                        0.5 * (F.softplus(-lr).mean() + F.softplus(lf).mean())])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--test-log", default=None, help="output of `pytest tests/test_patchgan_gpu.py -m gpu -s`: its error lines are appended")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/patchgan_bench.py: no HIP device; nothing was measured")
    import lpips_ref
    import patchgan_ref
    from frido_amd import patchgan as pg, tune
    from frido_amd.engine import current_stream_ptr
    from frido_amd.models import VQLPIPSWithDiscriminator

    B, S = args.batch, args.size
    tiles = ("the pinned cache where it holds the shape" if tune.cache_is_pinned_for_this_library() else
             "tuned live at plan time (frido_amd/tune.py: the committed tile cache is keyed to an earlier build of the library, so no "
             "pinned tile applied; it holds no entry of these shapes either)")
    print(HEAD.format(B=B, S=S, B2=2 * B, reps=args.reps, tiles=tiles))
    print("---- tools/patchgan_bench.py ----")
    print(f"# VQLPIPSWithDiscriminator on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; batch {B} pairs of {S} x {S}, precision bf16x3 "
          f"(fp16-pair planes), median of {args.reps} event-timed calls after 3 warm ones")
    x = torch.rand(B, 3, S, S, device="cuda") * 2 - 1
    y = (0.5 * x + 0.5 * (torch.rand(B, 3, S, S, device="cuda") * 2 - 1)).clamp(-1, 1)
    q = torch.tensor(0.25, device="cuda")
    t0 = time.perf_counter()
    loss = VQLPIPSWithDiscriminator(disc_start=0)
    patchgan_ref.fill(loss.discriminator)
    lpips_ref.fill(loss.perceptual_loss)
    loss = loss.cuda()
    disc = loss.discriminator
    (l0, log0), (l1, log1) = loss.evaluate(q, x, y, 1, split="val")
    torch.cuda.synchronize()
    plan = disc._plans[(B, S, S, True)][0]
    n_ops = sum(len(p.ops) for p in plan.progs)
    n_kern = len(plan.steps) - len(plan.progs)
    print(f"first evaluate, with filling the weights, planning and both captures: {time.perf_counter() - t0:.1f} s")
    print(f"discriminator graph: {n_kern} kernels of csrc/patchgan.hip (1 stem, {len(plan.progs)} affines, 1 head, terms, finish) + {n_ops} program ops in "
          f"{len(plan.progs)} slice programs (PACK + conv GEMM each); planes {plan.planes_hw}")
    print(f"values (filler weights: they mean nothing about image quality): total_loss {float(l0):.4f}, disc_loss {float(l1):.4f}, "
          f"logits_real {float(log1['val/logits_real']):.3f}, logits_fake {float(log1['val/logits_fake']):.3f}")
    sp = current_stream_ptr(x.device)
    t_eval = timed(lambda: loss.evaluate(q, x, y, 1, split="val"), args.reps)
    t_lp = timed(lambda: loss.perceptual_loss(x, y), args.reps)
    t_pair = timed(lambda: disc.pair(x, y), args.reps)
    t_graph = timed(lambda: plan.graph.launch(sp), args.reps)
    print(f"evaluate(codebook_loss, x, xrec, step), as validation_step calls it:    {fmt(t_eval)}")
    print(f"  of which LPIPS forward (its own graph, profiles/lpips.txt):           {fmt(t_lp)}")
    print(f"  of which discriminator.pair (two copies in, graph):                  {fmt(t_pair)}")
    print(f"    discriminator graph replay alone:                                  {fmt(t_graph)}")
    print(f"  the rest is torch: |x - xrec|, its mean with p_loss, the scalar combinations ({t_eval[0] - t_lp[0] - t_pair[0]:.3f} ms by difference)")
    total_k, total_p = 0.0, 0.0
    prog_i = 0
    S2 = 2 * B
    for name, what in plan.steps:
        if name == "prog":
            t = timed(lambda: what.run(sp), args.reps)
            total_p += t[0]
            hw = plan.planes_hw[prog_i + 1]
            print(f"  slice program {prog_i + 1} ({len(what.ops)} ops, output {hw[0]} x {hw[1]}), op by op (no graph): {fmt(t)}")
            prog_i += 1
            continue
        if name == "frido_disc_stem":
            h, w = plan.planes_hw[0]
            nbytes, label = 2 * B * 3 * S * S * 4 + S2 * h * w * what.ndf * 4, f"frido_disc_stem (-> {h} x {w} x {what.ndf})"
        elif name == "frido_affine_leaky":
            nbytes, label = 2 * what.rows * what.C * 4, f"frido_affine_leaky after program {prog_i} ({what.rows} rows x {what.C})"
        elif name == "frido_disc_head":
            nbytes, label = what.S * what.H * what.W * what.C * 4, f"frido_disc_head ({what.H} x {what.W} x {what.C}, input counted once)"
        else:
            nbytes, label = None, name
        t = timed(lambda: pg.launch(name, what, sp), args.reps)
        total_k += t[0]
        print(f"  {label + ':':74s}{fmt(t, nbytes)}")
    print(f"  sum of the medians: the {n_kern} new launches {total_k:.3f} ms ({100 * total_k / (total_k + total_p):.0f} % of the discriminator's "
          f"launches), the {len(plan.progs)} slice programs {total_p:.3f} ms")
    sd = {k: v.detach() for k, v in disc.state_dict().items()}
    with torch.no_grad():
        ref = eager_terms(sd, disc.table, x, y)
        t = timed(lambda: eager_terms(sd, disc.table, x, y), args.reps)
    got = disc.pair(x, y).out
    print(f"torch fp32 eager, the same discriminator and weights on both images + the five terms:   {fmt(t)}")
    print(f"  largest relative difference between the two sets of terms (other arithmetic, no parity claim): "
          f"{float(((got - ref) / ref).abs().max()):.2e}")
    if args.test_log:
        print("\n---- errors printed by tests/test_patchgan_gpu.py (one run of the file, same box) ----")
        for line in open(args.test_log):
            line = line.strip().lstrip(".")
            if line.startswith(("disc_", "affine_leaky", "gan_terms", "conv4x4", "patchgan net", "vqlpips", "validation_step")) or " passed" in line or " failed" in line:
                print(line[:400])
        print("stem, affine, head: max abs error against float64 | bound = 2 x the float32 evaluation of the same formula on the host.")
        print("terms: error of each output relative to its scale against float64; bound = 2 x T32, the largest float32-vs-float64 difference of the")
        print("host evaluation over all cases.  conv4x4: relative to max |y| against float64, the GEMM bounds of tests/test_kernels_gpu.py.  net: logits")
        print("relative to max |logits|, bound = 8 x E32 (the restatement's largest float32-vs-float64 difference over all cases and layers); loss:")
        print("entries relative to themselves, bound = 8 x E32 of the loss restatement; the bf16-pair build gets 10 x the default build's bounds.")


if __name__ == "__main__":
    main()
