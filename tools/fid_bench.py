"""Times frido_amd.models.FIDInceptionV3 on the MI355X and writes the report profiles/fid.txt is: milliseconds per call of the captured
graph, the share of the launches that are not GEMMs (the input transform, the thirteen pools, the global pool), the statistics update,
the distance on the host, the same network in torch fp32 eager beside it, and -- with --test-log -- the errors
tests/test_fid_gpu.py printed in the same run.  Weights are the deterministic filler's (no trained Inception ships here): times do
not depend on them, and the values mean nothing about image quality.

    python -m pytest tests/test_fid_gpu.py -m gpu -s > fid_tests.log
    python tools/fid_bench.py [--batch 16] [--size 256] [--reps 20] [--test-log fid_tests.log] > profiles/fid.txt

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

HEAD = """Fréchet Inception Distance (frido_amd/fid.py InceptionPlan + csrc/fid.hip) on one MI355X: what was run, what was seen, what was not run.

What was run
  1. python -m pytest tests/test_fid_gpu.py -m gpu -s      (the errors it printed are listed at the end)
  2. python tools/fid_bench.py --test-log <that log>       (batch {B} of {S} x {S} float images resized to 299 x 299; output below)
Both in one process each, on a shared box, profiler off.  Times are medians of {reps} device-event intervals after 3 warm calls
(min / max beside them); weights are the deterministic filler's, inputs uniform in [-1, 1].  GEMM tiles: {tiles}.

What was NOT run
  - Other batch sizes and image sizes, the uint8 layout, the bf16-pair build and precision="bf16": not timed (the bf16-pair build's
    errors are below).
  - No rocprofv3 trace: the split below is event-timed launches on an otherwise idle stream, not per-kernel times inside the graph.
  - No trained weights exist here and torch-fidelity is not installed: nothing below is a quality number, and the input transform is
    held to its written formula, not to that package.
  - One run on one box: the spread between boxes and between runs was not measured.  There is no pass mark on these times.

The torch fp32 eager line is the same network (F.conv2d with the folded weights, F.relu, torch's pools) on the same card in the same
process, for scale: it runs other arithmetic (MIOpen fp32) and is no parity reference.
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


def fmt(t):
    return f"{t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--test-log", default=None, help="output of `pytest tests/test_fid_gpu.py -m gpu -s`: its error lines are appended")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/fid_bench.py: no HIP device; nothing was measured")
    import inception_ref as R
    from frido_amd import fid, tune
    from frido_amd.engine import current_stream_ptr
    from frido_amd.models import FIDInceptionV3

    B, S = args.batch, args.size
    tiles = ("the pinned cache where it holds the shape" if tune.cache_is_pinned_for_this_library() else
             "tuned live at plan time (frido_amd/tune.py: the committed tile cache is keyed to an earlier build of the library, so no "
             "pinned tile applied; it holds no entry of these shapes either)")
    print(HEAD.format(B=B, S=S, reps=args.reps, tiles=tiles))
    print("---- tools/fid_bench.py ----")
    print(f"# FIDInceptionV3 on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; batch {B} of {S} x {S}, precision bf16x3 "
          f"(fp16-pair planes), median of {args.reps} event-timed calls after 3 warm ones")
    x = torch.rand(B, 3, S, S, device="cuda") * 2 - 1
    m = FIDInceptionV3()
    sd = R.fill(m)
    m = m.cuda()
    t0 = time.perf_counter()
    feats = m(x)
    torch.cuda.synchronize()
    print(f"first call (fold, pack, plan, tile choice, capture): {time.perf_counter() - t0:.1f} s")
    plan = next(iter(m._plans.values()))[0]
    sp = current_stream_ptr(x.device)
    n_prog = sum(1 for k, _ in plan.steps if k == "prog")
    n_gemm = sum(len(p.ops) for p in plan.progs)
    print(f"plan: {len(plan.steps)} steps = {n_prog} programs ({n_gemm} ops: the 94 convs and their PACKs) + {len(plan.steps) - n_prog} launches of csrc/fid.hip")
    t_graph = timed(lambda: plan.graph.launch(sp), args.reps)
    print(f"forward, captured graph, per call          {fmt(t_graph)}   = {t_graph[0] / B:.3f} ms per image")
    t_call = timed(lambda: m(x), args.reps)
    print(f"forward through the module (copy in, clone) {fmt(t_call)}")
    with fid._lib.use_planes(m.planes):
        side = {}
        for kind in ("frido_fid_preprocess", "frido_pool3", "frido_gap"):
            descs = [d for k, d in plan.steps if k == kind]
            side[kind] = timed(lambda: [fid.launch(kind, d, sp) for d in descs], args.reps)
            print(f"  {kind:22s} x {len(descs):2d}, launched alone     {fmt(side[kind])}")
        progs = timed(lambda: [p.run(sp) for p in plan.progs], args.reps)
        print(f"  the {n_prog} programs, launched alone            {fmt(progs)}")
    non_gemm = sum(t[0] for t in side.values())
    print(f"share of the non-GEMM launches: {non_gemm:.3f} ms of {non_gemm + progs[0]:.3f} ms launched alone = {100 * non_gemm / (non_gemm + progs[0]):.1f} % "
          "(the programs' PACK ops are counted with the GEMMs)")
    st = fid.FeatureStatistics(fid.FEATURES, "cuda")
    t_acc = timed(lambda: st.update(feats), args.reps)
    print(f"FeatureStatistics.update, batch {B}, D = 2048   {fmt(t_acc)}")
    big = torch.randn(64, fid.FEATURES, device="cuda")
    t_acc64 = timed(lambda: st.update(big), args.reps)
    print(f"FeatureStatistics.update, batch 64, D = 2048   {fmt(t_acc64)}   = {2 * 64 * 2048 * 2048 / t_acc64[0] / 1e6:.0f} GFLOP/s f64")
    other = fid.FeatureStatistics(fid.FEATURES, "cuda").update(torch.randn(4096, fid.FEATURES, device="cuda") * 0.5 + 0.1)
    t0 = time.perf_counter()
    d = fid.frechet_distance(st.mean(), st.cov(), other.mean(), other.cov())
    print(f"frechet_distance at D = 2048 on the host: {time.perf_counter() - t0:.2f} s (value {d:.6g}: filler features, no meaning)")

    # the same network in torch fp32 eager
    w = {k: v.cuda() for k, v in fid.folded_weights(sd, "cpu").items()}

    class Folded(R.Net):
        def bc(self, h, name, stride=1, padding=0):
            return torch.relu(torch.nn.functional.conv2d(h, w[name + ".weight"], w[name + ".bias"], stride=stride, padding=padding))

    net = Folded(None, torch.float32, True)
    pre = plan.pre.view(B, 299, 299, 3).permute(0, 3, 1, 2).contiguous()

    def eager():
        h = net.stem(pre)
        for n in R.BLOCK_NAMES:
            h = torch.cat(net.block(h, n), 1)
        return h.mean(dim=(2, 3))
    with torch.no_grad():
        t_eager = timed(eager, args.reps)
        e = eager()
    print(f"torch fp32 eager, same tower from the preprocessed input {fmt(t_eager)}   = {t_eager[0] / t_graph[0]:.2f} x the graph")
    print(f"  (its features differ from the graph's by {float((e - feats).abs().max() / feats.abs().max()):.2e} of the largest feature)")
    if args.test_log and os.path.exists(args.test_log):
        print("\n---- errors printed by tests/test_fid_gpu.py in the same run ----")
        for ln in open(args.test_log):
            ln = ln.lstrip(".")      # pytest -q prints its progress dots in front of a test's own output
            if ln.startswith(("fid_preprocess ", "conv ", "block ", "tower ", "fid end to end")) or " passed" in ln or " failed" in ln:
                print(ln.rstrip())


if __name__ == "__main__":
    main()
