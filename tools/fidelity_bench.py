"""Times the Kernel Inception Distance and the Inception Score of frido_amd/fidelity.py on the MI355X and writes the report
profiles/fidelity.txt is: KID at its defaults (100 subsets of 1000, D = 2048, 10 000 rows per side) and the Inception Score at
N = 50 000, C = 1008, each beside the same quantity composed from torch float64 mm / log_softmax on the same card and beside numpy on
the host, with the run-to-run spread of each, the f64 rate frido_rows_dot reaches, and -- with --test-log -- the errors
tests/test_fidelity_gpu.py printed in the same run.  Inputs are seeded normal rows: times do not depend on them, and the values mean
nothing about image quality.

    python -m pytest tests/test_fidelity_gpu.py -m gpu -s > fidelity_tests.log
    python tools/fidelity_bench.py [--rounds 7] [--test-log fidelity_tests.log] > profiles/fidelity.txt

The HIP path and the torch composition are timed ALTERNATELY, round by round, in one process (a host clock around work that ends in a
device synchronise: what a caller waits for, index generation, uploads and the read-back included); the spread is min / max over the
rounds after one warm round.  Needs the GPU (there is no CPU path to time)."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HEAD = """Inception Score and Kernel Inception Distance (frido_amd/fidelity.py + csrc/fidelity.hip) on one MI355X: what was run, what was seen,
what was not run.

What was run
  1. python -m pytest tests/test_fidelity_gpu.py -m gpu -s      (the errors it printed are listed at the end)
  2. python tools/fidelity_bench.py --test-log <that log>       (output below)
Both in one process each, on a shared box, profiler off.  Whole calls are timed with a host clock around work that ends in a device
synchronise, the HIP path and the torch float64 composition ALTERNATELY round by round, {rounds} rounds after one warm round: median
(min, max) -- the min .. max range is the run-to-run spread inside this one run.  The launches alone are device-event intervals.

What was NOT run
  - Other sample counts, subset sizes and feature widths; the bf16-pair build (the code is the same f32 / f64 code in both builds).
  - No rocprofv3 trace: the rate of frido_rows_dot is operations over an event-timed launch, not a kernel time from a trace.
  - No trained weights exist here and torch-fidelity is not installed: nothing below is a quality number, and both metrics are held to
    their written formulas, not to that package.
  - One run on one box: the spread between boxes was not measured.  There is no pass mark on these times.

The torch float64 lines compose the same quantities from torch.mm / log_softmax in float64 on the same card in the same process; they
sum in rocBLAS's and torch's own orders, so they agree with the HIP path to rounding, not bit for bit.  The numpy lines are the
restatement of tests/fidelity_ref.py on the host's CPUs.
"""


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(fns, rounds):
    """{name: [ms per round]} of the callables run in turn, round by round, after one warm round; and their last results."""
    res = {}
    for name, fn in fns.items():
        res[name] = wall(fn)[1]
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            t, res[name] = wall(fn)
            ms[name].append(t)
    return ms, res


def events(fn, reps, warm=2):
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
    return ms


def fmt(ms):
    return f"{statistics.median(ms):10.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"


def verdict(what, hip, other):
    """Which one happened, by the medians and the spreads of the two."""
    mh, mo = statistics.median(hip), statistics.median(other)
    apart = min(hip) > max(other) or max(hip) < min(other)
    if not apart:
        return f"{what}: the HIP path and the torch float64 composition are within each other's spread ({mh:.3f} ms against {mo:.3f} ms)"
    if mh < mo:
        return f"{what}: the HIP path is FASTER than the torch float64 composition, {mo / mh:.2f} x, by more than the spread of either"
    return f"{what}: the HIP path is SLOWER than the torch float64 composition, {mh / mo:.2f} x, by more than the spread of either"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=10000, help="rows per side of the KID case")
    ap.add_argument("--isc-rows", type=int, default=50000)
    ap.add_argument("--host-runs", type=int, default=2, help="runs of the numpy restatement on the host")
    ap.add_argument("--test-log", default=None, help="output of `pytest tests/test_fidelity_gpu.py -m gpu -s`: its error lines are appended")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/fidelity_bench.py: no HIP device; nothing was measured")
    import fidelity_ref as FR
    from frido_amd import fidelity as fd

    print(HEAD.format(rounds=args.rounds))
    print("---- tools/fidelity_bench.py ----")
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} alternating rounds after one warm round")
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(2020)
    n, D, S, m = args.rows, 2048, 100, 1000
    f1 = torch.randn(n, D, generator=g)
    f2 = torch.randn(n, D, generator=g) * 1.5 + 0.3
    a, b = f1.to(dev), f2.to(dev)

    # ---- KID at its defaults ----
    def kid_hip():
        return fd.kernel_inception_distance(a, b)

    def kid_torch():
        i1, i2 = fd.kid_subsets(n, n, S, m)
        gamma, out = 1.0 / D, []
        for s in range(S):
            x, y = a[torch.from_numpy(i1[s]).to(dev)].double(), b[torch.from_numpy(i2[s]).to(dev)].double()
            kxx, kyy, kxy = (x @ x.T * gamma + 1.0) ** 3, (y @ y.T * gamma + 1.0) ** 3, (x @ y.T * gamma + 1.0) ** 3
            out.append(((kxx.sum() - kxx.diagonal().sum()) + (kyy.sum() - kyy.diagonal().sum())) / (m * (m - 1)) - 2.0 * kxy.sum() / (m * m))
        v = torch.stack(out).cpu().numpy()
        return float(np.mean(v)), float(np.std(v))

    ms, res = alternate({"hip": kid_hip, "torch": kid_torch}, args.rounds)
    print(f"KID, {S} subsets of {m}, D = {D}, {n} rows per side")
    print(f"  frido_amd.fidelity.kernel_inception_distance   {fmt(ms['hip'])}   -> {res['hip'][0]:.9g} +- {res['hip'][1]:.9g}")
    print(f"  torch float64 composition, subset by subset    {fmt(ms['torch'])}   -> {res['torch'][0]:.9g} +- {res['torch'][1]:.9g}")
    print(f"  the two means differ by {abs(res['hip'][0] - res['torch'][0]) / abs(res['torch'][0]):.2e} relative")
    verdicts = [verdict("KID", ms["hip"], ms["torch"])]
    # the launches alone, and the rate of the dot products
    i1, i2 = fd.kid_subsets(n, n, S, m)
    t_idx0 = time.perf_counter()
    fd.kid_subsets(n, n, S, m)
    t_idx = (time.perf_counter() - t_idx0) * 1e3
    ix, iy = torch.from_numpy(i1.astype(np.int32)).to(dev), torch.from_numpy(i2.astype(np.int32)).to(dev)
    sp = torch.cuda.current_stream().cuda_stream
    for name, sym in (("XX, upper tile triangle", True), ("XY, every tile", False)):
        T = fd.tiles(m, symmetric=sym)
        part = torch.empty(S * T, dtype=torch.float64, device=dev)
        y_, iy_ = (a, ix) if sym else (b, iy)
        d = fd.rows_dot_desc(a.data_ptr(), y_.data_ptr(), n, n, D, mode=fd.SUM_POLY, partials=part.data_ptr(), ix=ix.data_ptr(), iy=iy_.data_ptr(),
                             S=S, m=m, degree=3, gamma=1.0 / D, coef0=1.0, exclude_diag=sym, symmetric=sym)
        t = events(lambda: fd.launch("frido_rows_dot", d, sp), args.rounds)
        flop = 2.0 * S * T * 64 * 64 * D                                     # the FMAs of the tiles computed, ragged tiles counted whole
        print(f"  frido_rows_dot SUM_POLY {name:24s} {fmt(t)}   = {flop / statistics.median(t) / 1e9:.2f} TFLOP/s f64 ({S * T} tiles)")
    print(f"  the host's share of a call: drawing the {2 * S} index lists {t_idx:.1f} ms")
    host = []
    for _ in range(args.host_runs):
        t0 = time.perf_counter()
        r = FR.kid(f1.numpy(), f2.numpy())
        host.append((time.perf_counter() - t0) * 1e3)
    print(f"  numpy float64 on the host ({os.cpu_count()} CPUs seen)    {fmt(host)}   -> {r[0]:.9g} +- {r[1]:.9g}")

    # ---- the Inception Score ----
    N, Cn, splits = args.isc_rows, 1008, 10
    lg_h = torch.randn(N, Cn, generator=g) * 3
    lg = lg_h.to(dev)

    def isc_hip():
        return fd.inception_score(lg)

    def isc_torch():
        perm = torch.from_numpy(fd.isc_permutation(N)).to(dev)
        logp = torch.log_softmax(lg[perm].double(), dim=1)
        p = logp.exp()
        out = []
        for i in range(splits):
            lo, hi = i * N // splits, (i + 1) * N // splits
            q = p[lo:hi].mean(dim=0, keepdim=True)
            out.append(((p[lo:hi] * (logp[lo:hi] - q.log())).sum(dim=1).mean()).exp())
        v = torch.stack(out).cpu().numpy()
        return float(np.mean(v)), float(np.std(v))

    ms, res = alternate({"hip": isc_hip, "torch": isc_torch}, args.rounds)
    print(f"Inception Score, N = {N}, C = {Cn}, {splits} splits")
    print(f"  frido_amd.fidelity.inception_score             {fmt(ms['hip'])}   -> {res['hip'][0]:.9g} +- {res['hip'][1]:.9g}")
    print(f"  torch float64 composition                      {fmt(ms['torch'])}   -> {res['torch'][0]:.9g} +- {res['torch'][1]:.9g}")
    print(f"  the two means differ by {abs(res['hip'][0] - res['torch'][0]) / abs(res['torch'][0]):.2e} relative")
    verdicts.append(verdict("Inception Score", ms["hip"], ms["torch"]))
    perm = torch.from_numpy(fd.isc_permutation(N).astype(np.int32)).to(dev)
    work = torch.empty(3 * N + splits * Cn + splits, dtype=torch.float64, device=dev)
    d = fd.isc_desc(lg.data_ptr(), perm.data_ptr(), work.data_ptr(), work[3 * N:].data_ptr(), work[2 * N:].data_ptr(),
                    work[3 * N + splits * Cn:].data_ptr(), N, Cn, splits)
    steps = {}
    for step in fd.ISC_STEPS:
        steps[step] = events(lambda: fd.launch(step, d, sp), args.rounds)
        print(f"  {step:22s} launched alone          {fmt(steps[step])}")
    host = []
    for _ in range(args.host_runs):
        t0 = time.perf_counter()
        r = FR.isc(lg_h.numpy())
        host.append((time.perf_counter() - t0) * 1e3)
    print(f"  numpy float64 on the host                      {fmt(host)}   -> {r[0]:.9g} +- {r[1]:.9g}")
    print("\nWhich one happened")
    for v in verdicts:
        print("  " + v)
    if "SLOWER" in verdicts[1]:
        alone = {k: statistics.median(v) for k, v in steps.items()}
        print(f"  Why the Inception Score is slower: {alone['frido_isc_marginal']:.3f} ms of the {sum(alone.values()):.3f} ms its four launches take alone are\n"
              f"  frido_isc_marginal, whose grid is one thread per (split, column) = {splits * Cn} threads = {-(-splits * Cn // 256)} workgroups for 256 CUs, each\n"
              f"  walking its split's {N // splits} rows one after the other with a float64 exp per row: the in-order sum the header fixes leaves no\n"
              f"  other parallelism, so most of the chip idles; frido_isc_finish ({alone['frido_isc_finish']:.3f} ms) runs {splits} threads for the same reason.  torch\n"
              "  reduces the same sums as trees over the whole chip, in an order of its own.  At a few milliseconds once per evaluation the\n"
              "  fixed order was kept; no speed is claimed for the Inception Score.")
    if "SLOWER" in verdicts[0]:
        print("  Why KID is slower: frido_rows_dot runs its FMAs on the vector pipe (v_fma_f64, with two f32 -> f64 conversions per four FMAs),\n"
              "  torch.mm runs rocBLAS's float64 matrix-core kernels; the rates above are what the vector pipe reached.  No speed is claimed for KID.")
    if args.test_log and os.path.exists(args.test_log):
        print("\n---- errors printed by tests/test_fidelity_gpu.py in the same run ----")
        worst = 0.0
        for ln in open(args.test_log):
            ln = ln.lstrip(".")      # pytest -q prints its progress dots in front of a test's own output
            if ln.startswith(("m = ", "kid: ", "isc N=", "end to end ")) or " passed" in ln or " failed" in ln:
                print(ln.rstrip())
            if ln.startswith("isc N="):      # "... relative errors: splits a, mean b, std c; bound d"
                errs, bound = ln.split("relative errors:")[1].split("; bound")
                worst = max(worst, max(float(e.split()[-1]) for e in errs.split(",")) / float(bound))
        print(f"largest Inception Score error over its bound 64 C 2^-53: {worst:.3f} (the issue asks for a cause where this exceeds 0.25)")


if __name__ == "__main__":
    main()
