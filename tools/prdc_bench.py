"""Times precision / recall / density / coverage of frido_amd/manifold.py on the MI355X and writes the report profiles/prdc.txt is:
prdc at N = M = 10 000 and 50 000 rows per side, D = 2048, k = 3, beside the same quantities composed from torch float64 on the same
card (torch.cdist in row batches, kthvalue, comparisons), with the run-to-run spread of each; the split of a call between the three
passes of frido_rows_dot and the four kernels of csrc/manifold.hip; each scan kernel's achieved bytes/s on one slab; and -- with
--test-log -- the lines tests/test_manifold_gpu.py printed in the same run.  Inputs are seeded normal rows: times do not depend on
them, and the values mean nothing about image quality.

    python -m pytest tests/test_manifold_gpu.py -m gpu -s > manifold_tests.log
    python tools/prdc_bench.py [--rounds 7] [--rows 10000 50000] [--test-log manifold_tests.log] > profiles/prdc.txt

The HIP path and the torch composition are timed ALTERNATELY, round by round, in one process (a host clock around work that ends in a
device synchronise: what a caller waits for); the spread is min / max over the rounds after one warm round.  The launches alone are
device-event intervals.  Needs the GPU (there is no CPU path to time)."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

HEAD = """Precision / recall / density / coverage (frido_amd/manifold.py + csrc/manifold.hip, dot products by frido_rows_dot) on one MI355X: what
was run, what was seen, what was not run.

What was run
  1. python -m pytest tests/test_manifold_gpu.py -m gpu -s      (the lines it printed are listed at the end)
  2. python tools/prdc_bench.py --test-log <that log>           (output below)
Both in one process each, on a shared box, profiler off.  Whole calls are timed with a host clock around work that ends in a device
synchronise, the HIP path and the torch float64 composition ALTERNATELY round by round, {rounds} rounds after one warm round: median
(min, max) -- the min .. max range is the run-to-run spread inside this one run.  The launches alone are device-event intervals.

What was NOT run
  - Other feature widths and neighbourhoods; the bf16-pair build (the code is the same f32 / f64 code in both builds).
  - No rocprofv3 trace: a kernel's rate is the bytes its algorithm reads over an event-timed launch, not a kernel time from a trace.
  - No trained weights exist here and neither torch-fidelity nor prdc is installed: nothing below is a quality number, and the metric
    is held to its written formulas, not to those packages.
  - One run on one box: the spread between boxes was not measured.  There is no pass mark on these times.

The torch float64 lines compose the same quantities on the same card in the same process: torch.cdist (float64, Euclidean, with its
square root) of row batches against the other side, kthvalue(k + 1) for the radii, <= comparisons and sums for the counts.  torch
rounds its distances in an order of its own, so a membership that sits on a rounding error may fall differently: the counts of both
are printed.
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


def events(fn, reps, warm=1):
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


def prdc_torch(real, fake, k, batch):
    """The four counts from torch float64 on the device: cdist in batches of `batch` rows, kthvalue, comparisons."""
    R, G = real.double(), fake.double()

    def radii(X):
        return torch.cat([torch.cdist(X[i:i + batch], X).kthvalue(k + 1, dim=1).values for i in range(0, X.shape[0], batch)])

    rr, rg = radii(R), radii(G)
    cnt_col = torch.zeros(R.shape[0], dtype=torch.int64, device=R.device)
    dmin = torch.full((R.shape[0],), float("inf"), dtype=torch.float64, device=R.device)
    cnts = []
    for i in range(0, G.shape[0], batch):
        d = torch.cdist(G[i:i + batch], R)
        cnts.append((d <= rr[None, :]).sum(dim=1))
        cnt_col += (d <= rg[i:i + batch, None]).sum(dim=0)
        dmin = torch.minimum(dmin, d.min(dim=0).values)
    cnt = torch.cat(cnts)
    c = torch.stack([(cnt > 0).sum(), cnt.sum(), (cnt_col > 0).sum(), (dmin <= rr).sum()]).cpu().tolist()
    return dict(precision=c[0], density=c[1], recall=c[2], coverage=c[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 50000], help="rows per side")
    ap.add_argument("--batch", type=int, default=2048, help="rows per torch.cdist call of the composition")
    ap.add_argument("--test-log", default=None, help="output of `pytest tests/test_manifold_gpu.py -m gpu -s`: its lines are appended")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/prdc_bench.py: no HIP device; nothing was measured")
    from frido_amd import fidelity as fd
    from frido_amd import manifold as mf

    print(HEAD.format(rounds=args.rounds))
    print("---- tools/prdc_bench.py ----")
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} alternating rounds after one warm round")
    dev = torch.device("cuda")
    D, k = 2048, 3
    verdicts, notes = [], []
    for n in args.rows:
        g = torch.Generator(device="cpu").manual_seed(2020 + n)
        a = torch.randn(n, D, generator=g).to(dev)
        b = (torch.randn(n, D, generator=g) * 0.9 + 0.35).to(dev)
        ms, res = alternate({"hip": lambda: mf.prdc(a, b, k), "torch": lambda: prdc_torch(a, b, k, args.batch)}, args.rounds)
        hc = {m: res["hip"]["counts"][m] for m in ("precision", "density", "recall", "coverage")}
        print(f"\nprdc, N = M = {n}, D = {D}, k = {k}, slab {mf.SLAB_BYTES >> 20} MiB")
        print(f"  frido_amd.manifold.prdc                        {fmt(ms['hip'])}   -> counts {hc}")
        print(f"  torch float64 composition, {args.batch} rows a batch     {fmt(ms['torch'])}   -> counts {res['torch']}")
        verdicts.append(verdict(f"prdc at {n} rows per side", ms["hip"], ms["torch"]))

        # ---- the split: the three passes of frido_rows_dot alone, and every kernel of manifold.hip alone on ONE slab ----
        sp = torch.cuda.current_stream().cuda_stream
        ldo = (n + 1) // 2 * 2
        rows = mf._slab_rows("prdc", n, ldo, mf.SLAB_BYTES, None)
        nslabs = -(-n // rows)
        slab = torch.empty(rows * ldo, dtype=torch.float64, device=dev)

        def dots():
            for _ in range(3):
                for a0 in range(0, n, rows):
                    r = min(rows, n - a0)
                    fd.launch("frido_rows_dot", fd.rows_dot_desc(a.data_ptr() + a0 * D * 4, b.data_ptr(), r, n, D, mode=fd.STORE_F64,
                                                                 out=slab.data_ptr(), ldo=ldo), sp)

        t_dots = events(dots, args.rounds)
        flop = 3 * 2.0 * n * n * D
        print(f"  the 3 passes of frido_rows_dot alone ({3 * nslabs} launches)   {fmt(t_dots)}   = {flop / statistics.median(t_dots) / 1e9:.2f} TFLOP/s f64")
        na, nb = mf.row_sqnorms(a), mf.row_sqnorms(b)
        fd.launch("frido_rows_dot", fd.rows_dot_desc(a.data_ptr(), a.data_ptr(), rows, n, D, mode=fd.STORE_F64, out=slab.data_ptr(), ldo=ldo), sp)
        rad = torch.empty(n, dtype=torch.float64, device=dev)
        out64 = torch.empty(n, dtype=torch.float64, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        cnt_col = torch.zeros(n, dtype=torch.int32, device=dev)
        dmin = torch.full((n,), float("inf"), dtype=torch.float64, device=dev)
        slab_bytes = rows * n * 8.0
        # (launcher, descriptor, launches of it per prdc in units of this one, bytes the algorithm reads per launch, what they are)
        kernels = [
            ("frido_row_sqnorm", mf.row_sqnorm_desc(a.data_ptr(), out64.data_ptr(), n, D), 2.0, n * D * 4.0, f"{n} rows of {D} f32"),
            ("frido_knn_select", mf.knn_select_desc(slab.data_ptr(), na.data_ptr(), na.data_ptr(), rad.data_ptr(), rows, n, ldo, k + 1),
             2.0 * n / rows, (k + 1) * slab_bytes, f"the slab of {rows} rows, K = {k + 1} times"),
            ("frido_ball_rows", mf.ball_rows_desc(slab.data_ptr(), na.data_ptr(), nb.data_ptr(), rad.data_ptr(), cnt.data_ptr(), rows, n, ldo),
             1.0 * n / rows, slab_bytes, f"the slab of {rows} rows once"),
            ("frido_ball_cols", mf.ball_cols_desc(slab.data_ptr(), na.data_ptr(), nb.data_ptr(), rad.data_ptr(), cnt_col.data_ptr(), dmin.data_ptr(),
                                                  rows, n, ldo), 1.0 * n / rows, slab_bytes, f"the slab of {rows} rows once"),
        ]
        mf.launch("frido_knn_select", kernels[1][1], sp)                      # radii for the ball scans to compare against
        scans_ms = 0.0
        for name, desc, per_call, nbytes, what in kernels:
            t = events(lambda: mf.launch(name, desc, sp), args.rounds)
            med = statistics.median(t)
            scans_ms += med * per_call
            rate = nbytes / med / 1e9
            print(f"  {name:18s} launched alone   {fmt(t)}   reads {nbytes / 1e6:.1f} MB ({what}) = {rate:.3f} TB/s; x {per_call:.1f} per call")
            if name != "frido_row_sqnorm" and rate < 3.0:
                notes.append((n, name, rate))
        td, th = statistics.median(t_dots), statistics.median(ms["hip"])
        print(f"  split of a call: dot products {td:.1f} ms + scans {scans_ms:.1f} ms (launched alone, scaled to the call's {nslabs} slabs a pass) = "
              f"{td + scans_ms:.1f} ms of the {th:.1f} ms a call takes; the scans are {100 * scans_ms / (td + scans_ms):.1f} % of that sum")
        print(f"  expectation written before the run: 3 x 2 N^2 D flops at 35 TFLOP/s = {flop / 35e12 * 1e3:.0f} ms, plus a few per cent for the scans")
        del a, b, slab
    print("\nWhich one happened")
    for v in verdicts:
        print("  " + v)
    if any("SLOWER" in v for v in verdicts):
        print("  Why prdc is slower: its time is frido_rows_dot's, which runs its FMAs on the vector pipe (v_fma_f64, with two f32 -> f64\n"
              "  conversions per four FMAs) in the in-order chain the specification fixes, while torch.cdist runs rocBLAS's float64 matrix-core\n"
              "  kernels, which sum in an order of their own.  The f64 MFMA is out of scope here; no speed is claimed for prdc.")
    for n, name, rate in notes:
        print(f"  {name} at {n} rows reads {rate:.2f} TB/s, below the 3 - 6 TB/s of the other metric kernels (see the README section for why)")
    if args.test_log and os.path.exists(args.test_log):
        print("\n---- lines printed by tests/test_manifold_gpu.py in the same run ----")
        for ln in open(args.test_log):
            ln = ln.lstrip(".")      # pytest -q prints its progress dots in front of a test's own output
            if ln.startswith(("prdc ", "variant ", "end to end ")) or " passed" in ln or " failed" in ln:
                print(ln.rstrip())


if __name__ == "__main__":
    main()
