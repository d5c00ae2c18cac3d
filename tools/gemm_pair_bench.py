#!/usr/bin/env python3
"""Per-launch timing of the self-attention pair (V^T projection + folded q' projection of one LayerNorm operand): ONE grid of both
(frido_gemm_pair, FridoGemm.flags bit 28) against the two single launches, each on its own best tile.  Captured graphs of 8 passes,
median of 10 replays, the three shipped planes at B = 16 (or: python tools/gemm_pair_bench.py B C HW [C HW ...] [--nsplit 1|2]).
The decision printed is the tuner's own (frido_amd/tune.py best_pair): a pair is merged only where it wins by its margin."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.pop("FRIDO_TUNE_CACHE", None)          # time everything here, read and write no pinned choice
os.environ["FRIDO_TUNE"], os.environ["FRIDO_TUNE_ON_MISS"] = "1", "tune"
from frido_amd import tune  # noqa: E402
from frido_amd.builder import Builder  # noqa: E402
from frido_amd.engine import require_gpu, rup  # noqa: E402


def main():
    a = sys.argv[1:]
    ns = 2
    if "--nsplit" in a:
        i = a.index("--nsplit")
        ns = int(a[i + 1])
        del a[i:i + 2]
    B = int(a[0]) if a else 16
    planes = [(int(a[i]), int(a[i + 1])) for i in range(1, len(a) - 1, 2)] or [(384, 1024), (576, 256), (960, 64)]
    dev = require_gpu("cuda:0")
    print(f"B = {B}, nsplit = {ns}; times in us per launch pair (median of 10 graph replays of 8 passes)")
    for C, HW in planes:
        b = Builder(dev, ns, {})
        n1 = b.op(B * HW, C)
        wv, wq = b.persistent_op(C, C, zero=True), b.persistent_op(C, C, zero=True)
        vT = b.persistent_op(C, rup(HW, 32), batch=B, zero=True)
        m = {}
        real = tune.best_pair
        tune.best_pair = lambda sa, sb, d: real(sa, sb, d, measure=m, reps=10)
        try:
            with b.gemm_pair():
                b.v_transposed(n1, C, wv, B, HW, C, out=vT)
                b.linear(n1, None, wop=wq, bias=False, out="op")
        finally:
            tune.best_pair = real
        vt, q = m["tiles"][:2], m["tiles"][2:]
        gain = 100.0 * (m["single_ms"] / m["pair_ms"] - 1.0)
        merged = bool(b.prog.ops[0][1].flags >> 28 & 1)
        print(f"C {C:4d} HW {HW:5d}: V^T (tile {vt[0]}, splitk {vt[1]}) + q' (tile {q[0]}, splitk {q[1]}) = {m['single_ms'] * 1e3:7.1f}   "
              f"pair (tile {m['tile']}, {'q first' if m['swap'] else 'V^T first'}) = {m['pair_ms'] * 1e3:7.1f}   {gain:+6.1f} %   "
              f"-> {'MERGED' if merged else 'left as two launches'}")
        print("    pair by tile / order: " + "  ".join(f"{t}{'q' if s else 'v'}:{dt * 1e3:.1f}" for t, s, dt in m["every"] if dt is not None))


if __name__ == "__main__":
    main()
