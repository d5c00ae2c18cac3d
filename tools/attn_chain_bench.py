#!/usr/bin/env python3
"""The attention section of a 32x32-plane transformer block of the bf16x3 sampler on its real shapes (B = 16, 1024 tokens, d = 384, 26
context tokens), as the plan emits it: self-attention + norm2 (flash kernel), cross-attention + operand copy + norm3 (short-key kernel) --
against the one flash launch that carries the cross tail (builder.ATTN_CHAIN).  Both programs are timed in ONE process, interleaved over
ROUNDS rounds (median and min per program).     python tools/attn_chain_bench.py [B]      FRIDO_LIB selects the library."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from frido_amd import builder as builder_mod  # noqa: E402
from frido_amd.builder import Builder  # noqa: E402

DEV = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
NQ, D, NCTX, ROUNDS, REPS = 1024, 384, 26, 7, 40
KEEP = []


def rand_op(b, rows, K, pad_from=None):
    x = torch.randn(rows, K, device=DEV)
    if pad_from is not None:
        x[:, pad_from:] = 0
    KEEP.append(x)
    return b.pack(x.data_ptr(), 1, rows, K, 0, K)


def program(chain):
    builder_mod.ATTN_CHAIN = chain
    w = {n: torch.randn(D, device=DEV) for n in ("n2.weight", "n2.bias", "n3.weight", "n3.bias")}
    b = Builder(DEV, 2, w)
    n1, qp = rand_op(b, B * NQ, D), rand_op(b, B * NQ, D)
    vT, kc, vTc = rand_op(b, B * D, NQ), rand_op(b, B * NCTX, D), rand_op(b, B * D, 32, pad_from=NCTX)
    bias = torch.randn(2, D, device=DEV)
    KEEP.append(bias)
    hcur = b.f32(B * NQ, D)
    hcur.view().normal_()
    b.prog.run(torch.cuda.current_stream().cuda_stream)      # fill the operands, then time the attention section alone
    torch.cuda.synchronize()
    b.prog.ops.clear()
    b.prog._packed = None
    if b.attention_chain_ok(D, D, NQ, D, NCTX, D):
        b.attention_chain(qp, D, n1, D, vT, B, NQ, NQ, D, bias_ptr=bias[0].data_ptr(), residual=hcur, ln=("n2", 1e-5), k2=kc, ldk2=D, vT2=vTc,
                          Nk2=NCTX, bias2_ptr=bias[1].data_ptr(), ln2=("n3", 1e-5), also_op=True, stream_dead=True)
    else:
        h2 = b.attention(qp, D, n1, D, vT, B, NQ, NQ, D, bias_ptr=bias[0].data_ptr(), residual=hcur, stream=True, ln=("n2", 1e-5))
        b.attention(h2.ln_copy, D, kc, D, vTc, B, NQ, NCTX, D, bias_ptr=bias[1].data_ptr(), residual=h2, stream=True, also_op=True,
                    ln=("n3", 1e-5), stream_dead=True)
    return b


def timed(b):
    s = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        b.prog.run(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


if __name__ == "__main__":
    progs = {"two launches": program(False), "one launch": program(True)}
    for name, b in progs.items():
        print(f"{name}: {len(b.prog.ops)} op(s)")
        timed(b)
    t = {name: [] for name in progs}
    for _ in range(ROUNDS):
        for name, b in progs.items():
            t[name].append(timed(b))
    for name, v in t.items():
        print(f"{name:13s} B={B}: median {statistics.median(v):7.1f} us  min {min(v):7.1f} us  per section ({ROUNDS} rounds x {REPS} runs)")
