#!/usr/bin/env python3
"""Time of one MS-VQGAN reconstruction (image -> quantised latent + codebook loss -> image) on the f8f4 first stage (VQ_F8F4) at B = 16,
256 x 256: MSFPNVQModel.forward's one captured graph next to the only way the code before it can produce the same image,
VQModelInterface.decode(VQModelInterface.encode(x)).  Appends to profiles/msvq_reconstruct.txt (--out).

    python tools/msvq_reconstruct_bench.py --drive --parent DIR [--out FILE]      # the whole measurement
    python tools/msvq_reconstruct_bench.py --arms graph,api,composed,aux [--repo DIR]      # one process, one tree

--drive starts one child process per tree and round, alternating: the tree in --parent (a built export of the parent commit; it only has
the `composed` arm) and this one.  Only one process has the GPU at a time and each runs under `timeout -k 10`; a child that fails ends the
measurement.  Each tree keeps its tuned tiles in a cache file of its own under --scratch, so only its first child tunes.

Every figure: device milliseconds between two HIP events on the launch stream around `--calls` (20) back-to-back calls after 3 warm ones,
divided by the calls; `--rounds` (3) such rounds per process, all reported.
Arms:
  graph      DecoderRuntime.reconstruct(x): copy-in, ONE graph replay (encode program, loss launcher, decode program), result clones
  api        MSFPNVQModel.forward(x): the same through the public call (automatic plane selection polls the status word: one stream
             synchronise per call)
  composed   DecoderRuntime.decode(DecoderRuntime.encode(x)) of VQModelInterface: two eager programs, the pre-quant latent in between
  composed-api   VQModelInterface.decode(VQModelInterface.encode(x))
  aux        forward under use_aux_loss (ONE decoder program at batch 3B) / aux3: the same three images from one reconstruct + two
             separate decode(quant, masked) calls at batch B
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(HERE), help="the tree to import frido_amd from")
    ap.add_argument("--arms", default="graph,api,composed,composed-api,aux,aux3")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--json", default=None, help="write this process's figures here")
    ap.add_argument("--drive", action="store_true")
    ap.add_argument("--parent", default=None, help="--drive: a built export of the parent commit")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "msvq_reconstruct_bench"), help="child results and per-tree tile caches")
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def measure(args):
    sys.path.insert(0, args.repo)
    import torch
    from frido_amd import _lib, configs, synth
    from frido_amd.models import VQModelInterface
    import frido_amd.models as M
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda")
    dummy = dict(target="taming.modules.losses.DummyLoss")
    B, S = args.batch, args.size
    x = torch.from_numpy(synth.seeded_normal("bench:msvq:img", (B, 3, S, S))).tanh().to(dev)
    arms, want = {}, args.arms.split(",")
    has_new = hasattr(M, "MSFPNVQModel")
    if has_new and any(a in want for a in ("graph", "api", "aux3")):
        m = synth.fill_module(M.MSFPNVQModel(**dict(configs.VQ_F8F4, lossconfig=dummy)), "first_stage_model.").to(dev).eval()
        with _lib.use_planes(m.planes):
            rt = m.runtime()
        arms["graph"] = lambda: rt.reconstruct(x)[0]
        arms["api"] = lambda: m(x)[0]
        e, Ct = m.embed_dim, sum(m.embed_dim)

        def aux3():
            dec, quant, _, _ = rt.reconstruct(x)
            qa, qb = quant.clone(), quant.clone()
            qa[:, :Ct - e[-1]] = 0
            qb[:, e[-1]:] = 0
            return rt.decode_quant(qa), rt.decode_quant(qb), dec
        arms["aux3"] = lambda: aux3()[0]
    if has_new and "aux" in want:
        ma = synth.fill_module(M.MSFPNVQModel(**dict(configs.VQ_F8F4, lossconfig=dummy, use_aux_loss=True)), "first_stage_model.").to(dev).eval()
        with _lib.use_planes(ma.planes):
            rta = ma.runtime()
        arms["aux"] = lambda: rta.reconstruct(x, aux=True)[0]
    if any(a.startswith("composed") for a in want):
        v = synth.fill_module(VQModelInterface(**dict(configs.VQ_F8F4, lossconfig=dummy)), "first_stage_model.").to(dev).eval()
        with _lib.use_planes(v.planes):
            rv = v.runtime()
        arms["composed"] = lambda: rv.decode(rv.encode(x))
        arms["composed-api"] = lambda: v.decode(v.encode(x))
    arms = {k: arms[k] for k in want if k in arms}
    for fn in arms.values():           # warm: plans, tuner, graphs
        for _ in range(3):
            out = fn()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.calls)
    res = dict(repo=args.repo, device=torch.cuda.get_device_name(0), B=B, size=S, calls=args.calls, ms=ms)
    if "graph" in arms and "composed" in arms:      # the two routes give the same image (the codes are the same, the route differs)
        a, b = arms["graph"](), arms["composed"]()
        res["graph_vs_composed_rel"] = float((a - b).abs().max() / b.abs().max())
    for name, v in ms.items():
        print(f"{name:13s} ms per call, per round: {', '.join(f'{q:.3f}' for q in v)}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f)
    return res


def drive(args):
    assert args.parent and os.path.exists(os.path.join(args.parent, "frido_amd", "libfrido_hip.so")), "--parent: a BUILT export of the parent commit"
    os.makedirs(args.scratch, exist_ok=True)
    here = os.path.dirname(HERE)
    runs = {"parent": [], "new": []}
    for r in range(args.rounds):
        for tag, repo, arms in (("parent", args.parent, "composed,composed-api"), ("new", here, "graph,api,composed,composed-api,aux,aux3")):
            out = os.path.join(args.scratch, f"msvq_bench_{tag}_{r}.json")
            env = dict(os.environ, FRIDO_TUNE_CACHE=os.path.join(args.scratch, f"msvq_tune_{tag}.json"), FRIDO_TUNE_CACHE_READONLY="0")
            cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--repo", repo, "--arms", arms,
                   "--rounds", "1", "--calls", str(args.calls), "--batch", str(args.batch), "--size", str(args.size), "--json", out]
            print(f"[round {r}] {tag}: {' '.join(cmd[4:])}", flush=True)
            rc = subprocess.call(cmd, env=env, cwd=repo)
            if rc != 0:
                raise SystemExit(f"the {tag} child of round {r} ended with status {rc}: nothing more is started")
            runs[tag].append(json.load(open(out)))
    one = lambda tag, arm: [run["ms"][arm][0] for run in runs[tag] if arm in run["ms"]]
    lines = [f"f8f4 MS-VQGAN (VQ_F8F4, bf16x3), B = {args.batch}, {args.size} x {args.size}, {runs['new'][0]['device']}",
             f"ms per call: device time between two HIP events around {args.calls} back-to-back calls after 3 warm ones; {args.rounds} rounds, one process "
             "per tree and round, parent and new alternating (one GPU process at a time)"]
    for tag, arm, what in (("new", "graph", "one-graph reconstruct (forward's graph replay)"), ("new", "api", "MSFPNVQModel.forward (public call)"),
                           ("parent", "composed", "PARENT: runtime decode(encode(x))"), ("parent", "composed-api", "PARENT: VQModelInterface.decode(encode(x))"),
                           ("new", "composed", "new tree: runtime decode(encode(x))"), ("new", "composed-api", "new tree: VQModelInterface.decode(encode(x))"),
                           ("new", "aux", "use_aux_loss: ONE decoder program at 3B"), ("new", "aux3", "the same images: reconstruct + two separate decodes")):
        v = one(tag, arm)
        if v:
            lines.append(f"{what:58s} {', '.join(f'{q:.3f}' for q in v)}   median {statistics.median(v):.3f}  spread {max(v) - min(v):.3f}")
    g, c = one("new", "graph"), one("parent", "composed")
    if g and c:
        d, spread = statistics.median(g) - statistics.median(c), max(c) - min(c)
        lines.append(f"one graph - parent composed = {d:+.3f} ms ({100 * d / statistics.median(c):+.2f} %); the composed path's own run-to-run spread: {spread:.3f} ms -> "
                     + ("not slower beyond that spread" if d <= spread else "SLOWER than the composed path by more than its spread"))
    a, a3 = one("new", "aux"), one("new", "aux3")
    if a and a3:
        lines.append(f"3B aux decode - three separate decodes = {statistics.median(a) - statistics.median(a3):+.3f} ms")
    if "graph_vs_composed_rel" in runs["new"][0]:
        lines.append(f"same image: one graph vs composed route, max-abs relative {runs['new'][0]['graph_vs_composed_rel']:.2e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    a = _args()
    drive(a) if a.drive else measure(a)
