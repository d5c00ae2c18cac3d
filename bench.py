#!/usr/bin/env python3
"""Headline benchmark: images/sec @ DDIM-200, COCO layout2img 256x256 (BASELINE.json), on N MI355X.

One "step" = one full pass of the hot path over one per-GPU batch of synthetic inputs: x_T draw, the
2-stage DDIM-200 loop (400 denoiser forwards, hipGraph replays), stage hand-off, MS-VQGAN decode, and (N>1)
the RCCL all-gather of decoded images.  Inputs (context) are resident in HBM when the timed region starts.

    python bench.py --gpus 1 --steps 2 --warmup 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (see the driver contract): value is whole-job images/s, ms_per_step the time of one
timed step.  A plain run sets up, warms up, times the steps and prints the line; --dump-outputs DIR also writes
what the last timed step returned (DIR/images.npy, float32).  --full adds everything else the line can carry: the
loop-only pass, "roofline" (measured live with HIP events on the launch stream around every op of one denoiser
forward), the bf16 throughput mode, BASELINE configs 3 / 5 (N = 1) or 4 (N > 1), and "cpu_baseline" (the oracle,
the CPU restatement of the reference, timed on this host's cores on a bounded sample).

    python bench.py --gpus 1 --steps 2 --warmup 1 --full
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
# pinned tile / split-K choices (frido_amd/tune.py): with the committed cache every run and every rank uses the same tiles, so
# results are bitwise repeatable and no time goes into re-tuning; a rebuilt library (different size) starts a new cache
os.environ.setdefault("FRIDO_TUNE_CACHE", os.path.join(REPO, "profiles", "tune_cache.json"))

from frido_amd import _lib, configs, synth  # noqa: E402


GEMM_FAMILY = ("igemm_kernel", "conv3x3_patch_kernel", "conv3x3_gn_kernel")      # the kernels of the MFMA implicit-GEMM family


def build_model(precision, device):
    from frido_amd.models import instantiate_from_config
    cfg = configs.frido_cfg(configs.UNET_F8F4, configs.VQ_F8F4, configs.BERT_FULL)
    cfg["cond_stage_config"] = "__is_unconditional__"    # synthetic context tensors stand in for the cond stage (§8f)
    cfg["conditioning_key"] = "crossattn"
    cfg["use_ema"] = False
    cfg["unet_config"]["params"]["precision"] = precision
    cfg["first_stage_config"]["params"]["precision"] = precision
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    # synth.fill_module's weights, generated on 8 threads: every tensor has its own generator (keyed by its name) and numpy releases the
    # GIL while it draws, so the bits are the same; on one core the draw was over half of a plain run's set-up
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool, torch.no_grad():
        for module, prefix in ((m.model, "model."), (m.first_stage_model, "first_stage_model.")):
            params = list(module.named_parameters())
            for (name, p), a in zip(params, pool.map(lambda np_, pre=prefix: synth.fill_tensor(pre + np_[0], np_[1].shape), params)):
                p.copy_(torch.from_numpy(a))
            if hasattr(module, "invalidate"):
                module.invalidate()
    return m.to(device).eval()


def family_gflop_per_forward(eng):
    """Algorithmic 2MNK of the GEMM-family launches of ONE denoiser forward, per stage (GFLOP)."""
    from frido_amd import _lib
    k_gemm = _lib.OP_KINDS["FRIDO_OP_GEMM"]
    return [sum(2.0 * st.M * st.N * (st.K + st.K2) * st.batch for kind, st in stg.step.ops if kind == k_gemm) / 1e9 for stg in eng.stages]


def trace_roofline(gflop_per_stage, peak):
    """(r06, r05 verdict next 7) The family's figure from the REPLAYED graph: the committed kernel trace of this bench command
    (tools/run_profiles.sh -> tools/gap_analysis.py `sampling_loop`: summed durations of the family's kernels between the first and the
    last update kernel of one sampling pass, and the number of forwards in that window) against this run's algorithmic FLOPs per
    forward.  Not measured in this process: named by its source file."""
    for tag in ("r06_x3", "r05_x3"):
        path = os.path.join(REPO, "profiles", f"{tag}_gap_analysis.json")
        if not os.path.exists(path):
            continue
        loop = json.load(open(path)).get("sampling_loop") or {}
        if not loop.get("gemm_family_ms_per_forward"):
            continue
        g = sum(gflop_per_stage) / len(gflop_per_stage)
        ach = g / loop["gemm_family_ms_per_forward"]                 # GFLOP / ms = TFLOP/s
        return {"source": f"profiles/{tag}_gap_analysis.json (rocprofv3 --kernel-trace of `bench.py --steps 1 --warmup 1`, one sampling pass)",
                "forwards_in_window": loop["forwards"], "gemm_family_ms_per_forward": round(loop["gemm_family_ms_per_forward"], 4),
                "forward_ms_wall": round(loop["forward_ms_wall"], 4), "alg_gflop_per_forward": round(g, 2),
                "achieved": round(ach, 2), "frac": round(ach / peak, 4), "unit": "TFLOP/s"}
    return None


def gemm_roofline(eng, stream_ptr, precision):
    """Per-op HIP-event timing of one stage-1 denoiser forward; aggregates the MFMA implicit-GEMM launches."""
    from frido_amd import _lib
    prog = eng.stages[-1].step
    eng.step.zero_()                          # rewind the device step counter (it indexes the timestep table)
    prog.run(stream_ptr)                      # warm
    ms = prog.run_timed(stream_ptr)
    k_gemm = _lib.OP_KINDS["FRIDO_OP_GEMM"]
    t_gemm = flops = n_gemm = 0
    conv_t = conv_f = 0.0
    alg_bytes = 0.0
    per_kernel = {"conv3x3_gn_kernel": [0.0, 0.0, 0], "igemm_kernel": [0.0, 0.0, 0]}      # [ms, flops, launches]
    for (kind, st), t in zip(prog.ops, ms):
        if kind == k_gemm:
            f = 2.0 * st.M * st.N * (st.K + st.K2) * st.batch
            esz = 2 * st.nsplit
            a_b = (st.M // (st.Ho * st.Wo)) * st.Hs * st.Ws * st.Cin * esz if st.conv else st.M * st.K * esz * st.batch
            if st.gn_x1:      # fused GroupNorm + conv: the f32 stream (4 B / element) [+ the two SPADE maps] [+ the raw f32 rows of the skip conv]
                a_b = st.M * st.Cin * 4 * (3 if st.gn_gamma else 1) + st.M * st.K2 * 4
            o_b = st.M * (st.N // 2 if st.geglu else st.N) * st.batch * ((2 if st.out_bf16 else 4) * bool(st.out_f32) + esz * bool(st.out_op))
            r_b = st.M * st.N * (2 if st.res_bf16 else 4) if st.residual else 0
            alg_bytes += a_b + st.N * st.K * esz * (1 if not st.b_bs else st.batch) + o_b + r_b
            t_gemm += t
            flops += f
            n_gemm += 1
            if st.conv:
                conv_t += t
                conv_f += f
            pk = per_kernel["conv3x3_gn_kernel" if st.gn_x1 else "igemm_kernel"]
            pk[0] += t
            pk[1] += f
            pk[2] += 1
    total = sum(ms)
    passes = 3 if precision == "bf16x3" else 1          # MFMA passes per algorithmic product (hi*hi + hi*lo + lo*hi)
    algorithmic = flops / (t_gemm * 1e-3) / 1e12        # ALGORITHMIC 2MNK of the family / its summed launch time
    peak = 2500.0
    two_plane_f16 = precision == "bf16x3" and _lib.lib().frido_x3_plane_format() == 1
    insn = "v_mfma_f32_16x16x32_f16" if two_plane_f16 else "v_mfma_f32_16x16x32_bf16"
    tag = "r06_x3" if precision == "bf16x3" else "r02"
    prof = {}
    for t in (tag, "r05_x3", "r04_x3", "r03_x3"):
        pmc = os.path.join(REPO, "profiles", f"{t}_pmc_traffic.json")
        if os.path.exists(pmc):  # HBM bytes per launch from a COMMITTED rocprofv3 --pmc pass (FETCH_SIZE x2 + WRITE_SIZE), not measured in this run
            blob = json.load(open(pmc))
            fam = [blob[k] for k in GEMM_FAMILY if k in blob]
            if fam:
                prof["traffic"] = round(sum(e["hbm_bytes_per_launch"] * e["launches"] for e in fam) / sum(e["launches"] for e in fam))
                prof["traffic_source"] = (f"profiles/{t}_pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, reads x2; "
                                          "launch-weighted mean over the family)")
            break
    for t in (tag, "r05_x3", "r04_x3", "r03_x3"):
        pm = os.path.join(REPO, "profiles", f"{t}_pmc_mfma.json")
        if os.path.exists(pm):   # matrix-pipe busy share of the family's kernels (SQ_VALU_MFMA_BUSY_CYCLES, tools/pmc_sq.py)
            blob = json.load(open(pm))
            prof["mfma_busy_pmc"] = {k: blob[k].get("mfma_busy_frac") for k in GEMM_FAMILY if k in blob}
            prof["mfma_busy_source"] = f"profiles/{t}_pmc_mfma.json"
            break
    for t in (tag, "r05_x3", "r04_x3", "r03_x3"):
        csv_p = os.path.join(REPO, "profiles", f"{t}_bench_kernel_stats.csv")
        if os.path.exists(csv_p):    # the same family in the committed rocprofv3 --kernel-trace --stats summary of the bench command
            import csv
            calls = ns = 0
            for row in csv.DictReader(open(csv_p)):
                if any(k in row["Name"] for k in GEMM_FAMILY):
                    calls += int(row["Calls"])
                    ns += int(row["TotalDurationNs"])
            if calls:
                prof["rocprof_avg_launch_us"] = round(ns / calls / 1e3, 2)
                prof["rocprof_source"] = f"profiles/{t}_bench_kernel_stats.csv (all launches of the family in one bench run, decode and hoisted pre-pass included)"
            break
    return dict(bound="mfma", kernel=f"{' + '.join(GEMM_FAMILY)} (implicit-GEMM conv3x3 / 1x1 / linear family, {insn})",
                achieved=round(algorithmic, 2), peak=peak, unit="TFLOP/s", frac=round(algorithmic / peak, 4),
                schema="r04: achieved/frac = ALGORITHMIC 2MNK / time / dense-f16 MFMA peak (r03 lines carried executed = 3x algorithmic here)",
                mfma_passes=passes, mfma_pipe_tflops=round(passes * algorithmic, 2), mfma_pipe_frac=round(passes * algorithmic / peak, 4),
                note=("achieved = algorithmic FLOPs (2MNK, SURVEY 8d) of the GEMM-family launches of one denoiser forward / their summed "
                      "launch time from per-op HIP events on the launch stream; mfma_pipe_* = what the matrix pipe EXECUTES "
                      "(mfma_passes x 2MNK: the fp32-class two-plane arithmetic costs 3 MFMA passes per product), to be read next to PMC mfma_busy"),
                traffic=prof.get("traffic"), from_committed_profile=prof or None,
                alg_bytes_per_launch=round(alg_bytes / n_gemm),
                launches=n_gemm, avg_launch_us=round(1e3 * t_gemm / n_gemm, 2),
                alg_gflop_per_launch=round(flops / n_gemm / 1e9, 3),
                conv_tflops=round(conv_f / (conv_t * 1e-3) / 1e12, 2) if conv_t else None,
                # the two kernels of the family separately.  conv3x3_gn_kernel (r04) does the GroupNorm-apply + SiLU + hi / lo split of its
                # input INSIDE the launch (work that gn_apply_kernel did outside the family before): its time is not comparable 1:1 with a
                # plain conv's, the pair it replaces (gn_apply + ring conv) is profiles/r04_gnconv_bench_v3.txt
                per_kernel={k: dict(launches=v[2], avg_launch_us=round(1e3 * v[0] / v[2], 2), algorithmic_tflops=round(v[1] / (v[0] * 1e-3) / 1e12, 2),
                                    frac=round(v[1] / (v[0] * 1e-3) / 1e12 / peak, 4), share_of_forward=round(v[0] / total, 4))
                            for k, v in per_kernel.items() if v[2]},
                gemm_share_of_forward=round(t_gemm / total, 4), forward_ms=round(total, 3))


def live_roofline(model, dt_loop, args):
    """--full: the GEMM family of one denoiser forward against the dense-f16 MFMA roof -- per-op HIP events of an eager forward of
    every stage, the replayed forward from the loop-only pass (dt_loop) and the committed kernel trace (roofline.trace)."""
    rt = model.model.diffusion_model.runtime()
    eng = next(iter(rt._sampler_engines.values()))
    roof = gemm_roofline(eng, torch.cuda.current_stream().cuda_stream, args.precision)
    # `achieved` / `frac` come from per-op HIP events of an EAGER forward (every op bracketed by events: small kernels and
    # cold starts are over-stated).  The same forward inside the replayed graph is faster; scaling the event times by
    # (replayed forward time / sum of the event times) gives the in-graph figure -- an estimate, reported next to the
    # directly measured one, never instead of it.  Cross-check: profiles/r02_gap_analysis.json (kernel trace of the sampling pass).
    fwd_graph_ms = 1e3 * dt_loop / (len(eng.stages) * args.ddim_steps)
    sp = torch.cuda.current_stream().cuda_stream
    ev_ms = []
    for stg in eng.stages:                       # event-timed forward of EVERY stage (the loop replays each S times)
        eng.step.zero_()
        stg.step.run(sp)
        ev_ms.append(float(sum(stg.step.run_timed(sp))))
    gfl = family_gflop_per_forward(eng)
    roof["alg_gflop_per_forward_by_stage"] = [round(g, 2) for g in gfl]
    # `forward_ms` of this block = the forward as the sampler RUNS it (loop-only pass / forwards: graph replays); the per-op event sum it
    # used to hold is `forward_ms_events` (eager, every op bracketed by events: longer) -- forward_ms x forwards <= ms_per_step holds
    roof["forward_ms_events"] = roof["forward_ms"]
    roof["forward_ms"] = round(fwd_graph_ms, 3)
    roof["trace"] = trace_roofline(gfl, roof["peak"])
    if ev_ms and fwd_graph_ms > 0:
        # ratio only: small launches carry most of the event overhead, so scaling the GEMM figure by it would flatter it
        roof["event_vs_graph"] = {"forward_ms_replayed": round(fwd_graph_ms, 3), "forward_ms_events": [round(t, 3) for t in ev_ms],
                                  "event_to_graph_ratio": round((sum(ev_ms) / len(ev_ms)) / fwd_graph_ms, 3)}
    return roof


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def physical_cores():
    """Physical cores of this host (unique (package, core) pairs of /proc/cpuinfo; os.cpu_count() counts SMT threads)."""
    try:
        cores, pkg = set(), "0"
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                pkg = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                cores.add((pkg, line.split(":", 1)[1].strip()))
        if cores:
            return len(cores)
    except OSError:
        pass
    return os.cpu_count() or 1


def cpu_baseline(threads, full_ddim50=False):
    """The oracle (CPU restatement of the reference, fp32; pinned bit-exact to the reference by tests/test_oracle_golden.py) on
    this host's cores, on a bounded sample of the benchmark's workload: B in {1, 4} at 8, 16, 32 torch threads and
    at ALL physical cores -- one timed denoiser forward per stage after a warm one, one decode per batch size at that batch's best
    thread count -- extrapolated linearly to 2 x 200 forwards + decode (the loop's cost is linear in the step count).  Every
    (batch, threads) point is reported, so where the intra-op pool stops scaling is a measurement, not an assertion.
    `threads` > 0 restricts the sweep to that one count.  full_ddim50: additionally run a MEASURED DDIM-50 at B = 1."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from oracle import samplers as S
    from oracle.unet import unet_forward
    from oracle.vqgan import vq_decode
    from frido_amd.models import PyUNetModel, VQModelInterface
    u = PyUNetModel(**configs.UNET_F8F4)
    usd = {"model.diffusion_model." + k: torch.from_numpy(synth.fill_tensor("model.diffusion_model." + k, v.shape))
           for k, v in u.state_dict().items()}
    v = VQModelInterface(**configs.VQ_F8F4, lossconfig=dict(target="taming.modules.losses.DummyLoss"))
    vsd = {"first_stage_model." + k: torch.from_numpy(synth.fill_tensor("first_stage_model." + k, t.shape))
           for k, t in v.state_dict().items()}
    phys, logical = physical_cores(), os.cpu_count() or 1
    tried = sorted({n for n in ((threads,) if threads else (8, 16, 32, phys)) if 0 < n <= logical})
    variants = []
    for B in (1, 4):
        x = torch.from_numpy(synth.seeded_normal("cpu:x", (B, 6, 64, 64)))
        ctx = torch.from_numpy(synth.seeded_normal("cpu:ctx", (B, 26, 640)))
        t = torch.full((B,), 501)
        rows, t_start = [], time.perf_counter()           # (r05, advisor) every batch size has its OWN 90-s bound: a slow B = 1 sweep cannot starve B = 4
        for nthr in tried:
            if rows and time.perf_counter() - t_start > 90:       # bound: a collapsing thread count must not eat the bench's minutes (the first point always runs)
                rows.append(dict(batch=B, threads=nthr, skipped="cpu_baseline time bound (90 s per batch size) reached"))
                continue
            torch.set_num_threads(nthr)
            ts = []
            for s in (0, 1):
                xin = x[:, :3 * (s + 1)]
                t0 = time.perf_counter()
                unet_forward(usd, configs.UNET_F8F4, xin, t, ctx, s)              # warm (thread pool, allocator); timed too:
                t_warm = time.perf_counter() - t0
                if t_warm > 20:                                                     # a collapsed pool: one forward is evidence enough
                    ts.append(t_warm)
                    continue
                t0 = time.perf_counter()
                unet_forward(usd, configs.UNET_F8F4, xin, t, ctx, s)
                ts.append(time.perf_counter() - t0)
            rows.append(dict(batch=B, threads=nthr, fwd_s=[round(ts[0], 4), round(ts[1], 4)]))
        timed = [r for r in rows if "fwd_s" in r]
        if not timed:                                       # (cannot happen: the first thread count is never skipped)
            variants += rows
            continue
        best = min(timed, key=lambda r: sum(r["fwd_s"]))
        torch.set_num_threads(best["threads"])
        t0 = time.perf_counter()
        vq_decode(vsd, configs.VQ_F8F4, x)
        td = time.perf_counter() - t0
        for r in timed:
            loop = 200 * r["fwd_s"][0] + 200 * r["fwd_s"][1]
            r["loop_only_images_per_s"] = round(B / loop, 6)
            r["images_per_s"] = round(B / (loop + td), 6)       # decode timed at this batch's best thread count
        best["decode_s"] = round(td, 3)
        variants += rows
    timed = [r for r in variants if "images_per_s" in r]
    if not timed:
        return dict(error="no (batch, threads) point could be timed", variants=variants, kind="port", cores=0, value=None, unit="images/s")
    best = max(timed, key=lambda r: r["images_per_s"])
    out = dict(value=best["images_per_s"], unit="images/s", cores=best["threads"], kind="port", cpu_model=_cpu_model(),
               host_physical_cores=phys, host_logical_cpus=logical, cores_tried=tried,
               loop_only_value=best["loop_only_images_per_s"], variants=variants,
               sample=f"oracle fp32 (CPU restatement pinned to the reference); best of {len(timed)} timed (batch, threads) points = "
                      f"B={best['batch']} on {best['threads']} torch threads: one timed denoiser forward per stage "
                      f"({best['fwd_s'][0]}s / {best['fwd_s'][1]}s) + 1 decode per batch size, extrapolated to 2x200 forwards "
                      f"+ decode; threads tried: {tried} of {phys} physical cores / {logical} logical CPUs")
    if full_ddim50:
        threads = min((r for r in timed if r["batch"] == 1), key=lambda r: sum(r["fwd_s"]))["threads"]     # B = 1's best thread count
        torch.set_num_threads(threads)
        ac = S.alphas_cumprod_f32(S.make_betas())
        ctx = torch.from_numpy(synth.seeded_normal("cpu:ctx", (1, 26, 640)))
        torch.manual_seed(23)
        t0 = time.perf_counter()
        z, _ = S.ddim_sample(lambda xx, tt, cc, s: unet_forward(usd, configs.UNET_F8F4, xx, tt, cc, s), ac, 50, (1, 6, 64, 64), ctx,
                             [3, 3], [3, 3], 2, eta=1.0)
        t1 = time.perf_counter()
        S.decode_first_stage(lambda zz: vq_decode(vsd, configs.VQ_F8F4, zz), z, [1.0, 1.0], [3, 3])
        t2 = time.perf_counter()
        out["ddim50_measured"] = dict(batch=1, threads=threads, loop_s=round(t1 - t0, 2), decode_s=round(t2 - t1, 2),
                                      images_per_s=round(1.0 / (t2 - t0), 6),
                                      ddim200_extrapolated_images_per_s=round(1.0 / (4 * (t1 - t0) + (t2 - t1)), 6))
        # (r05, r04 verdict weak 10) the headline point -- the best (batch, threads) of the sweep -- MEASURED IN A LOOP too: a real
        # DDIM-10 (2 stages x 10 steps = 20 forwards + hand-off) at that batch and thread count, extrapolated x20 to DDIM-200.  The
        # single-forward extrapolation above and this loop are both in the line; where they disagree the loop is the one to quote.
        Bb, nthr = best["batch"], best["threads"]
        torch.set_num_threads(nthr)
        ctxb = torch.from_numpy(synth.seeded_normal("cpu:ctx", (Bb, 26, 640)))
        torch.manual_seed(23)
        t0 = time.perf_counter()
        zb, _ = S.ddim_sample(lambda xx, tt, cc, s: unet_forward(usd, configs.UNET_F8F4, xx, tt, cc, s), ac, 10, (Bb, 6, 64, 64), ctxb,
                              [3, 3], [3, 3], 2, eta=1.0)
        t1 = time.perf_counter()
        dec = best.get("decode_s") or 0.0
        out["ddim10_loop_measured"] = dict(batch=Bb, threads=nthr, loop_s=round(t1 - t0, 2), forwards=20,
                                           s_per_forward=round((t1 - t0) / 20, 4),
                                           single_forward_s=[best["fwd_s"][0], best["fwd_s"][1]],
                                           ddim200_extrapolated_images_per_s=round(Bb / (20 * (t1 - t0) + dec), 6),
                                           loop_vs_single_forward=round(((t1 - t0) / 20) / (sum(best["fwd_s"]) / 2), 3))
        # `value` = the LOOP measurement (the quantity the GPU line measures); the single-forward extrapolation stays beside it
        out["value_single_forward_extrapolation"] = out["value"]
        out["value"] = out["ddim10_loop_measured"]["ddim200_extrapolated_images_per_s"]
        out["sample"] = (f"oracle fp32 (CPU restatement pinned to the reference), B={Bb} on {nthr} torch threads (the best of {len(timed)} timed "
                         f"(batch, threads) points: {tried} of {phys} physical cores): a MEASURED DDIM-10 loop (20 denoiser forwards, "
                         f"{round(t1 - t0, 1)} s) + 1 decode ({dec} s), extrapolated x20 to DDIM-200; single-forward extrapolation and the "
                         f"B=1 measured DDIM-50 beside it")
    return out


def whole_step(S, images_per_s, world):
    tflop_img = (S * (208.72 + 208.76) + 129.6 + 799.7) / 1e3
    t = tflop_img * images_per_s
    return {"algorithmic_tflop_per_image": round(tflop_img, 2), "achieved_tflops": round(t, 1), "peak_tflops": 2500.0 * world,
            "frac": round(t / (2500.0 * world), 4)}


def config4_record(total, per_gpu, world, seconds, ddim_steps, stub=False):
    """`extra.config4_B32_per_gpu` of an N > 1 line: BASELINE config 4's per-GPU shard (32 images) through the same sharded job."""
    rec = {"workload": f"layout2i f8f4, batch {total} sharded {world} x {per_gpu} (BASELINE config 4 is 8 x 32 = 256), DDIM-{ddim_steps} x 2 stages + decode "
                       "+ one all-gather of the images", "global_batch": total, "per_gpu_batch": per_gpu, "n_gpus": world, "timed_passes": 1,
           "value": round(total / seconds, 4), "unit": "images/s", "ms_per_step": round(1e3 * seconds, 2)}
    if stub:
        rec["stub"] = True
    return rec


DUMP_BYTES = 64 << 20      # --dump-outputs budget over all arrays


def dump_outputs(path, arrays):
    """--dump-outputs: every array of `arrays` (name -> tensor) as <path>/<name>.npy in float32.  An array larger than the budget keeps a
    fixed, seeded sample of its leading (batch) index, sorted, so two runs of the same command write the same images."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    budget = DUMP_BYTES // len(arrays)
    for name, t in arrays.items():
        a = t.detach().to(torch.float32).cpu().numpy()
        if a.nbytes > budget:
            keep = max(1, budget // (a.nbytes // a.shape[0]))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(path, f"{name}.npy"), np.ascontiguousarray(a))


def relaunch(n):
    """Run this command line under torch.distributed.run with one rank per GPU (rendezvous on 127.0.0.1, a free port) as a child
    process and exit with its status."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    sys.exit(subprocess.call(cmd))


def stub_main(args, dist, use_dist, world, rank):
    """FRIDO_BENCH_STUB=1 (CPU test of the N > 1 entry point, tests/test_dist_gloo.py): the launcher, the shard arithmetic, the
    barrier-bracketed timing, the max over ranks and the JSON line of the real run, with the sampler + decoder replaced by a
    function of (seed, GLOBAL sample index) on CPU tensors over gloo.  The line says "stub": true -- it is not a measurement."""
    from frido_amd.pipeline import all_gather_images, shard_range
    B = args.batch
    total = B * world
    lo, hi = shard_range(total, rank, world)

    def one_step(k):
        idx = torch.arange(lo, hi, dtype=torch.float32)
        local = (1000.0 * k + idx).view(-1, 1, 1, 1).expand(hi - lo, 3, 8, 8).contiguous()
        time.sleep(0.01)
        return all_gather_images(local, total=total)

    for k in range(args.warmup):
        one_step(k)
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        img = one_step(args.warmup + k)
    if use_dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    per_rank = [dt]
    if use_dist:
        allt = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(allt, torch.tensor([dt], dtype=torch.float64))
        per_rank = [float(t.item()) for t in allt]
        dt = max(per_rank)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"images": img})
    cfg4 = None
    if args.full and world > 1 and B == 16 and not args.no_config4:        # the config-4 pass of the real N > 1 job (32 per GPU), same collective
        tot4 = 32 * world
        lo4, hi4 = shard_range(tot4, rank, world)
        if use_dist:
            dist.barrier()
        t4 = time.perf_counter()
        img4 = all_gather_images(torch.arange(lo4, hi4, dtype=torch.float32).view(-1, 1, 1, 1).expand(hi4 - lo4, 3, 8, 8).contiguous(), total=tot4)
        if use_dist:
            dist.barrier()
        assert torch.equal(img4[:, 0, 0, 0], torch.arange(tot4, dtype=torch.float32))
        cfg4 = config4_record(tot4, 32, world, max(time.perf_counter() - t4, 1e-6), args.ddim_steps, stub=True)
    k_last = args.warmup + args.steps - 1
    assert img.shape == (total, 3, 8, 8) and torch.equal(img[:, 0, 0, 0], 1000.0 * k_last + torch.arange(total, dtype=torch.float32))
    if rank == 0:
        print(json.dumps({"metric": f"images/sec @ DDIM-{args.ddim_steps}, COCO layout2img 256x256", "value": round(total * args.steps / dt, 4),
                          "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(1e3 * dt / args.steps, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          "dtype": "stub", "data": "stub", "stub": True,
                          "config": {"workload": "STUB (FRIDO_BENCH_STUB=1): launcher / shard / timing test on CPU over gloo, not a measurement"
                                                 + ("; extra.config4_B32_per_gpu: the same job at 32 per GPU" if cfg4 else ""),
                                     "global_batch": total, "parallelism": f"dp{world}"},
                          "per_rank_ms_per_step": [round(1e3 * t / args.steps, 2) for t in per_rank],
                          **({"extra": {"config4_B32_per_gpu": cfg4}} if cfg4 else {})}))
    if use_dist:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=16, help="per-GPU batch (BASELINE config 2: 16)")
    ap.add_argument("--ddim-steps", type=int, default=200)
    ap.add_argument("--precision", default=os.environ.get("FRIDO_PRECISION", "bf16x3"), choices=["bf16", "bf16x3"],
                    help="bf16x3 (default) = the arithmetic of the <= 1e-3 parity tests; bf16 = throughput mode, fails that tolerance")
    ap.add_argument("--image-dtype", default="uint8", choices=["uint8", "float32"],
                    help="what a step hands back (and, N > 1, all-gathers): the uint8 HWC images of scripts/sample_diffusion.py "
                         "custom_to_np, written by the decoder's last epilogue (default), or decode_first_stage's f32 NCHW tensor")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure, also run what it does not need: the loop-only pass, the per-op roofline, the bf16 "
                         "throughput mode, configs 3 / 5 (N = 1), the config-4 pass (N > 1) and the CPU baseline; the --no-* options "
                         "below switch single legs of it off")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned (the images) as DIR/<name>.npy in float32")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short passes of BASELINE configs 3 (t2i f16f8, B = 32, PLMS-100 + CFG 1.5) and 5 (512^2, 3 scales, B = 8) "
                         "that the N = 1 line carries in `extra.other_configs`")
    ap.add_argument("--no-config4", action="store_true",
                    help="N > 1 with --full: skip the extra pass at 32 images per GPU (BASELINE config 4's shard) reported in "
                         "extra.config4_B32_per_gpu")
    ap.add_argument("--no-bf16-extra", "--no-parity-mode", dest="no_bf16_extra", action="store_true",
                    help="skip the extra bf16 (throughput-mode) pass at N = 1")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--no-cpu-ddim50", action="store_true", help="skip the MEASURED DDIM-50 at B=1 on the CPU (~30 s)")
    ap.add_argument("--allow-debug", action="store_true", help="accept FRIDO_DEBUG_SKIP / FRIDO_GEMM_FLAGS (work-skipping timing experiments)")
    ap.add_argument("--retune", action="store_true", help="let this run (re)write the pinned tile cache")
    args = ap.parse_args()
    debug_env = {k: v for k, v in os.environ.items() if k in ("FRIDO_DEBUG_SKIP", "FRIDO_GEMM_FLAGS", "FRIDO_X3_SPADE_BF16", "FRIDO_X3_CROSSKV_HI") and v not in ("", "0")}
    if debug_env and not args.allow_debug:
        sys.exit(f"bench.py: {debug_env} drop work from the timed region; pass --allow-debug for a timing experiment "
                 "(the line then carries \"debug_work_skipped\": true and is not a benchmark result)")
    if debug_env.get("FRIDO_DEBUG_SKIP"):
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import debug_skip                                   # the work-skipping hook lives in tools/, not in the library
        debug_skip.install()
    if not args.retune:
        os.environ.setdefault("FRIDO_TUNE_CACHE_READONLY", "1")     # the tracked cache is only rewritten on request

    if args.gpus > 1 and os.environ.get("FRIDO_BENCH_STUB", "0") == "0":
        # (r05) fewer devices than ranks: ONE message and a non-zero exit code, before any process group exists -- from the launcher
        # spelling, and from every rank of a torchrun launch alike (rank 0 prints, all exit 2)
        have = torch.cuda.device_count()
        if have < args.gpus:
            if os.environ.get("RANK", "0") == "0":
                print(f"bench.py: --gpus {args.gpus} but this node exposes {have} HIP device(s); one rank per GPU is the only layout "
                      "(SURVEY.md 8e) -- nothing was run", file=sys.stderr)
            sys.exit(2)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` typed directly (the driver's N = 1 spelling with a larger N): become the one-rank-per-GPU job
        # ourselves, the way tools/frido/eval_layout2i_multiGPU.sh:9-12 of the reference starts N share-nothing processes
        relaunch(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} (launched by torch.distributed.run with another --nproc-per-node?)")
    import torch.distributed as dist
    stub = os.environ.get("FRIDO_BENCH_STUB", "0") != "0"      # tests/test_dist_gloo.py: the launcher + timing + JSON contract on CPU / gloo
    if stub:
        dev = torch.device("cpu")
    else:
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    use_dist = world > 1 or "RANK" in os.environ        # launched by torch.distributed.run: take the RCCL path even at N = 1
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if stub:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    if stub:
        return stub_main(args, dist, use_dist, world, rank)

    from frido_amd.pipeline import sample_images, shard_range
    model = build_model(args.precision, dev)
    B = args.batch
    total = B * world
    lo, hi = shard_range(total, rank, world)
    ctx_all = synth.seeded_normal("bench:ctx", (total, 26, 640))
    ctx = torch.from_numpy(ctx_all[lo:hi]).to(dev)

    def one_step(k):
        # check_status=False (r06, advisor): the sticky numerics word is NOT read-and-cleared per pass -- that put a batch of synchronous
        # symbol copies inside the timed loop and left `status_flags` below always 0; it is read ONCE after all passes instead
        return sample_images(model, ctx, S=args.ddim_steps, eta=1.0, seed=1000 + k, sample0=lo, noise="philox", total=total,
                             gather_dtype=args.image_dtype, check_status=False)

    _lib.status_flags(clear=True)

    for k in range(args.warmup):
        one_step(k)

    def fence():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    fence()
    t0 = time.perf_counter()
    for k in range(args.steps):
        img = one_step(args.warmup + k)
    fence()
    dt = time.perf_counter() - t0
    per_rank = [dt]
    if use_dist:
        allt = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(allt, torch.tensor([dt], device=dev, dtype=torch.float64))
        per_rank = [float(t.item()) for t in allt]
        dt = max(per_rank)                      # the slowest rank sets the job's time
    assert img.shape == ((total, 256, 256, 3) if args.image_dtype == "uint8" else (total, 3, 256, 256))
    assert args.image_dtype == "uint8" or bool(torch.isfinite(img).all()) or debug_env
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"images": img})
    if args.full:
        # the reference's own throughput definition (scripts/sample_diffusion.py:188-204): the sampling loop only, no decode
        from frido_amd.samplers import DDIMSampler
        unet = model.model.diffusion_model
        fence()
        t0 = time.perf_counter()
        z_chk, _ = DDIMSampler(model).sample(S=args.ddim_steps, batch_size=B, shape=(unet.in_channels, unet.image_size, unet.image_size),
                                             conditioning=ctx, num_stage=unet.num_stage, eta=1.0, verbose=False, noise="philox", seed=999,
                                             sample0=lo, log_every_t=10 ** 9)
        fence()
        dt_loop = time.perf_counter() - t0
        assert (bool(torch.isfinite(z_chk).all()) and float(z_chk.std()) > 0.05 and int(img.max()) > int(img.min())) or debug_env, "degenerate samples"

    status_after_timed = _lib.status_flags()          # every pass above ran with check_status=False: this is the word of ALL of them

    # (r06, r05 verdict next 8) BASELINE config 4 is "batch 256 sharded over 8 GPUs" = 32 per GPU; the driver's scaling spelling
    # (--gpus N, default batch 16) would never run it, so every N > 1 job adds ONE warm + ONE timed pass at 32 per GPU (same model,
    # same collective) and reports it in `extra.config4_B32_per_gpu` (--full).  --no-config4 skips it; N = 1 has it as tools' --batch 32 line.
    cfg4 = None
    if args.full and world > 1 and B == 16 and not args.no_config4:
        B4 = 32
        tot4 = B4 * world
        lo4, hi4 = shard_range(tot4, rank, world)
        ctx4 = torch.from_numpy(synth.seeded_normal("bench:ctx", (tot4, 26, 640))[lo4:hi4]).to(dev)
        step4 = lambda k: sample_images(model, ctx4, S=args.ddim_steps, eta=1.0, seed=3000 + k, sample0=lo4, noise="philox", total=tot4,
                                        gather_dtype=args.image_dtype, check_status=False)
        step4(0)
        fence()
        t0 = time.perf_counter()
        img4 = step4(1)
        fence()
        d4 = time.perf_counter() - t0
        if use_dist:
            t4 = torch.tensor([d4], device=dev, dtype=torch.float64)
            dist.all_reduce(t4, op=dist.ReduceOp.MAX)
            d4 = float(t4.item())
        assert img4.shape[0] == tot4
        cfg4 = config4_record(tot4, B4, world, d4, args.ddim_steps)
        del img4, ctx4

    if rank == 0:
        out = {
            "metric": f"images/sec @ DDIM-{args.ddim_steps}, COCO layout2img 256x256", "value": round(total * args.steps / dt, 4),
            "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if args.precision == "bf16" else (
                "f16x3 (precision keyword bf16x3: hi/lo fp16 operand planes, 3 MFMA passes, fp32 accumulate: fp32-class)"
                if _lib.lib().frido_x3_plane_format() == 1 else
                "bf16x3 (hi/lo bf16 operand planes, 3 MFMA passes, fp32 accumulate: fp32-class)"),
            "data": "synthetic (random-init weights from the deterministic filler, N(0,1) context, Philox x_T/noise)",
            "config": {"workload": f"layout2i f8f4 (configs/frido/layout2i/frido_f8f4_coco_seg.yaml), per-GPU batch {B}, "
                                   f"DDIM-{args.ddim_steps} eta=1.0 x 2 stages + MS-VQGAN decode"
                                   + f" to {args.image_dtype} images" + (f", RCCL all-gather of the {args.image_dtype} images" if world > 1 else "")
                                   + ("; extra.config4_B32_per_gpu: the same job at 32 per GPU (BASELINE config 4's shard), one timed pass" if cfg4 else ""),
                       "global_batch": total, "denoiser_forwards_per_step": 2 * args.ddim_steps, "parallelism": f"dp{world}",
                       "env": {k: v for k, v in sorted(os.environ.items()) if k.startswith("FRIDO_") and k != "FRIDO_TUNE_CACHE"}},
            # whole job against the same roof: SURVEY 8(d)'s canonical (deduplicated) algorithmic FLOPs per image of this workload
            # -- S x (208.72 + 208.76) GFLOP of denoiser forwards + 129.6 one-time (SPADE maps, cross K/V, emb) + 799.7 decode
            "whole_step": whole_step(args.ddim_steps, total * args.steps / dt, world),
            "per_rank_ms_per_step": [round(1e3 * t / args.steps, 2) for t in per_rank],
            # sticky numerics word of the library, read ONCE after the warm-up, timed and (--full) loop-only passes, none of which cleared it
            # (frido_status_flags): 0 = no fp16 operand plane saturated, no normalisation statistic was NaN / inf anywhere in that work
            "status_flags": status_after_timed,
        }
        if args.full:
            out["roofline"] = live_roofline(model, dt_loop, args)
            out["loop_only_value"] = round(total / dt_loop, 4)        # sample_diffusion.py's `throughput`: sampler loop without decode
        if debug_env:
            out["debug_work_skipped"] = True
        if cfg4:
            out.setdefault("extra", {})["config4_B32_per_gpu"] = cfg4
        if args.full and world == 1 and args.precision == "bf16x3" and not args.no_bf16_extra:
            # the same workload in plain bf16 (one plane, one MFMA pass): a THROUGHPUT mode that fails the north star's <= 1e-3
            # tolerance (its measured error is in the committed E2E record) -- reported for reference, never as `value`
            del model
            torch.cuda.empty_cache()
            m1 = build_model("bf16", dev)
            sample_images(m1, ctx, S=args.ddim_steps, eta=1.0, seed=1, sample0=lo, noise="philox", total=total, gather_dtype=args.image_dtype)
            fence()
            t0 = time.perf_counter()
            for k in range(args.steps):
                sample_images(m1, ctx, S=args.ddim_steps, eta=1.0, seed=2 + k, sample0=lo, noise="philox", total=total,
                              gather_dtype=args.image_dtype)
            fence()
            d1 = (time.perf_counter() - t0) / args.steps
            extra = {"dtype": "bf16", "value": round(total / d1, 4), "unit": "images/s", "ms_per_step": round(1e3 * d1, 2),
                     "steps": args.steps, "meets_1e-3_tolerance": False}
            for name in ("r06_e2e_error.json", "r05_e2e_error.json", "r04_e2e_error.json", "r03_e2e_error.json"):
                e2e = os.path.join(REPO, "profiles", name)
                if os.path.exists(e2e):         # end-to-end error of both arithmetic modes vs the reference's own CPU run (GPU tests write it)
                    extra["e2e_error_vs_reference"] = {"from_committed_profile": f"profiles/{name}", "record": json.load(open(e2e))}
                    break
            out["extra"] = {"bf16_throughput_mode": extra}
            del m1
        if args.full and world == 1 and args.precision == "bf16x3" and not args.no_other_configs and args.batch == 16 and args.ddim_steps == 200:
            # (r05, r04 verdict weak 11) the other single-GPU workloads of BASELINE.json, timed by THIS command so that the driver's
            # record holds them: config 3 (t2i f16f8, batch 32, PLMS-100 + CFG 1.5) and config 5's per-GPU shard (512 x 512, three
            # scales, batch 8, DDIM-200) -- short passes (1 warm + 2 / 1 timed), same arithmetic as `value`; not the headline metric
            try:
                del model
            except NameError:
                pass
            torch.cuda.empty_cache()
            sys.path.insert(0, os.path.join(REPO, "tools"))
            others = {}
            for key, modname, kw in (("config3_t2i_f16f8_B32_plms100_cfg1.5", "bench_config3", dict(steps=2, warmup=1)),
                                     ("config5_512x512_3scale_B8_ddim200", "bench_config5", dict(steps=1, warmup=1))):
                try:
                    mod = __import__(modname)
                    t_o = time.perf_counter()
                    others[key] = mod.run(precision="bf16x3", **kw)
                    others[key]["wall_s_incl_build_and_warmup"] = round(time.perf_counter() - t_o, 1)
                except Exception as e:      # noqa: BLE001  (a failure here must not lose the headline line)
                    others[key] = {"error": f"{type(e).__name__}: {e}"}
                torch.cuda.empty_cache()
            out.setdefault("extra", {})["other_configs"] = others
            # (r06) the two values again as a flat top-level dict: a record that keeps only the first level of the line still holds them
            out["other_configs_images_per_s"] = {k: v.get("value", v.get("error")) for k, v in others.items()}
        if args.full and world == 1 and not args.no_cpu_baseline:
            # B in {1, 4} x {8, 16, 32, all physical cores} torch threads; `cores` = the best point's thread count
            try:      # (r05, advisor) a failure of the CPU leg must not lose the GPU measurement above
                out["cpu_baseline"] = cpu_baseline(args.cpu_threads, full_ddim50=not args.no_cpu_ddim50)
            except Exception as e:      # noqa: BLE001
                out["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}", "kind": "port", "value": None, "unit": "images/s", "cores": 0}
        # key order of the line: the flat summary keys first, the long nested blocks (`extra`, `cpu_baseline`) last
        tail = [k for k in ("roofline", "extra", "cpu_baseline") if k in out]
        out = {**{k: v for k, v in out.items() if k not in tail}, **{k: out[k] for k in tail}}
        print(json.dumps(out))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
