"""Times FrozenClipImageEmbedder on the MI355X: milliseconds per batch at the ViT-B/32 and ViT-L/14 geometries, the split between the
preprocess kernel and the tower's program, the launch count, and -- when `transformers` imports -- the same tower in torch fp32 eager
beside it.  Weights are the deterministic filler's (no trained CLIP ships here): times do not depend on them.

    python tools/clip_image_bench.py [--batch 16] [--size 256] [--reps 30] [--versions ViT-B/32 ViT-L/14] > profiles/clip_image.txt

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


def hf_tower(arch):
    """transformers' CLIPVisionModelWithProjection of the same geometry (random weights, fp32, eager), or the reason there is none."""
    try:
        os.environ.setdefault("HF_HUB_OFFLINE", "1")
        import transformers
    except Exception as e:      # noqa: BLE001
        return None, f"transformers does not import here ({type(e).__name__}: {e})"
    embed, res, layers, width, patch = arch
    cfg = transformers.CLIPVisionConfig(hidden_size=width, intermediate_size=4 * width, num_hidden_layers=layers,
                                        num_attention_heads=width // 64, image_size=res, patch_size=patch, projection_dim=embed,
                                        hidden_act="quick_gelu", layer_norm_eps=1e-5)
    return transformers.CLIPVisionModelWithProjection(cfg).float().eval().cuda(), f"transformers {transformers.__version__}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--versions", nargs="+", default=["ViT-B/32", "ViT-L/14"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/clip_image_bench.py: no HIP device; nothing was measured")
    from frido_amd import holders, tune, vision
    from frido_amd.engine import current_stream_ptr
    from frido_amd.models import FrozenClipImageEmbedder
    from frido_amd.synth import fill_module

    B, S = args.batch, args.size
    print(f"# FrozenClipImageEmbedder on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; batch {B}, inputs {S} x {S}, "
          f"precision bf16x3 (fp16-pair planes), median of {args.reps} event-timed calls after 3 warm ones")
    print(f"# GEMM tiles: {'the pinned cache' if tune.cache_is_pinned_for_this_library() else 'tuned live at plan time (no pinned cache for this build)'}")
    x = torch.rand(B, 3, S, S, device="cuda") * 2 - 1
    mean = torch.tensor(vision.CLIP_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(vision.CLIP_STD, device="cuda").view(1, 3, 1, 1)
    for version in args.versions:
        arch = holders.CLIP_VISUAL_ARCH[version]
        t0 = time.perf_counter()
        m = fill_module(FrozenClipImageEmbedder(version), "clip_image.").cuda()
        m(x)
        torch.cuda.synchronize()
        plan = next(iter(m._plans.values()))[0]
        print(f"\n## {version}: embed_dim {arch[0]}, {arch[1]}^2 pixels, {arch[2]} layers, width {arch[3]}, patch {arch[4]} -> {plan.n} tokens "
              f"(first call, with filling the weights, planning and the capture: {time.perf_counter() - t0:.1f} s)")
        print(f"launches per call: 1 preprocess + {len(plan.prog.ops)} program ops, replayed as one graph")
        sp = current_stream_ptr(x.device)
        print(f"forward(x), as a user calls it (copy in, graph, copy out): {fmt(timed(lambda: m(x), args.reps))}")
        print(f"  graph replay alone:                                      {fmt(timed(lambda: plan.graph.launch(sp), args.reps))}")
        print(f"  preprocess kernel alone (frido_clip_preprocess):         {fmt(timed(lambda: vision.clip_preprocess(plan.pre, sp), args.reps))}")
        print(f"  tower program alone, launched op by op (no graph):       {fmt(timed(lambda: plan.prog.run(sp), args.reps))}")
        hf, why = hf_tower(arch)
        if hf is None:
            print(f"torch fp32 eager: not measured -- {why}")
        else:
            def eager():
                v = F.interpolate(x, (arch[1], arch[1]), mode="bicubic", align_corners=True)
                with torch.no_grad():
                    return hf(pixel_values=((v + 1.0) / 2.0 - mean) / std).image_embeds
            print(f"torch fp32 eager ({why}; F.interpolate + CLIPVisionModelWithProjection, random weights): {fmt(timed(eager, args.reps))}")
            del hf
        del m, plan
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
