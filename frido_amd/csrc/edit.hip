// The editing blend of the DDIM loop (img2img start and keep-mask inpainting) on the NHWC f32 latent state: FridoKeepBlend in
// include/frido_hip.h.  On a channel window [c0, c1) of x[B][HW][Cx]
//   q  = sa * z0 + sb * n          (frido/models/diffusion/frido.py:306-307, this order)
//   x' = q * m + (1 - m) * x       (frido/models/diffusion/ddim.py:161, this order)
// in plain f32, every product and sum rounded on its own (no FMA contraction, like the ancestral kernel in misc.hip), so the two builds
// of the library compile the same kernel; common.h is included for the sticky status word only (a non-finite x' raises
// FRIDO_STATUS_NONFINITE).  Channels outside the window are never read or written.
// Bandwidth-bound and tiny next to a denoiser forward: its job is to keep the blend inside the captured step body.  One thread owns one
// Philox group -- up to 4 consecutive window channels of one pixel -- and reads scalars: the normal window, 3 channels at offset 3 of 6,
// is never 16-byte aligned, so a vector path would serve no shipped shape.
#include "common.h"

namespace {

#include "philox.h"      // the generator of frido_randn and the sampler updates (misc.hip includes the same file)

constexpr int EDIT_GRID_CAP = 2048;

// Unit i = (pixel i / ngrp of the batch, group i % ngrp of its window): window channels [4 g, min(4 g + 4, c1 - c0)).
__global__ __launch_bounds__(256) void keep_blend_kernel(const FridoKeepBlend d, int ngrp, int64_t units) {
    const int step = d.step ? *d.step : 0;
    const int row = step + d.row_offset;
    const float sa = d.clean ? 1.0f : d.qtab[2 * (int64_t)row], sb = d.clean ? 0.0f : d.qtab[2 * (int64_t)row + 1];
    const uint64_t seed = d.rng_dev ? (uint64_t)d.rng_dev[0] : d.seed;
    const int64_t sample0 = d.rng_dev ? d.rng_dev[1] : d.sample0;
    const int wn = d.c1 - d.c0;
    const float* tape = d.noise ? d.noise + (int64_t)step * d.noise_stride : nullptr;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int g = (int)(i % ngrp);
        const int64_t pix = i / ngrp;                    // (b, p)
        const float m = d.mask ? d.mask[pix] : 1.0f;
        const int j0 = g * 4, nj = wn - j0 < 4 ? wn - j0 : 4;
        float n[4] = {0.f, 0.f, 0.f, 0.f};
        if (!d.clean) {
            if (tape) {
                for (int k = 0; k < nj; ++k) n[k] = tape[pix * d.noise_C + d.c0 + j0 + k];
            } else {
                const int64_t b = pix / d.HW, p = pix - b * d.HW;
                randn4(seed, sample0 + b, (uint32_t)row + 1u, (uint32_t)d.rng_stream, (uint32_t)(p * ngrp + g), n);
            }
        }
        const int64_t xi = pix * d.Cx + d.c0 + j0;
        for (int k = 0; k < nj; ++k) {
            const float z = d.z0[xi + k];
            const float q = d.clean ? z : __fadd_rn(__fmul_rn(sa, z), __fmul_rn(sb, n[k]));
            const float o = d.mask ? __fadd_rn(__fmul_rn(q, m), __fmul_rn(__fsub_rn(1.0f, m), d.x[xi + k])) : q;
            bad |= nonfinite(o);
            d.x[xi + k] = o;
        }
    }
    status_raise(false, bad);
}

}  // namespace

extern "C" int frido_keep_blend(const FridoKeepBlend* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->x && d->z0, "null pointer");
    FRIDO_REQUIRE(d->clean == 0 || d->clean == 1, "clean is 0 or 1");
    FRIDO_REQUIRE(d->clean || d->qtab, "null pointer: the coefficient table (only clean = 1 does without)");
    FRIDO_REQUIRE(d->B > 0 && d->HW > 0 && d->Cx > 0, "B, HW and Cx must be positive");
    FRIDO_REQUIRE(d->c0 >= 0 && d->c0 < d->c1 && d->c1 <= d->Cx, "the channel window must be non-empty and lie inside [0, Cx]");
    FRIDO_REQUIRE(d->row_offset >= 0, "row_offset must not be negative");
    FRIDO_REQUIRE(!(d->noise && (d->rng_dev || d->seed || d->sample0 || d->rng_stream)), "a noise tape together with a Philox key: one noise form per launch");
    FRIDO_REQUIRE(!d->noise || (d->noise_C >= d->c1 && d->noise_stride >= 0), "the noise tape holds the channels reached so far: noise_C >= c1, noise_stride >= 0");
    FRIDO_REQUIRE(!(d->clean && (d->noise || d->rng_dev)), "clean = 1 reads no noise: pass neither a tape nor rng_dev");
    const int ngrp = (d->c1 - d->c0 + 3) >> 2;
    FRIDO_REQUIRE((int64_t)d->HW * ngrp < ((int64_t)1 << 32), "a sample has more Philox groups than the 32-bit group counter holds");
    const int64_t units = (int64_t)d->B * d->HW * ngrp;
    hipLaunchKernelGGL(keep_blend_kernel, dim3(grid_for(units, EDIT_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, ngrp, units);
    return frido_check_launch("keep_blend");
}
