// DDIM inversion update (DDIM's deterministic encoder: the probability-flow ODE walked upwards, upstream latent-diffusion's
// DDIMSampler.encode; not in the reference) on the NHWC f32 latent state: FridoInvertStep in include/frido_hip.h.  On the stage's channel
// window [c_lo, c_hi) of x[B][HW][Cx], with {c0, c1} = coef[*step + coef_row_offset] (frido_amd/schedules.py ddim_inversion_table)
//   e  = eps_cond, or under guidance  e_u + s * (e_c - e_u),  s = *cfg_dev if cfg_dev else cfg_scale
//        -- guided_eps (launch.h): the DDIM / PLMS and DPM-Solver updates' expression
//   x' = c0 * x + c1 * e
// in plain f32, every product and sum rounded on its own (no FMA contraction), so the two builds of the library compile the same kernel;
// common.h is included for the sticky status word only (a non-finite x' raises FRIDO_STATUS_NONFINITE).  Channels outside the window are
// never read or written.  Bandwidth-bound and tiny next to a denoiser forward: its job is to keep the update inside the captured step
// body.  One thread owns one element and reads scalars: the normal window, 3 channels at offset 0 or 3 of 6, is never 16-byte aligned, so
// a vector path would serve no shipped shape.
#include "common.h"

namespace {

constexpr int INVERT_ROW = 2;       // c0, c1
constexpr int INVERT_GRID_CAP = 2048;

// Unit i = (pixel i / wn of the batch, window channel i % wn); eps is [B * HW][wn], so unit i reads eps[i].
__global__ __launch_bounds__(256) void ddim_invert_step_kernel(const FridoInvertStep d, int64_t units) {
    const int step = d.step ? *d.step : 0;
    const float* cf = d.coef + (int64_t)(step + d.coef_row_offset) * INVERT_ROW;
    const float c0 = cf[0], c1 = cf[1];
    const float cfg = d.cfg_dev ? *d.cfg_dev : d.cfg_scale;
    const int wn = d.c_hi - d.c_lo;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = i / wn;
        const int64_t xi = pix * d.Cx + d.c_lo + (i - pix * wn);
        float e = d.eps_cond[i];
        if (d.eps_uncond) {
            const float eu = d.eps_uncond[i];
            e = guided_eps(e, eu, cfg);
        }
        const float o = __fadd_rn(__fmul_rn(c0, d.x[xi]), __fmul_rn(c1, e));
        bad |= nonfinite(o);
        d.x[xi] = o;
    }
    status_raise(false, bad);
}

}  // namespace

extern "C" int frido_invert_step(const FridoInvertStep* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->x && d->eps_cond && d->coef, "null pointer");
    FRIDO_REQUIRE(d->B > 0 && d->HW > 0 && d->Cx > 0, "B, HW and Cx must be positive");
    FRIDO_REQUIRE(d->c_lo >= 0 && d->c_lo < d->c_hi && d->c_hi <= d->Cx, "the channel window must be non-empty and lie inside [0, Cx]");
    FRIDO_REQUIRE(d->coef_row_offset >= 0, "coef_row_offset must not be negative");
    FRIDO_REQUIRE(d->cfg_scale == d->cfg_scale, "cfg_scale is NaN");
    const int64_t units = (int64_t)d->B * d->HW * (d->c_hi - d->c_lo);
    hipLaunchKernelGGL(ddim_invert_step_kernel, dim3(grid_for(units, INVERT_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, units);
    return frido_check_launch("invert_step");
}
