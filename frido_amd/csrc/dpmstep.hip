// DPM-Solver++(2M) state update (Lu et al. 2022: data prediction, multistep, order 1 / 2) on the NHWC f32 latent state: FridoDpmStep in
// include/frido_hip.h.  Plain f32 arithmetic, every product and sum rounded on its own, so the two builds of the library compile the
// same kernel; common.h is included for the sticky status word only (a non-finite x' raises FRIDO_STATUS_NONFINITE).  Bandwidth-bound: per
// active element it reads x, eps (twice under guidance) and -- on a second-order row -- the previous x0, and writes x', x0 and the history.
#include "common.h"

namespace {

constexpr int DPM_ROW = 8;      // inv_alpha, sigma, c_x, c_d, w_cur, w_last, pad x2 (frido_amd/schedules.py dpm_solver_rows)
constexpr int DPM_GRID_CAP = 2048;

// One unit = V consecutive channels of one pixel among channels [0, start + nch).  V == 4: Cx, start and nch are multiples of 4, so a unit
// is frozen or active as a whole and one 16-byte access on every tensor.  V == 1: any channel counts.  Channels from start + nch on are
// left alone in x_out and pred_x0, like sampler_step_kernel leaves them.
template <int V>
__global__ __launch_bounds__(256) void dpm_step_kernel(const FridoDpmStep d, int64_t units) {
    const int end = d.start + d.nch;
    const int cv = end / V;
    const int step = d.step ? *d.step : 0;
    const float* cf = d.coef + (int64_t)(step + d.coef_row_offset) * DPM_ROW;
    const float inv_alpha = cf[0], sigma = cf[1], c_x = cf[2], c_d = cf[3], w_cur = cf[4], w_last = cf[5];
    const bool second = w_last != 0.0f;      // a first-order row never reads the history: a stage's first step finds it stale
    const float cfg = d.cfg_dev ? *d.cfg_dev : d.cfg_scale;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % cv) * V;
        const int64_t pix = i / cv;
        const int64_t xi = pix * d.Cx + c;
        float xv[V];
        load_vec<V>(d.x + xi, xv);
        if (c < d.start) {      // frozen channels: x0 = x, x' = x
            if (d.x_out != d.x) store_vec<V>(d.x_out + xi, xv);
            if (d.pred_x0) store_vec<V>(d.pred_x0 + xi, xv);
            continue;
        }
        const int64_t ei = pix * d.nch + (c - d.start);
        float e[V], eu[V], h[V], x0[V], xo[V];
        load_vec<V>(d.eps_cond + ei, e);
        if (d.eps_uncond) load_vec<V>(d.eps_uncond + ei, eu);
        if (second) load_vec<V>(d.x0_hist + ei, h);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float ev = e[k];
            if (d.eps_uncond) ev = guided_eps(ev, eu[k], cfg);
            x0[k] = __fmul_rn(__fsub_rn(xv[k], __fmul_rn(sigma, ev)), inv_alpha);
            const float D = second ? __fadd_rn(__fmul_rn(w_cur, x0[k]), __fmul_rn(w_last, h[k])) : x0[k];
            xo[k] = __fadd_rn(__fmul_rn(c_x, xv[k]), __fmul_rn(c_d, D));
            bad |= nonfinite(xo[k]);
        }
        store_vec<V>(d.x_out + xi, xo);
        if (d.pred_x0) store_vec<V>(d.pred_x0 + xi, x0);
        store_vec<V>(d.x0_hist + ei, x0);
    }
    status_raise(false, bad);
}

}  // namespace

extern "C" int frido_dpm_step(const FridoDpmStep* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->x && d->eps_cond && d->coef && d->x_out && d->x0_hist, "null pointer");
    FRIDO_REQUIRE(d->B > 0 && d->HW > 0 && d->Cx > 0 && d->nch > 0, "B, HW, Cx and nch must be positive");
    FRIDO_REQUIRE(d->start >= 0 && (int64_t)d->start + d->nch <= d->Cx, "the channel range must lie inside [0, Cx]");
    FRIDO_REQUIRE(d->cfg_scale == d->cfg_scale, "cfg_scale is NaN");
    const int end = d->start + d->nch;
    const bool vec = d->Cx % 4 == 0 && d->start % 4 == 0 && d->nch % 4 == 0 && aligned16(d->x) && aligned16(d->x_out) && aligned16(d->pred_x0) &&
                     aligned16(d->eps_cond) && aligned16(d->eps_uncond) && aligned16(d->x0_hist);
    const int64_t n = (int64_t)d->B * d->HW * end;
    if (vec)
        hipLaunchKernelGGL(dpm_step_kernel<4>, dim3(grid_for(n / 4, DPM_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, n / 4);
    else
        hipLaunchKernelGGL(dpm_step_kernel<1>, dim3(grid_for(n, DPM_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, n);
    return frido_check_launch("dpm_step");
}
