// The diffusion objective of FridoDiffusion (frido/models/diffusion/frido.py): q_sample as p_losses calls it (:302-318, 1184) and the
// loss of one stage (:1196-1222).  Plain f32 / f64 arithmetic: no operand planes, so no status word (launch.h alone: common.h is not included on purpose
// -- it would register one) and the two builds of the library compile the same code.  Both kernels are bandwidth-bound.
// Noise is a tape [B][HW][Cx] or Philox4x32-10 in frido_randn's numbering (misc.hip: 4-float groups over the flat sample [HW][Cx],
// draw 0, key (seed, sample0 + b, rng_stream)); the loss kernel regenerates its target from the same key, so no noise tensor exists
// in Philox mode.
#include "launch.h"

namespace {

constexpr int LOSS_GRID_CAP = 8192;

#include "philox.h"      // the generator of frido_randn (misc.hip includes the same file)

__device__ __forceinline__ int table_row(const int64_t* t, int64_t b, int T) {      // a timestep outside the tables must not read outside them
    const int64_t v = t[b];
    return (int)(v < 0 ? 0 : (v >= T ? T - 1 : v));
}

// ---- q_sample ----------------------------------------------------------------------------------------------------------------------
// The noise of elements [e, e + V) of sample `sample`'s flat [HW][Cx]: from the tape, else the Philox group that holds them (V == 4: e is a
// multiple of 4, the unit is exactly one group; V == 1: the group is drawn whole and one lane of it used).
template <int V>
__device__ __forceinline__ void noise_vec(const float* tape, uint64_t seed, int64_t sample, uint32_t stream, int64_t e, float n[V]) {
    if (tape) {
        load_vec<V>(tape + e, n);
        return;
    }
    float r[4];
    randn4(seed, sample, 0u, stream, (uint32_t)(e >> 2), r);
    if constexpr (V == 4) {
        n[0] = r[0]; n[1] = r[1]; n[2] = r[2]; n[3] = r[3];
    } else {
        n[0] = r[e & 3];
    }
}

// One unit = V consecutive channels of one pixel, channels [0, ch_end).  V == 4: Cx and ch_end are multiples of 4, so a unit is one
// 16-byte access on every tensor.  V == 1: any channel counts.  A unit of coarse channels only is a copy when mix == 0: no noise is
// loaded or drawn for it.
template <int V>
__global__ __launch_bounds__(256) void qsample_kernel(const FridoQSample d, float keep, float mix, int64_t units) {
    const int cv = d.ch_end / V;
    const uint64_t seed = d.rng_dev ? (uint64_t)d.rng_dev[0] : d.seed;
    const int64_t sample0 = d.rng_dev ? d.rng_dev[1] : d.sample0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % cv) * V;
        const int64_t pix = i / cv;                      // (b, p)
        const int64_t b = pix / d.HW, p = pix - b * d.HW;
        const int row = table_row(d.t, b, d.T);
        const float a = d.sqrt_ac[row], s = d.sqrt_1mac[row];
        const int64_t e = p * d.Cx + c;                  // index within the flat sample [HW][Cx]
        float x[V], n[V], o[V];
        load_vec<V>(d.x0 + pix * d.Cx + c, x);
        const bool copy = mix == 0.0f && c + V <= d.ch_start;
        if (!copy) noise_vec<V>(d.noise ? d.noise + b * d.HW * d.Cx : nullptr, seed, sample0 + b, (uint32_t)d.rng_stream, e, n);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (c + k >= d.ch_start) o[k] = __fadd_rn(__fmul_rn(a, x[k]), __fmul_rn(s, n[k]));
            else if (mix != 0.0f) o[k] = __fadd_rn(__fmul_rn(keep, x[k]), __fmul_rn(mix, n[k]));
            else o[k] = x[k];
        }
        float* dst = d.x_noisy + pix * d.ch_end + c;
        if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        else *dst = o[0];
    }
}

// ---- loss --------------------------------------------------------------------------------------------------------------------------
// One workgroup per sample: thread j owns units j, j + 256, ... of the sample's HW * nch elements (a unit = V consecutive channels of
// one pixel) and adds their fp32 element losses into an f64 partial in that order; the 256 partials are added pairwise through LDS.
// Nothing depends on B or on the sample's position in the batch, and there is no atomic: the same bits on every launch.
template <int V>
__global__ __launch_bounds__(256) void loss_sample_kernel(const FridoDiffusionLoss d) {
    __shared__ double part[256];
    const int64_t b = blockIdx.x;
    const int cv = d.nch / V;
    const int64_t units = (int64_t)d.HW * cv;
    const uint64_t seed = d.rng_dev ? (uint64_t)d.rng_dev[0] : d.seed;
    const int64_t sample0 = d.rng_dev ? d.rng_dev[1] : d.sample0;
    const float* pred = d.pred + b * d.HW * d.nch;
    const float* noise = d.noise ? d.noise + b * d.HW * d.Cx : nullptr;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < units; i += 256) {
        const int c = (int)(i % cv) * V;
        const int64_t p = i / cv;
        const int64_t e = p * d.Cx + d.ch_start + c;     // the target's index within the flat sample [HW][Cx]
        float pr[V], tg[V];
        load_vec<V>(pred + p * d.nch + c, pr);
        noise_vec<V>(noise, seed, sample0 + b, (uint32_t)d.rng_stream, e, tg);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float df = __fsub_rn(tg[k], pr[k]);
            acc += (double)(d.loss_type == 0 ? fabsf(df) : __fmul_rn(df, df));
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) d.per_sample[b] = (float)(part[0] / (double)((int64_t)d.HW * d.nch));
}

// The stage row from the stored per-sample means (p_losses reads loss_simple as the f32 tensor it is): lane j adds samples j, j + 64, ...
// in f64, lane 0 adds the 64 partials in order.
__global__ __launch_bounds__(64) void loss_row_kernel(const FridoDiffusionLoss d) {
    __shared__ double part[3][64];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int b = threadIdx.x; b < d.B; b += 64) {
        const int row = table_row(d.t, b, d.T);
        const double ls = (double)d.per_sample[b], lv = (double)d.logvar[row];
        s0 += ls;
        s1 += ls / exp(lv) + lv;
        s2 += (double)d.lvlb_weights[row] * ls;
    }
    part[0][threadIdx.x] = s0; part[1][threadIdx.x] = s1; part[2][threadIdx.x] = s2;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[3] = {0.0, 0.0, 0.0};
        for (int j = 0; j < 64; ++j) { r[0] += part[0][j]; r[1] += part[1][j]; r[2] += part[2][j]; }
        const double simple = r[0] / d.B, gamma = r[1] / d.B, vlb = r[2] / d.B;
        d.out[0] = (float)simple;
        d.out[1] = (float)gamma;
        d.out[2] = (float)vlb;
        d.out[3] = (float)((double)d.l_simple_weight * gamma + (double)d.original_elbo_weight * vlb);
    }
}

}  // namespace

extern "C" int frido_qsample(const FridoQSample* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->x0 && d->x_noisy && d->t && d->sqrt_ac && d->sqrt_1mac, "null pointer");
    FRIDO_REQUIRE(d->B > 0 && d->HW > 0 && d->Cx > 0 && d->T > 0, "B, HW, Cx and T must be positive");
    FRIDO_REQUIRE(d->ch_start >= 0 && d->ch_start < d->ch_end && d->ch_end <= d->Cx, "the channel range must lie inside [0, Cx]");
    FRIDO_REQUIRE(d->mix_tau == d->mix_tau, "mix_tau is NaN");
    FRIDO_REQUIRE(d->noise || ((int64_t)d->HW * d->Cx) % 4 == 0, "Philox noise is numbered in groups of 4 floats: HW * Cx must be a multiple of 4");
    FRIDO_REQUIRE((int64_t)d->HW * d->Cx < ((int64_t)1 << 33), "a sample has more Philox groups than the 32-bit group counter holds");
    const bool vec = d->Cx % 4 == 0 && d->ch_end % 4 == 0;
    FRIDO_REQUIRE(!vec || (aligned16(d->x0) && aligned16(d->x_noisy) && aligned16(d->noise)), "16-byte accesses: x0, x_noisy and noise must be 16-byte aligned");
    // torch multiplies the f32 tensor by the Python doubles (1 - mix_tau) and mix_tau, each cast to f32
    const float keep = (float)(1.0 - d->mix_tau), mix = (float)d->mix_tau;
    const int64_t n = (int64_t)d->B * d->HW * d->ch_end;
    if (vec)
        hipLaunchKernelGGL(qsample_kernel<4>, dim3(grid_for(n / 4, LOSS_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, keep, mix, n / 4);
    else
        hipLaunchKernelGGL(qsample_kernel<1>, dim3(grid_for(n, LOSS_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, keep, mix, n);
    return frido_check_launch("qsample");
}

extern "C" int frido_diffusion_loss(const FridoDiffusionLoss* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->pred && d->per_sample, "null pointer");
    FRIDO_REQUIRE(!d->out || (d->t && d->logvar && d->lvlb_weights && d->T > 0), "the stage row needs t, logvar, lvlb_weights and T");
    FRIDO_REQUIRE(d->B > 0 && d->HW > 0 && d->Cx > 0 && d->nch > 0, "B, HW, Cx and nch must be positive");
    FRIDO_REQUIRE(d->ch_start >= 0 && (int64_t)d->ch_start + d->nch <= d->Cx, "the channel range must lie inside [0, Cx]");
    FRIDO_REQUIRE(d->loss_type == 0 || d->loss_type == 1, "unknown loss type: 0 (l1) or 1 (l2)");
    FRIDO_REQUIRE(d->noise || ((int64_t)d->HW * d->Cx) % 4 == 0, "Philox noise is numbered in groups of 4 floats: HW * Cx must be a multiple of 4");
    FRIDO_REQUIRE((int64_t)d->HW * d->Cx < ((int64_t)1 << 33), "a sample has more Philox groups than the 32-bit group counter holds");
    const bool vec = d->Cx % 4 == 0 && d->ch_start % 4 == 0 && d->nch % 4 == 0;
    FRIDO_REQUIRE(!vec || (aligned16(d->pred) && aligned16(d->noise)), "16-byte accesses: pred and noise must be 16-byte aligned");
    if (vec)
        hipLaunchKernelGGL(loss_sample_kernel<4>, dim3(d->B), dim3(256), 0, (hipStream_t)s, *d);
    else
        hipLaunchKernelGGL(loss_sample_kernel<1>, dim3(d->B), dim3(256), 0, (hipStream_t)s, *d);
    if (d->out) {
        const int rc = frido_check_launch("diffusion_loss");
        if (rc != FRIDO_OK) return rc;
        hipLaunchKernelGGL(loss_row_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, *d);
    }
    return frido_check_launch("diffusion_loss");
}
