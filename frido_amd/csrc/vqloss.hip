// The codebook / commitment loss of the MS-VQGAN (taming/models/msvqgan.py:116-154 MSFPNVQModel.encode: emb_loss = sum(emb_loss_ms);
// taming/modules/vqvae/quantize.py:286-291 VectorQuantizer2.forward: mean((z_q - z)^2) twice, weighted 1 and beta).
// Plain f32 / f64 arithmetic: no operand planes, so no status word (launch.h alone: common.h is not included on purpose -- it would register one) and
// the two builds of the library compile the same code.  Bandwidth-bound and small: the maps are the e-channel latents of every scale.
#include "launch.h"

namespace {

constexpr int MAXS = FRIDO_VQLOSS_MAX_SCALES, MAXWG = FRIDO_VQLOSS_MAX_WG;
constexpr int64_t UNITS_PER_WG = 256 * 16;      // a workgroup is worth starting for 16 units per thread

// Workgroups of a scale: a function of the scale's OWN size only, so its partials -- and its mean -- do not depend on which other scales
// share the launch.
inline int wgs_of(int64_t units) {
    const int64_t n = (units + UNITS_PER_WG - 1) / UNITS_PER_WG;
    return (int)(n < 1 ? 1 : (n > MAXWG ? MAXWG : n));
}

struct Split { int32_t wg0[MAXS + 1]; int32_t vec[MAXS]; };      // first workgroup of every scale; 16-byte (1) or scalar (0) accesses

// Workgroup w of a scale's n: thread j owns units w * 256 + j, + n * 256, ... (a unit = V consecutive channels of one pixel) and adds
// their fp32 squares into an f64 partial in that order; the 256 partials are added pairwise through LDS (loss.hip's scheme).  No atomic:
// the same bits on every launch.
template <int V>
__device__ __forceinline__ double scale_partial(const FridoVqCommitLoss& d, int s, int w, int n) {
    const int cv = d.e[s] / V;
    const int64_t units = d.npix[s] * cv;
    const float* z = d.z[s] + d.c0[s];
    const float* q = d.zq[s] + d.c0[s];
    double acc = 0.0;
    for (int64_t i = (int64_t)w * 256 + threadIdx.x; i < units; i += (int64_t)n * 256) {
        const int64_t p = i / cv;
        const int64_t o = p * d.C[s] + (i - p * cv) * V;
        if constexpr (V == 4) {
            const float4 a = *reinterpret_cast<const float4*>(z + o), b = *reinterpret_cast<const float4*>(q + o);
            const float d0 = __fsub_rn(b.x, a.x), d1 = __fsub_rn(b.y, a.y), d2 = __fsub_rn(b.z, a.z), d3 = __fsub_rn(b.w, a.w);
            acc += (double)__fmul_rn(d0, d0);
            acc += (double)__fmul_rn(d1, d1);
            acc += (double)__fmul_rn(d2, d2);
            acc += (double)__fmul_rn(d3, d3);
        } else {
            const float df = __fsub_rn(q[o], z[o]);
            acc += (double)__fmul_rn(df, df);
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void vqloss_partial_kernel(const FridoVqCommitLoss d, const Split sp) {
    __shared__ double part[256];
    int s = 0;
    while (s + 1 < d.n_scales && (int)blockIdx.x >= sp.wg0[s + 1]) ++s;      // uniform per workgroup
    const int w = (int)blockIdx.x - sp.wg0[s], n = sp.wg0[s + 1] - sp.wg0[s];
    part[threadIdx.x] = sp.vec[s] ? scale_partial<4>(d, s, w, n) : scale_partial<1>(d, s, w, n);
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) d.partials[s * MAXWG + w] = part[0];
}

// Lane s adds scale s's workgroup partials in index order and rounds the mean to fp32; lane 0 then forms the reference's expression.
__global__ __launch_bounds__(64) void vqloss_finish_kernel(const FridoVqCommitLoss d, const Split sp) {
    __shared__ float mean[MAXS];
    const int s = threadIdx.x;
    if (s < d.n_scales) {
        const int n = sp.wg0[s + 1] - sp.wg0[s];
        double sum = 0.0;
        for (int w = 0; w < n; ++w) sum += d.partials[s * MAXWG + w];
        const float m = (float)(sum / (double)(d.npix[s] * (int64_t)d.e[s]));
        mean[s] = m;
        d.out[s] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.0f;                                    // sum(emb_loss_ms): 0 + l_0 + l_1 + ..., coarse first
        for (int k = 0; k < d.n_scales; ++k) {
            const float bm = __fmul_rn(d.beta, mean[k]);
            const float l = d.legacy ? __fadd_rn(mean[k], bm) : __fadd_rn(bm, mean[k]);      // quantize.py:287-291
            total = __fadd_rn(total, l);
        }
        *d.emb_loss = total;
    }
}

}  // namespace

extern "C" int frido_vq_commit_loss(const FridoVqCommitLoss* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->partials && d->out && d->emb_loss, "null pointer");
    FRIDO_REQUIRE(d->n_scales >= 1 && d->n_scales <= MAXS, "1 to 4 scales");
    FRIDO_REQUIRE(d->beta == d->beta, "beta is NaN");
    FRIDO_REQUIRE(aligned16(d->partials), "the partials workspace must be 16-byte aligned");
    Split sp = {};
    for (int k = 0; k < d->n_scales; ++k) {
        FRIDO_REQUIRE(d->z[k] && d->zq[k], "null pointer");
        FRIDO_REQUIRE(d->npix[k] > 0 && d->C[k] > 0 && d->e[k] > 0, "npix, C and e must be positive");
        FRIDO_REQUIRE(d->c0[k] >= 0 && (int64_t)d->c0[k] + d->e[k] <= d->C[k], "the channel slice must lie inside [0, C]");
        FRIDO_REQUIRE(d->npix[k] <= ((int64_t)1 << 40), "npix is out of range");
        const bool vec = d->C[k] % 4 == 0 && d->c0[k] % 4 == 0 && d->e[k] % 4 == 0;
        FRIDO_REQUIRE(!vec || (aligned16(d->z[k]) && aligned16(d->zq[k])), "16-byte accesses: z and zq must be 16-byte aligned");
        sp.vec[k] = vec ? 1 : 0;
        sp.wg0[k + 1] = sp.wg0[k] + wgs_of(d->npix[k] * (d->e[k] / (vec ? 4 : 1)));
    }
    hipLaunchKernelGGL(vqloss_partial_kernel, dim3(sp.wg0[d->n_scales]), dim3(256), 0, (hipStream_t)s, *d, sp);
    const int rc = frido_check_launch("vq_commit_loss");
    if (rc != FRIDO_OK) return rc;
    hipLaunchKernelGGL(vqloss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, *d, sp);
    return frido_check_launch("vq_commit_loss");
}
