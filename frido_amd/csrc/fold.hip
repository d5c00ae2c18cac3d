// Patch-wise ("convolutional") mode of FridoDiffusion (frido/models/diffusion/frido.py:714-764, 1076-1152): the crops of an NHWC
// f32 map (nn.Unfold) and their weighted, normalised recombination (nn.Fold of o * weighting, divided by fold(weighting)).
// Plain f32 arithmetic: no operand planes, so no status word (launch.h alone: common.h is not included on purpose -- it would register one) and
// the two builds of the library compile the same code.  Both kernels move every byte once and are bandwidth-bound.
// Batch layout of the crop tensor (include/frido_hip.h): crop l of sample b is entry b * L + l.
#include "launch.h"

namespace {

constexpr int FOLD_GRID_CAP = 8192;

// One unit = V consecutive floats of a crop row (kw * C contiguous floats in the source AND in the destination).
template <int V>
__global__ __launch_bounds__(256) void unfold_kernel(const FridoUnfold d, int Lx, int L, int64_t units) {
    const int row = d.kw * d.C / V;                      // units per crop row
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i % row);
        const int64_t r = i / row;                       // (bc, ky)
        const int ky = (int)(r % d.kh);
        const int64_t bc = r / d.kh;
        const int l = (int)(bc % L);
        const int64_t b = bc / L;
        const int y = (l / Lx) * d.sy + ky, x0 = (l % Lx) * d.sx;
        const int64_t s = ((b * d.H + y) * d.W + x0) * d.C + (int64_t)j * V;
        const int64_t o = r * ((int64_t)d.kw * d.C) + (int64_t)j * V;
        if (V == 4)
            *reinterpret_cast<float4*>(d.dst + o) = *reinterpret_cast<const float4*>(d.src + s);
        else
            d.dst[o] = d.src[s];
    }
}

__device__ __forceinline__ uint8_t fold_u8(float x, int mode) {      // FridoGemm.out_u8's two conversions (igemm_shared.h), expression for expression
    float u;
    if (mode == 2) u = __fmul_rn(255.0f, __fmul_rn(__fadd_rn(fminf(fmaxf(x, -1.0f), 1.0f), 1.0f), 0.5f));
    else u = fminf(fmaxf(__fmul_rn(__fadd_rn(x, 1.0f), 127.5f), 0.0f), 255.0f);
    return (uint8_t)u;
}

// One thread owns V consecutive channels of one output pixel and walks the crops that cover it in ascending l.
template <int V>
__global__ __launch_bounds__(256) void fold_kernel(const FridoFold d, int Ly, int Lx, int64_t units) {
    const int L = Ly * Lx, cv = d.C / V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % cv) * V;
        const int64_t p = i / cv;                        // (b, y, x)
        const int x = (int)(p % d.W);
        const int y = (int)((p / d.W) % d.H);
        const int64_t b = p / ((int64_t)d.W * d.H);
        // crops ly with ly * sy <= y < ly * sy + kh
        const int ly0 = y >= d.kh ? (y - d.kh) / d.sy + 1 : 0, ly1 = min(Ly - 1, y / d.sy);
        const int lx0 = x >= d.kw ? (x - d.kw) / d.sx + 1 : 0, lx1 = min(Lx - 1, x / d.sx);
        float acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.0f;
        for (int ly = ly0; ly <= ly1; ++ly) {
            const int yy = y - ly * d.sy;
            for (int lx = lx0; lx <= lx1; ++lx) {
                const int xx = x - lx * d.sx, l = ly * Lx + lx;
                const float w = d.wt[(int64_t)(yy * d.kw + xx) * L + l];
                const int64_t o = (((b * L + l) * d.kh + yy) * d.kw + xx) * d.C + c;
                float v[V];
                if (V == 4) {
                    const float4 q = *reinterpret_cast<const float4*>(d.crops + o);
                    v[0] = q.x; v[1 % V] = q.y; v[2 % V] = q.z; v[3 % V] = q.w;
                } else {
                    v[0] = d.crops[o];
                }
#pragma unroll
                for (int k = 0; k < V; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(v[k], w));      // the reference rounds o * weighting before fold sums
            }
        }
        const float nrm = d.norm[(int64_t)y * d.W + x];
        float r[V];
#pragma unroll
        for (int k = 0; k < V; ++k) r[k] = __fdiv_rn(acc[k], nrm);
        const int64_t q = p * d.C + c;
        if (d.out) {
            if (V == 4) *reinterpret_cast<float4*>(d.out + q) = make_float4(r[0], r[1 % V], r[2 % V], r[3 % V]);
            else d.out[q] = r[0];
        }
        if (d.out_u8) {
#pragma unroll
            for (int k = 0; k < V; ++k) d.out_u8[q + k] = fold_u8(r[k], d.u8_mode);
        }
    }
}

// exact tiling: the reference's fold(weighting) is 0 where no crop reaches, and it then divides 0 by 0
inline bool geometry_ok(int H, int W, int kh, int kw, int sy, int sx) {
    return H > 0 && W > 0 && kh > 0 && kw > 0 && sy > 0 && sx > 0 && kh <= H && kw <= W && (H - kh) % sy == 0 && (W - kw) % sx == 0;
}

}  // namespace

extern "C" int frido_unfold(const FridoUnfold* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->src && d->dst && d->B > 0 && d->C > 0, "bad arguments");
    FRIDO_REQUIRE(geometry_ok(d->H, d->W, d->kh, d->kw, d->sy, d->sx), "the crops must tile the map exactly: (H - kh) % sy == 0 and (W - kw) % sx == 0");
    const int Ly = (d->H - d->kh) / d->sy + 1, Lx = (d->W - d->kw) / d->sx + 1, L = Ly * Lx;
    const int64_t floats = (int64_t)d->B * L * d->kh * d->kw * d->C;
    // 16-byte accesses where every crop row starts on a 16-byte boundary on both sides and is a whole number of vectors long
    const bool vec = (d->kw * d->C) % 4 == 0 && (d->W * d->C) % 4 == 0 && (d->sx * d->C) % 4 == 0 && aligned16(d->src) && aligned16(d->dst);
    if (vec)
        hipLaunchKernelGGL(unfold_kernel<4>, dim3(grid_for(floats / 4, FOLD_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, Lx, L, floats / 4);
    else
        hipLaunchKernelGGL(unfold_kernel<1>, dim3(grid_for(floats, FOLD_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, Lx, L, floats);
    return frido_check_launch("unfold");
}

extern "C" int frido_fold(const FridoFold* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->crops && d->wt && d->norm && (d->out || d->out_u8) && d->B > 0 && d->C > 0, "bad arguments");
    FRIDO_REQUIRE(geometry_ok(d->H, d->W, d->kh, d->kw, d->sy, d->sx), "the crops must tile the map exactly: (H - kh) % sy == 0 and (W - kw) % sx == 0");
    FRIDO_REQUIRE(!d->out_u8 || d->u8_mode == 1 || d->u8_mode == 2, "out_u8: u8_mode 1 (custom_to_np) or 2 (custom_to_pil)");
    const int Ly = (d->H - d->kh) / d->sy + 1, Lx = (d->W - d->kw) / d->sx + 1;
    const int64_t floats = (int64_t)d->B * d->H * d->W * d->C;
    const bool vec = d->C % 4 == 0 && aligned16(d->crops) && (!d->out || aligned16(d->out));
    if (vec)
        hipLaunchKernelGGL(fold_kernel<4>, dim3(grid_for(floats / 4, FOLD_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, Ly, Lx, floats / 4);
    else
        hipLaunchKernelGGL(fold_kernel<1>, dim3(grid_for(floats, FOLD_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, Ly, Lx, floats);
    return frido_check_launch("fold");
}
