// The launches of the Inception Score and the Kernel Inception Distance (include/frido_fidelity.h): row dot products in f64 with their
// four epilogues, the finish of the MMD^2 estimate, the four steps of the Inception Score.  Plain f32 / f64 arithmetic: no operand
// planes, so no status word (launch.h alone, like fid.hip) and the two builds of the library compile the same code.  Nothing is added
// across threads except by the written shuffle trees, and every sum has a fixed order: a replay returns the same bits.  The build
// contracts a * b + c into an fma (-ffp-contract=on); where the header promises separately rounded operations the contraction is
// switched off locally.
// frido_rows_dot is the one compute kernel: 2 RX RY D f64 FMAs on the vector pipe (KID at its defaults: 3 x 100 x 1000^2 x 2048 FMAs).
#include "launch.h"
#include "frido_fidelity.h"

namespace {

constexpr int ISC_GRID_CAP = 1024;        // 4 workgroups per CU, as in fid.hip
constexpr int TILE = 64;                  // pairs per tile side
constexpr int KC = 32;                    // floats of D staged per chunk: 2 x 32 x 68 x 4 B = 17 KB of LDS, one float4 per thread, row half and operand
// The LDS images are [k][row] (k-major), so that a thread reads its four rows at one k as ONE 16-byte ds_read: a wave's X reads are 4
// distinct slots (ty) broadcast over tx, its Y reads the 16 slots of one 256-byte bank row -- conflict-free with any row stride that
// is a multiple of 4 floats.  The padding is for the transposed staging WRITES (4-byte, banks of 32 dwords, lanes of a 32-lane half:
// 8 k-quads x 4 rows): bank = (k * LDT + row) % 32 is one bank for all k at LDT = 64 (8-way per row) and 16 kq + 4 j + row at
// LDT = 68 (4-way).  An odd stride would make them conflict-free but break the 16-byte alignment of the reads, which are the
// 2 x 32 per chunk and thread against 8 writes.  All of this is derived from the bank rule and the code, NOT measured (no counter run):
// by that estimate the writes' 4-way conflict costs about 3 % of the time of the chunk's 512 FMAs.
constexpr int LDT = TILE + 4;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// ((t * t) * t) * t with t = dot * gamma + coef0, every operation rounded on its own
__device__ __forceinline__ double poly(double dot, double gamma, double coef0, int degree) {
#pragma clang fp contract(off)
    const double t = __dadd_rn(__dmul_rn(dot, gamma), coef0);
    double r = t;
    for (int p = 1; p < degree; ++p) r = __dmul_rn(r, t);
    return r;
}

// the row of X (Y) that position `a` of subset `s` stands for, or null (a row of zeros): behind the subset's end, or an index outside
__device__ __forceinline__ const float* row_of(const float* base, const int32_t* idx, int64_t s, int m, int a, int R, int n, int D) {
    if (a >= R) return nullptr;
    const int r = idx ? idx[s * m + a] : a;
    return (r >= 0 && r < n) ? base + (int64_t)r * D : nullptr;
}

__device__ __forceinline__ float4 load_or_zero(const float* row, int k, int D) {
    return (row && k < D) ? *reinterpret_cast<const float4*>(row + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// Workgroup = one 64 x 64 tile of pairs per trip; thread (ty, tx) = (t / 16, t % 16) owns pairs a = i0 + 4 ty .. + 3, b = j0 + 4 tx .. + 3:
// sixteen f64 accumulators.  Staging: thread t loads k-quad t % 8 of rows t / 8 and t / 8 + 32 of both operands, 8 lanes on 128
// contiguous bytes of a row, and holds the NEXT chunk in registers while the current one is multiplied.  Rows behind the subset's
// end and k behind D are zeros: fma(0, 0, acc) leaves acc as it is, and those pairs are neither stored nor summed.
__global__ __launch_bounds__(256) void rows_dot_kernel(const FridoRowsDot d, int RX, int RY, int ntx, int nty, int64_t T, int64_t total) {
    __shared__ __attribute__((aligned(16))) float xs[KC * LDT], ys[KC * LDT];
    __shared__ double wsum[4];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int sr = t >> 3, sk = (t & 7) * 4;
    for (int64_t g = blockIdx.x; g < total; g += gridDim.x) {
        const int64_t s = g / T;
        int rem = (int)(g - s * T), ti, tj;
        if (d.symmetric) {
            ti = 0;
            while (rem >= ntx - ti) { rem -= ntx - ti; ++ti; }
            tj = ti + rem;
        } else {
            ti = rem / nty;
            tj = rem - ti * nty;
        }
        const int i0 = ti * TILE, j0 = tj * TILE;
        const float *xr[2], *yr[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            xr[h] = row_of(d.x, d.ix, s, d.m, i0 + sr + 32 * h, RX, d.nx, d.D);
            yr[h] = row_of(d.y, d.iy, s, d.m, j0 + sr + 32 * h, RY, d.ny, d.D);
        }
        double acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
        }
        float4 px[2], py[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            px[h] = load_or_zero(xr[h], sk, d.D);
            py[h] = load_or_zero(yr[h], sk, d.D);
        }
        for (int k0 = 0; k0 < d.D; k0 += KC) {
            __syncthreads();                                    // the previous chunk (or trip) has been read
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = sr + 32 * h;
                xs[(sk + 0) * LDT + r] = px[h].x; xs[(sk + 1) * LDT + r] = px[h].y; xs[(sk + 2) * LDT + r] = px[h].z; xs[(sk + 3) * LDT + r] = px[h].w;
                ys[(sk + 0) * LDT + r] = py[h].x; ys[(sk + 1) * LDT + r] = py[h].y; ys[(sk + 2) * LDT + r] = py[h].z; ys[(sk + 3) * LDT + r] = py[h].w;
            }
            __syncthreads();
            if (k0 + KC < d.D) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    px[h] = load_or_zero(xr[h], k0 + KC + sk, d.D);
                    py[h] = load_or_zero(yr[h], k0 + KC + sk, d.D);
                }
            }
#pragma unroll 8
            for (int k = 0; k < KC; ++k) {
                const float4 xa = *reinterpret_cast<const float4*>(&xs[k * LDT + 4 * ty]);
                const float4 yb = *reinterpret_cast<const float4*>(&ys[k * LDT + 4 * tx]);
                const double xv[4] = {(double)xa.x, (double)xa.y, (double)xa.z, (double)xa.w};
                const double yv[4] = {(double)yb.x, (double)yb.y, (double)yb.z, (double)yb.w};
#pragma unroll
                for (int a = 0; a < 4; ++a) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[a][c] = fma(xv[a], yv[c], acc[a][c]);
                }
            }
        }
        const int pa0 = i0 + 4 * ty, pb0 = j0 + 4 * tx;
        if (d.mode == FRIDO_ROWS_DOT_SUM_POLY) {
            double local = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int pa = pa0 + a, pb = pb0 + c;
                    if (pa < RX && pb < RY && !(d.exclude_diag && pa == pb)) local += poly(acc[a][c], d.gamma, d.coef0, d.degree);
                }
            }
            local = wave_sum(local);
            if ((t & 63) == 0) wsum[t >> 6] = local;
            __syncthreads();
            if (t == 0) {
                const double v = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
                d.partials[g] = (d.symmetric && tj > ti) ? 2.0 * v : v;
            }
            continue;                                           // wsum is written again behind the next trip's two barriers at the least
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int pa = pa0 + a;
            if (pa >= RX) continue;
            const int64_t o = (s * RX + pa) * (int64_t)d.ldo + pb0;
            if (d.mode == FRIDO_ROWS_DOT_STORE_F32) {
                float* op = static_cast<float*>(d.out) + o;
                const float v[4] = {(float)acc[a][0], (float)acc[a][1], (float)acc[a][2], (float)acc[a][3]};
                if (pb0 + 4 <= RY && (d.ldo & 3) == 0) store_vec<4>(op, v);
                else {
                    for (int c = 0; c < 4; ++c) {
                        if (pb0 + c < RY) op[c] = v[c];
                    }
                }
            } else {
                double* op = static_cast<double*>(d.out) + o;
                double v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = d.mode == FRIDO_ROWS_DOT_STORE_F64 ? acc[a][c] : poly(acc[a][c], d.gamma, d.coef0, d.degree);
                if (pb0 + 4 <= RY && (d.ldo & 1) == 0) {
                    *reinterpret_cast<double2*>(op) = make_double2(v[0], v[1]);
                    *reinterpret_cast<double2*>(op + 2) = make_double2(v[2], v[3]);
                } else {
                    for (int c = 0; c < 4; ++c) {
                        if (pb0 + c < RY) op[c] = v[c];
                    }
                }
            }
        }
    }
}

// one thread per subset: the partials in tile order
__global__ __launch_bounds__(256) void mmd_finish_kernel(const FridoMmdFinish d) {
#pragma clang fp contract(off)
    for (int s = blockIdx.x * 256 + threadIdx.x; s < d.S; s += gridDim.x * 256) {
        double sxx = 0.0, syy = 0.0, sxy = 0.0;
        for (int i = 0; i < d.nxx; ++i) sxx += d.pxx[(int64_t)s * d.nxx + i];
        for (int i = 0; i < d.nyy; ++i) syy += d.pyy[(int64_t)s * d.nyy + i];
        for (int i = 0; i < d.nxy; ++i) sxy += d.pxy[(int64_t)s * d.nxy + i];
        const double m = (double)d.m;
        const double mmd2 = __dsub_rn(__ddiv_rn(__dadd_rn(sxx, syy), __dmul_rn(m, m - 1.0)), __ddiv_rn(__dmul_rn(2.0, sxy), __dmul_rn(m, m)));
        double* o = d.out + 4 * (int64_t)s;
        *reinterpret_cast<double2*>(o) = make_double2(sxx, syy);
        *reinterpret_cast<double2*>(o + 2) = make_double2(sxy, mmd2);
    }
}

__device__ __forceinline__ const float* isc_row(const FridoIsc& d, int p) {
    int r = d.perm[p];
    r = r < 0 ? 0 : (r >= d.N ? d.N - 1 : r);
    return d.logits + (int64_t)r * d.C;
}
// first position of split i
__device__ __forceinline__ int isc_lo(const FridoIsc& d, int i) { return (int)((int64_t)i * d.N / d.splits); }

// one wave per position; the lanes read 256 contiguous bytes of the row per step, 4 bytes each: the lane order the header fixes
// (lane j owns c = j, j + 64, ...) rules out 16-byte loads here and in the two kernels below
__global__ __launch_bounds__(256) void isc_rowstats_kernel(const FridoIsc d) {
    const int lane = threadIdx.x & 63;
    for (int p = blockIdx.x * 4 + (threadIdx.x >> 6); p < d.N; p += gridDim.x * 4) {
        const float* l = isc_row(d, p);
        double mx = -INFINITY;
        for (int c = lane; c < d.C; c += 64) mx = fmax(mx, (double)l[c]);
        mx = wave_max(mx);
        double sum = 0.0;
        for (int c = lane; c < d.C; c += 64) sum += exp((double)l[c] - mx);
        sum = wave_sum(sum);
        if (lane == 0) *reinterpret_cast<double2*>(d.rowstats + 2 * (int64_t)p) = make_double2(mx, log(sum));
    }
}

// one thread per (split, column), the split's positions in order; a wave reads 256 contiguous bytes of each row
__global__ __launch_bounds__(256) void isc_marginal_kernel(const FridoIsc d, int64_t units) {
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
        const int i = (int)(u / d.C), c = (int)(u - (int64_t)i * d.C);
        const int lo = isc_lo(d, i), hi = isc_lo(d, i + 1);
        double sum = 0.0;
        for (int p = lo; p < hi; ++p) {
            const double2 st = *reinterpret_cast<const double2*>(d.rowstats + 2 * (int64_t)p);
            sum += exp(((double)isc_row(d, p)[c] - st.x) - st.y);
        }
        d.q[u] = sum / (double)(hi - lo);
    }
}

__global__ __launch_bounds__(256) void isc_kl_kernel(const FridoIsc d) {
    const int lane = threadIdx.x & 63;
    for (int p = blockIdx.x * 4 + (threadIdx.x >> 6); p < d.N; p += gridDim.x * 4) {
        const float* l = isc_row(d, p);
        const int i = (int)((((int64_t)p + 1) * d.splits - 1) / d.N);      // the split whose positions hold p
        const double* q = d.q + (int64_t)i * d.C;
        const double2 st = *reinterpret_cast<const double2*>(d.rowstats + 2 * (int64_t)p);
        double sum = 0.0;
        for (int c = lane; c < d.C; c += 64) {
            const double logp = ((double)l[c] - st.x) - st.y, p = exp(logp);
            if (p > 0.0) sum += p * (logp - log(q[c]));         // p == 0 (logp below -745): the term's limit 0, not 0 * inf
        }
        sum = wave_sum(sum);
        if (lane == 0) d.kl[p] = sum;
    }
}

__global__ __launch_bounds__(256) void isc_finish_kernel(const FridoIsc d) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < d.splits; i += gridDim.x * 256) {
        const int lo = isc_lo(d, i), hi = isc_lo(d, i + 1);
        double sum = 0.0;
        for (int p = lo; p < hi; ++p) sum += d.kl[p];
        d.scores[i] = exp(sum / (double)(hi - lo));
    }
}

inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// the four launchers of the Inception Score take one descriptor: its refusals, under the name of the launcher that meets them
#define FRIDO_ISC_REQUIRE(d)                                                                                                              \
    FRIDO_REQUIRE(d && d->logits && d->perm && d->rowstats && d->q && d->kl && d->scores, "bad arguments");                               \
    FRIDO_REQUIRE(d->N > 0 && d->C > 0, "N and C must be positive");                                                                      \
    FRIDO_REQUIRE(d->splits >= 1 && d->splits <= d->N, "splits must lie in 1 .. N");                                                      \
    FRIDO_REQUIRE(aligned16(d->rowstats) && aligned8(d->q) && aligned8(d->kl) && aligned8(d->scores) && ((uintptr_t)d->logits & 3) == 0 && \
                  ((uintptr_t)d->perm & 3) == 0, "rowstats must be 16-byte, q, kl and scores 8-byte, logits and perm 4-byte aligned")

}  // namespace

extern "C" int frido_sizeof_rows_dot(void) { return (int)sizeof(FridoRowsDot); }
extern "C" int frido_sizeof_mmd_finish(void) { return (int)sizeof(FridoMmdFinish); }
extern "C" int frido_sizeof_isc(void) { return (int)sizeof(FridoIsc); }

extern "C" int frido_rows_dot(const FridoRowsDot* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->x && d->y && d->nx > 0 && d->ny > 0 && d->D > 0, "bad arguments");
    FRIDO_REQUIRE(d->D % 4 == 0, "D must be a multiple of 4");
    FRIDO_REQUIRE(aligned16(d->x) && aligned16(d->y), "x and y must be 16-byte aligned");
    FRIDO_REQUIRE(d->mode >= FRIDO_ROWS_DOT_STORE_F32 && d->mode <= FRIDO_ROWS_DOT_SUM_POLY,
                  "mode: store f32 (0), store f64 (1), store poly f64 (2) or sum poly (3)");
    FRIDO_REQUIRE((d->ix == nullptr) == (d->iy == nullptr), "ix and iy come together or not at all");
    const bool lists = d->ix != nullptr;
    FRIDO_REQUIRE(lists ? (d->S >= 1 && d->m >= 1) : (d->S == 1 && d->m == 0), "S, m: S >= 1 and m >= 1 with index lists, S == 1 and m == 0 without");
    FRIDO_REQUIRE(!lists || ((((uintptr_t)d->ix | (uintptr_t)d->iy) & 3) == 0), "ix and iy must be 4-byte aligned");
    const int RX = lists ? d->m : d->nx, RY = lists ? d->m : d->ny;
    const bool sum = d->mode == FRIDO_ROWS_DOT_SUM_POLY, pol = sum || d->mode == FRIDO_ROWS_DOT_STORE_POLY_F64;
    FRIDO_REQUIRE(!pol || (d->degree >= 1 && d->degree <= 4), "degree must lie in 1 .. 4");
    FRIDO_REQUIRE(d->exclude_diag == 0 || (d->exclude_diag == 1 && sum), "exclude_diag: 0, or 1 in mode sum poly");
    FRIDO_REQUIRE(d->symmetric == 0 || (d->symmetric == 1 && sum), "symmetric: 0, or 1 in mode sum poly");
    FRIDO_REQUIRE(!d->symmetric || (d->x == d->y && d->ix == d->iy && RX == RY), "symmetric needs y == x, iy == ix and as many rows on both sides");
    if (sum) {
        FRIDO_REQUIRE(d->partials && aligned8(d->partials), "partials must be given, 8-byte aligned");
    } else {
        FRIDO_REQUIRE(d->out && d->ldo >= RY, "out must be given with ldo >= the pairs of a row");
        FRIDO_REQUIRE(aligned16(d->out), "out must be 16-byte aligned");
    }
    const int ntx = (RX + TILE - 1) / TILE, nty = (RY + TILE - 1) / TILE;
    const int64_t T = d->symmetric ? (int64_t)ntx * (ntx + 1) / 2 : (int64_t)ntx * nty;
    FRIDO_REQUIRE(T < ((int64_t)1 << 31), "too many tiles in one subset");
    const int64_t total = T * d->S;
    const int grid = (int)(total < FRIDO_ROWS_DOT_GRID_CAP ? total : FRIDO_ROWS_DOT_GRID_CAP);
    hipLaunchKernelGGL(rows_dot_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, *d, RX, RY, ntx, nty, T, total);
    return frido_check_launch("rows_dot");
}

extern "C" int frido_mmd_finish(const FridoMmdFinish* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->pxx && d->pyy && d->pxy && d->out && d->S > 0, "bad arguments");
    FRIDO_REQUIRE(d->m >= 2, "m must be at least 2");
    FRIDO_REQUIRE(d->nxx > 0 && d->nyy > 0 && d->nxy > 0, "nxx, nyy and nxy must be positive");
    FRIDO_REQUIRE(aligned8(d->pxx) && aligned8(d->pyy) && aligned8(d->pxy) && aligned16(d->out), "the partials must be 8-byte, out 16-byte aligned");
    hipLaunchKernelGGL(mmd_finish_kernel, dim3(grid_for(d->S, ISC_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d);
    return frido_check_launch("mmd_finish");
}

extern "C" int frido_isc_rowstats(const FridoIsc* d, frido_stream_t s) {
    FRIDO_ISC_REQUIRE(d);
    const int grid = (int)(((int64_t)d->N + 3) / 4 < ISC_GRID_CAP ? ((int64_t)d->N + 3) / 4 : ISC_GRID_CAP);
    hipLaunchKernelGGL(isc_rowstats_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, *d);
    return frido_check_launch("isc_rowstats");
}

extern "C" int frido_isc_marginal(const FridoIsc* d, frido_stream_t s) {
    FRIDO_ISC_REQUIRE(d);
    const int64_t units = (int64_t)d->splits * d->C;
    hipLaunchKernelGGL(isc_marginal_kernel, dim3(grid_for(units, ISC_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, units);
    return frido_check_launch("isc_marginal");
}

extern "C" int frido_isc_kl(const FridoIsc* d, frido_stream_t s) {
    FRIDO_ISC_REQUIRE(d);
    const int grid = (int)(((int64_t)d->N + 3) / 4 < ISC_GRID_CAP ? ((int64_t)d->N + 3) / 4 : ISC_GRID_CAP);
    hipLaunchKernelGGL(isc_kl_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, *d);
    return frido_check_launch("isc_kl");
}

extern "C" int frido_isc_finish(const FridoIsc* d, frido_stream_t s) {
    FRIDO_ISC_REQUIRE(d);
    hipLaunchKernelGGL(isc_finish_kernel, dim3(grid_for(d->splits, ISC_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d);
    return frido_check_launch("isc_finish");
}
