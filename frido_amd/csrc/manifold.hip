// The scans of precision / recall and density / coverage (include/frido_manifold.h): row norms, the k-th nearest neighbour of every row
// and the ball-membership counts, on squared distances formed on the fly from a slab of frido_rows_dot's f64 dot products.  Plain f64
// and integer arithmetic: no operand planes, so no status word (launch.h alone, like fidelity.hip) and the two builds of the library
// compile the same code.  Every result is an integer count, a minimum or a value selected from the slab: nothing depends on an order
// of summation, and a replay returns the same bits.  The build contracts a * b + c into an fma (-ffp-contract=on); d2 is written with
// separately rounded operations and the contraction switched off locally, as the header promises.
// All four kernels are memory-bound: they read a slab element (8 bytes) for a handful of f64 operations.
#include "launch.h"
#include "frido_manifold.h"

namespace {

// (n(x) + n(y)) - 2.0 * dot, clamped at 0: every operation rounded on its own
__device__ __forceinline__ double d2_of(double na, double nb, double dot) {
#pragma clang fp contract(off)
    return fmax(__dsub_rn(__dadd_rn(na, nb), __dmul_rn(2.0, dot)), 0.0);
}

constexpr int AHEAD = 4;                  // trips of a scan loop whose loads are issued together: the scans live on loads in flight

// (d, b) < (e, c) lexicographically
__device__ __forceinline__ bool pair_less(double d, int b, double e, int c) { return d < e || (d == e && b < c); }

// one thread per row: the in-order chain of frido_rows_dot's diagonal, 16 bytes of the row per load
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const FridoRowSqnorm d) {
    for (int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x; a < d.n; a += (int64_t)gridDim.x * 256) {
        const float* r = d.x + a * d.D;
        double acc = 0.0;
        for (int q = 0; q < d.D; q += 4) {
            const float4 v = *reinterpret_cast<const float4*>(r + q);
            const double x0 = (double)v.x, x1 = (double)v.y, x2 = (double)v.z, x3 = (double)v.w;
            acc = fma(x0, x0, acc);
            acc = fma(x1, x1, acc);
            acc = fma(x2, x2, acc);
            acc = fma(x3, x3, acc);
        }
        d.out[a] = acc;
    }
}

// one wave per slab row; K rounds of a wave-wide lexicographic minimum over the pairs (d2, b) behind the previous round's pair
__global__ __launch_bounds__(256) void knn_select_kernel(const FridoKnnSelect d) {
    const int lane = threadIdx.x & 63, npair = d.ny >> 1;
    for (int a = blockIdx.x * 4 + (threadIdx.x >> 6); a < d.rows; a += gridDim.x * 4) {
        const double* row = d.slab + (int64_t)a * d.ldo;
        const double na = d.nrow[a];
        double pd = -1.0;                                       // d2 >= 0: every pair lies behind (-1.0, -1)
        int pb = -1;
        for (int r = 0; r < d.K; ++r) {
            double bd = INFINITY;
            int bb = INT32_MAX;
            const auto take = [&](double v, int b) {
                const bool t = pair_less(pd, pb, v, b) && pair_less(v, b, bd, bb);
                bd = t ? v : bd;
                bb = t ? b : bb;
            };
            int p = lane;
            for (; p + 64 * (AHEAD - 1) < npair; p += 64 * AHEAD) {      // the loads of AHEAD trips are issued before the first is used
                double2 s[AHEAD], n[AHEAD];
#pragma unroll
                for (int u = 0; u < AHEAD; ++u) {
                    s[u] = *reinterpret_cast<const double2*>(row + 2 * (p + 64 * u));
                    n[u] = *reinterpret_cast<const double2*>(d.ncol + 2 * (p + 64 * u));
                }
#pragma unroll
                for (int u = 0; u < AHEAD; ++u) {
                    take(d2_of(na, n[u].x, s[u].x), 2 * (p + 64 * u));
                    take(d2_of(na, n[u].y, s[u].y), 2 * (p + 64 * u) + 1);
                }
            }
            for (; p < npair; p += 64) {
                const double2 s = *reinterpret_cast<const double2*>(row + 2 * p), n = *reinterpret_cast<const double2*>(d.ncol + 2 * p);
                take(d2_of(na, n.x, s.x), 2 * p);
                take(d2_of(na, n.y, s.y), 2 * p + 1);
            }
            if ((d.ny & 1) && lane == 0) take(d2_of(na, d.ncol[d.ny - 1], row[d.ny - 1]), d.ny - 1);      // the last column of an odd ny: the padding behind it is not read
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double od = __shfl_xor(bd, off, 64);
                const int ob = __shfl_xor(bb, off, 64);
                if (pair_less(od, ob, bd, bb)) {
                    bd = od;
                    bb = ob;
                }
            }
            pd = bd;
            pb = bb;
        }
        if (lane == 0) d.rad2[a] = pd;
    }
}

// one wave per slab row: the columns whose ball holds the row
__global__ __launch_bounds__(256) void ball_rows_kernel(const FridoBallRows d) {
    const int lane = threadIdx.x & 63, npair = d.ny >> 1;
    for (int a = blockIdx.x * 4 + (threadIdx.x >> 6); a < d.rows; a += gridDim.x * 4) {
        const double* row = d.slab + (int64_t)a * d.ldo;
        const double na = d.nrow[a];
        int cnt = 0, p = lane;
        for (; p + 64 * (AHEAD - 1) < npair; p += 64 * AHEAD) {
            double2 s[AHEAD], n[AHEAD], r[AHEAD];
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) {
                s[u] = *reinterpret_cast<const double2*>(row + 2 * (p + 64 * u));
                n[u] = *reinterpret_cast<const double2*>(d.ncol + 2 * (p + 64 * u));
                r[u] = *reinterpret_cast<const double2*>(d.rad2_col + 2 * (p + 64 * u));
            }
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) cnt += (int)(d2_of(na, n[u].x, s[u].x) <= r[u].x) + (int)(d2_of(na, n[u].y, s[u].y) <= r[u].y);
        }
        for (; p < npair; p += 64) {
            const double2 s = *reinterpret_cast<const double2*>(row + 2 * p), n = *reinterpret_cast<const double2*>(d.ncol + 2 * p);
            const double2 r = *reinterpret_cast<const double2*>(d.rad2_col + 2 * p);
            cnt += (int)(d2_of(na, n.x, s.x) <= r.x) + (int)(d2_of(na, n.y, s.y) <= r.y);
        }
        if ((d.ny & 1) && lane == 0) cnt += (int)(d2_of(na, d.ncol[d.ny - 1], row[d.ny - 1]) <= d.rad2_col[d.ny - 1]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if (lane == 0) d.cnt[a] = cnt;
    }
}

// a workgroup per tile of 32 columns, its eight half-waves on every eighth slab row; thread (0, col) alone updates the column
__global__ __launch_bounds__(256) void ball_cols_kernel(const FridoBallCols d, int tiles) {
    __shared__ int scnt[8][32];
    __shared__ double smin[8][32];
    const int col = threadIdx.x & 31, grp = threadIdx.x >> 5;
    for (int c = blockIdx.x; c < tiles; c += gridDim.x) {
        const int b = c * 32 + col;
        int cnt = 0;
        double mn = INFINITY;
        if (b < d.ny) {
            const double nb = d.ncol[b];
            const double* p = d.slab + b;
            int a = grp;
            for (; a + 8 * (AHEAD - 1) < d.rows; a += 8 * AHEAD) {
                double s[AHEAD];
#pragma unroll
                for (int u = 0; u < AHEAD; ++u) s[u] = p[(int64_t)(a + 8 * u) * d.ldo];
#pragma unroll
                for (int u = 0; u < AHEAD; ++u) {
                    const double v = d2_of(d.nrow[a + 8 * u], nb, s[u]);
                    cnt += (int)(v <= d.rad2_row[a + 8 * u]);
                    mn = fmin(mn, v);
                }
            }
            for (; a < d.rows; a += 8) {
                const double v = d2_of(d.nrow[a], nb, p[(int64_t)a * d.ldo]);
                cnt += (int)(v <= d.rad2_row[a]);
                mn = fmin(mn, v);
            }
        }
        scnt[grp][col] = cnt;
        smin[grp][col] = mn;
        __syncthreads();
        if (grp == 0 && b < d.ny) {
#pragma unroll
            for (int g = 1; g < 8; ++g) {
                cnt += scnt[g][col];
                mn = fmin(mn, smin[g][col]);
            }
            d.cnt_col[b] += cnt;
            d.dmin_col[b] = fmin(d.dmin_col[b], mn);
        }
        __syncthreads();                                        // the next tile writes scnt and smin again
    }
}

inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
inline int waves_grid(int rows) {
    const int64_t b = ((int64_t)rows + 3) / 4;
    return (int)(b < FRIDO_MANIFOLD_GRID_CAP ? b : FRIDO_MANIFOLD_GRID_CAP);
}

// what the three slab launchers ask of a slab, under the name of the launcher that meets it
#define FRIDO_SLAB_REQUIRE(d)                                                                                              \
    FRIDO_REQUIRE(d->rows > 0 && d->ny > 0 && d->ny <= (1 << 30), "rows must be positive, ny in 1 .. 2^30");               \
    FRIDO_REQUIRE(d->ldo >= d->ny, "ldo must be at least ny")

}  // namespace

extern "C" int frido_sizeof_row_sqnorm(void) { return (int)sizeof(FridoRowSqnorm); }
extern "C" int frido_sizeof_knn_select(void) { return (int)sizeof(FridoKnnSelect); }
extern "C" int frido_sizeof_ball_rows(void) { return (int)sizeof(FridoBallRows); }
extern "C" int frido_sizeof_ball_cols(void) { return (int)sizeof(FridoBallCols); }

extern "C" int frido_row_sqnorm(const FridoRowSqnorm* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->x && d->out && d->n > 0 && d->D > 0, "bad arguments");
    FRIDO_REQUIRE(d->D % 4 == 0, "D must be a multiple of 4");
    FRIDO_REQUIRE(aligned16(d->x) && aligned8(d->out), "x must be 16-byte, out 8-byte aligned");
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3(grid_for(d->n, FRIDO_MANIFOLD_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d);
    return frido_check_launch("row_sqnorm");
}

extern "C" int frido_knn_select(const FridoKnnSelect* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->slab && d->nrow && d->ncol && d->rad2, "bad arguments");
    FRIDO_SLAB_REQUIRE(d);
    FRIDO_REQUIRE(d->ldo % 2 == 0, "ldo must be even");
    FRIDO_REQUIRE(d->K >= 1 && d->K <= FRIDO_MANIFOLD_MAX_K + 1 && d->K <= d->ny, "K must lie in 1 .. min(ny, FRIDO_MANIFOLD_MAX_K + 1)");
    FRIDO_REQUIRE(aligned16(d->slab) && aligned16(d->ncol) && aligned8(d->nrow) && aligned8(d->rad2),
                  "slab and ncol must be 16-byte, nrow and rad2 8-byte aligned");
    hipLaunchKernelGGL(knn_select_kernel, dim3(waves_grid(d->rows)), dim3(256), 0, (hipStream_t)s, *d);
    return frido_check_launch("knn_select");
}

extern "C" int frido_ball_rows(const FridoBallRows* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->slab && d->nrow && d->ncol && d->rad2_col && d->cnt, "bad arguments");
    FRIDO_SLAB_REQUIRE(d);
    FRIDO_REQUIRE(d->ldo % 2 == 0, "ldo must be even");
    FRIDO_REQUIRE(aligned16(d->slab) && aligned16(d->ncol) && aligned16(d->rad2_col) && aligned8(d->nrow) && ((uintptr_t)d->cnt & 3) == 0,
                  "slab, ncol and rad2_col must be 16-byte, nrow 8-byte, cnt 4-byte aligned");
    hipLaunchKernelGGL(ball_rows_kernel, dim3(waves_grid(d->rows)), dim3(256), 0, (hipStream_t)s, *d);
    return frido_check_launch("ball_rows");
}

extern "C" int frido_ball_cols(const FridoBallCols* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->slab && d->nrow && d->ncol && d->rad2_row && d->cnt_col && d->dmin_col, "bad arguments");
    FRIDO_SLAB_REQUIRE(d);
    FRIDO_REQUIRE(aligned8(d->slab) && aligned8(d->nrow) && aligned8(d->ncol) && aligned8(d->rad2_row) && aligned8(d->dmin_col) &&
                  ((uintptr_t)d->cnt_col & 3) == 0, "slab, nrow, ncol, rad2_row and dmin_col must be 8-byte, cnt_col 4-byte aligned");
    const int tiles = (d->ny + 31) / 32;
    hipLaunchKernelGGL(ball_cols_kernel, dim3(tiles < FRIDO_MANIFOLD_GRID_CAP ? tiles : FRIDO_MANIFOLD_GRID_CAP), dim3(256), 0, (hipStream_t)s, *d, tiles);
    return frido_check_launch("ball_cols");
}
