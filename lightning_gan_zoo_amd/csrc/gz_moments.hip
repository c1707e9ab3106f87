// Mean and covariance of an activation set (the statistics behind the Frechet distance, reference
// core/callback_inception_metrics.py:223-231), in fp64, as numpy computes them:
//
//     mean = sum_rows(act) / n,   C = act - mean,   cov = (C^T C) * (1.0 / (n - 1))            (np.cov(act, rowvar=False))
//
// Three launches on one stream:
//   1. moments_colsum_kernel: every block of MOM_ROWS consecutive rows is summed per column, one thread per column,
//      row after row, into partial[block][column] (the workspace);
//   2. moments_mean_kernel: mean[column] = (partial[0] + partial[1] + ...) / n, the blocks in block order;
//   3. moments_tile_kernel: one workgroup per 64 x 64 tile (ti <= tj) of the upper triangle of cov, the whole sample axis
//      inside it, so no partial covariance ever meets another one.  The tile runs on the fp64 tile core (gz_f64_tile.h:
//      both operands [k][feature] images, the interleaved k-slot map):
//      * the reduction index of the GEMM is the SAMPLE row.  A 64-feature slice of a row is 512 contiguous bytes, so a
//        wave's global load is one row slice; a thread owns one feature of each operand and subtracts that feature's
//        mean as the value arrives.  Features >= d are zero in LDS; rows >= n are zero AFTER the subtraction (the
//        centred value is masked, not the raw one).  An entry is summed over the rows in row order (four at a time
//        inside an MFMA);
//      * epilogue: the tile times 1 / (n - 1) (the reciprocal is formed on the host, in fp64) goes through LDS (pitch 65:
//        the transposed read walks 2 banks per lane) and is stored twice with rows of 64 lanes along the fast axis: as
//        cov[ti rows][tj columns] and transposed as cov[tj rows][ti columns].  A diagonal tile stores only the entries
//        on and above the diagonal and mirrors those, so cov[i][j] and cov[j][i] are one value's bits everywhere.
// No floating-point atomics, a fixed order for every sum, nothing read from `mean`, `cov` or the workspace before this
// call wrote it: two calls give equal bits.
#include "gz_f64_tile.h"
#include "../../include/gz_ops.h"

namespace gz {

constexpr int MOM_THREADS = F64_THREADS;
constexpr int MOM_TILE = F64_TILE;            // features per tile side
constexpr int MOM_OUT_LD = MOM_TILE + 1;      // pitch of the epilogue's tile image
constexpr int MOM_ROWS = 512;                 // rows per partial column sum
static_assert(MOM_TILE * MOM_OUT_LD <= 2 * F64KCol::SIZE, "the epilogue's tile image reuses the operand images");

__global__ __launch_bounds__(MOM_THREADS) void moments_colsum_kernel(const double* __restrict__ act, long long n, int d,
                                                                     double* __restrict__ partial) {
    const int col = blockIdx.x * MOM_THREADS + threadIdx.x;
    if (col >= d) return;
    const long long r0 = (long long)blockIdx.y * MOM_ROWS;
    const long long r1 = r0 + MOM_ROWS < n ? r0 + MOM_ROWS : n;
    const double* p = act + r0 * d + col;
    double s = 0.0;
    for (long long r = r0; r < r1; ++r, p += d) s += *p;
    partial[(long long)blockIdx.y * d + col] = s;
}

__global__ __launch_bounds__(MOM_THREADS) void moments_mean_kernel(const double* __restrict__ partial, int nblk,
                                                                   long long n, int d, double* __restrict__ mean) {
    const int col = blockIdx.x * MOM_THREADS + threadIdx.x;
    if (col >= d) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += partial[(long long)b * d + col];
    mean[col] = s / (double)n;
}

// the thread's 8 sample rows of the chunk starting at row c0, feature f (mean m): centred, masked
__device__ __forceinline__ void moments_fetch(const double* __restrict__ act, long long n, int d, long long c0, int f,
                                              double m, double (&v)[F64_LOADS]) {
#pragma unroll
    for (int i = 0; i < F64_LOADS; ++i) {
        const long long row = c0 + F64KCol::own_k(threadIdx.x, i);
        v[i] = (row < n && f < d) ? act[row * d + f] - m : 0.0;
    }
}

__global__ __launch_bounds__(MOM_THREADS) void moments_tile_kernel(const double* __restrict__ act, long long n, int d,
                                                                   int tiles, const double* __restrict__ mean,
                                                                   double inv, double* __restrict__ cov) {
    __shared__ __attribute__((aligned(16))) double smem[2 * F64KCol::SIZE];

    int ti = 0, rest = (int)blockIdx.x;                  // tile (ti, tj), ti <= tj, rows of the triangle in order
    while (rest >= tiles - ti) {
        rest -= tiles - ti;
        ++ti;
    }
    const int tj = ti + rest;

    const int tid = threadIdx.x;
    const int lf = F64KCol::own_index(tid, 0);           // loader: feature within the slice
    const int fa = ti * MOM_TILE + lf, fb = tj * MOM_TILE + lf;
    const double ma = fa < d ? mean[fa] : 0.0, mb = fb < d ? mean[fb] : 0.0;

    f64x4 acc[4];
    f64_tile_mainloop<F64KCol, F64KCol, F64SlotInterleaved>(
        smem, smem + F64KCol::SIZE, (n + F64_KC - 1) / F64_KC,
        [&](long long c, double (&v)[F64_LOADS]) { moments_fetch(act, n, d, c * F64_KC, fa, ma, v); },
        [&](long long c, double (&v)[F64_LOADS]) { moments_fetch(act, n, d, c * F64_KC, fb, mb, v); }, acc);

    // acc[j][r] is the centred dot product of features ti*64 + f64_acc_row(r) and tj*64 + f64_acc_col(j)
    __syncthreads();                                     // the last chunk's readers are done with the images
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) smem[f64_acc_row(tid, r) * MOM_OUT_LD + f64_acc_col(tid, j)] = acc[j][r] * inv;
    __syncthreads();
    const int hi = tid & 63;
    for (int lo = tid >> 6; lo < MOM_TILE; lo += MOM_THREADS / 64) {
        {                                                // cov[ti rows][tj columns]: row lo, column hi
            const int gi = ti * MOM_TILE + lo, gj = tj * MOM_TILE + hi;
            if (gi < d && gj < d && gj >= gi) cov[(long long)gi * d + gj] = smem[lo * MOM_OUT_LD + hi];
        }
        {                                                // cov[tj rows][ti columns]: the transpose, row lo, column hi
            const int gi = ti * MOM_TILE + hi, gj = tj * MOM_TILE + lo;
            if (gi < d && gj < d && gj > gi) cov[(long long)gj * d + gi] = smem[hi * MOM_OUT_LD + lo];
        }
    }
}

inline int moments_row_blocks(long long n) { return (int)((n + MOM_ROWS - 1) / MOM_ROWS); }

}  // namespace gz

using namespace gz;

extern "C" {

size_t gz_feature_moments_workspace_bytes(long long n, int d) {
    if (n < 1 || d < 1) return 0;
    return (size_t)moments_row_blocks(n) * (size_t)d * sizeof(double);
}

int gz_feature_moments(const double* act, long long n, int d, double* mean, double* cov, void* workspace,
                       size_t ws_bytes, hipStream_t stream) {
    gz::clear_stale_error();
    if (n < 2 || d < 1 || !act || !mean || !cov || !workspace) return GZ_ERR_BAD_SHAPE;
    if (ws_bytes < gz_feature_moments_workspace_bytes(n, d)) return GZ_ERR_WORKSPACE;
    const long long tiles = ((long long)d + MOM_TILE - 1) / MOM_TILE;
    const long long blocks = tiles * (tiles + 1) / 2;
    const long long nblk = (n + MOM_ROWS - 1) / MOM_ROWS;
    if (blocks > 0x7fffffffll || nblk > 65535) return GZ_ERR_TOO_LARGE;
    double* partial = reinterpret_cast<double*>(workspace);
    const unsigned colblocks = (unsigned)((d + MOM_THREADS - 1) / MOM_THREADS);
    hipLaunchKernelGGL(moments_colsum_kernel, dim3(colblocks, (unsigned)nblk), dim3(MOM_THREADS), 0, stream, act, n, d,
                       partial);
    int rc = launch_status();
    if (rc != GZ_OK) return rc;
    hipLaunchKernelGGL(moments_mean_kernel, dim3(colblocks), dim3(MOM_THREADS), 0, stream, (const double*)partial,
                       (int)nblk, n, d, mean);
    rc = launch_status();
    if (rc != GZ_OK) return rc;
    hipLaunchKernelGGL(moments_tile_kernel, dim3((unsigned)blocks), dim3(MOM_THREADS), 0, stream, act, n, d, (int)tiles,
                       (const double*)mean, 1.0 / (double)(n - 1), cov);
    return launch_status();
}

}  // extern "C"
