// KID (reference core/callback_inception_metrics.py:15-133): everything `_mmd2_and_variance` reads of the three
// polynomial-kernel matrices of every subset, in fp64, without a kernel matrix ever existing in memory.
//
//     K_AB = (gamma * A B^T + coef0)^degree,   G = codes_g[idx[s][0]],   R = codes_r[idx[s][1]]      (rows gathered on load)
//
// One workgroup per (subset, product, band of 64 rows); the four products are GG, RR, GR and RG, the last one only for
// its row sums, which are the column sums of K_GR.  The workgroup walks every 64-column tile of its band on the fp64
// tile core (gz_f64_tile.h: both operands [row][feature] images, the blocked k-slot map), so each row sum, the band's
// diagonal and the band's share of the Frobenius sum finish inside it:
//   * a lane adds the entries it holds to its four row accumulators tile after tile, 16-column block after block; at
//     the end the 16 lanes of a row are folded by an xor butterfly (8 after 4 after 2 after 1);
//   * the Frobenius share is summed per lane in the same order, folded over the workgroup in the core's fixed order and
//     written to the workspace; a second, tiny launch adds the bands in band order.
// No floating-point atomics, no dependence on the previous content of `out` or the workspace: two calls give equal bits.
// Tails: rows and columns >= m read row m-1 and are masked in the epilogue; features >= d are zero in LDS.
#include "gz_f64_tile.h"
#include "../../include/gz_ops.h"

namespace gz {

// features k of the thread's 8 gathered rows, zero from d on
__device__ __forceinline__ void kid_fetch(const double* __restrict__ codes, const long long (&off)[F64_LOADS], int k,
                                          int d, double (&v)[F64_LOADS]) {
#pragma unroll
    for (int i = 0; i < F64_LOADS; ++i) v[i] = k < d ? codes[off[i] + k] : 0.0;
}

__global__ __launch_bounds__(F64_THREADS) void kid_band_kernel(const double* __restrict__ codes_g,
                                                               const double* __restrict__ codes_r, int d,
                                                               const int* __restrict__ idx, int m, int nb, double gamma,
                                                               double coef0, int degree, double* __restrict__ out,
                                                               double* __restrict__ frob) {
    __shared__ __attribute__((aligned(16))) double sA[F64RowK::SIZE];
    __shared__ __attribute__((aligned(16))) double sB[F64RowK::SIZE];
    __shared__ int rowA[F64_TILE], rowB[F64_TILE];
    __shared__ double sF[F64_THREADS / 64];

    const int band = blockIdx.x % nb;
    const int p = (blockIdx.x / nb) & 3;                 // 0: GG, 1: RR, 2: GR, 3: RG
    const int s = blockIdx.x / (nb * 4);
    const int a_slot = (p == 1 || p == 3) ? 1 : 0, b_slot = (p == 1 || p == 2) ? 1 : 0;
    const double* __restrict__ A = a_slot ? codes_r : codes_g;
    const double* __restrict__ B = b_slot ? codes_r : codes_g;
    const int* ia = idx + ((size_t)s * 2 + a_slot) * m;
    const int* ib = idx + ((size_t)s * 2 + b_slot) * m;
    double* out_s = out + (size_t)s * (6 * (size_t)m + 3);
    double* out_rows = out_s + (size_t)(p == 0 ? 0 : p == 1 ? 2 : p == 2 ? 4 : 5) * m;
    double* out_diag = out_s + (size_t)(p == 0 ? 1 : 3) * m;       // (written for p < 2 only)

    const int tid = threadIdx.x;
    const int lk = F64RowK::own_k(tid, 0);               // loader: feature within the chunk

    if (tid < F64_TILE) rowA[tid] = ia[min(band * F64_TILE + tid, m - 1)];
    __syncthreads();
    long long offA[F64_LOADS], offB[F64_LOADS];
#pragma unroll
    for (int i = 0; i < F64_LOADS; ++i) offA[i] = (long long)rowA[F64RowK::own_index(tid, i)] * d;

    double rs[4] = {0.0, 0.0, 0.0, 0.0};
    double fsum = 0.0;
    const int nchunks = (d + F64_KC - 1) / F64_KC;

    for (int ct = 0; ct < nb; ++ct) {
        __syncthreads();
        if (tid < F64_TILE) rowB[tid] = ib[min(ct * F64_TILE + tid, m - 1)];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < F64_LOADS; ++i) offB[i] = (long long)rowB[F64RowK::own_index(tid, i)] * d;

        f64x4 acc[4];
        f64_tile_mainloop<F64RowK, F64RowK, F64SlotBlocked>(
            sA, sB, nchunks,
            [&](long long c, double (&v)[F64_LOADS]) { kid_fetch(A, offA, (int)c * F64_KC + lk, d, v); },
            [&](long long c, double (&v)[F64_LOADS]) { kid_fetch(B, offB, (int)c * F64_KC + lk, d, v); }, acc);
        // epilogue of the tile, j outer and r inner: the order of the row sums and of the Frobenius share
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = ct * F64_TILE + f64_acc_col(tid, j);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = band * F64_TILE + f64_acc_row(tid, r);
                const double t = gamma * acc[j][r] + coef0;
                double k = t;
                for (int q = 1; q < degree; ++q) k *= t;
                if (col < m) {
                    rs[r] += k;
                    if (row < m) {
                        fsum += k * k;
                        if (p < 2 && row == col) out_diag[row] = k;
                    }
                }
            }
        }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double v = rs[r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);      // a row's 16 columns sit in 16 consecutive lanes
        const int row = band * F64_TILE + f64_acc_row(tid, r);
        if (f64_acc_col(tid, 0) == 0 && row < m) out_rows[row] = v;
    }
    if (p < 3) {                                          // (uniform over the workgroup)
        fsum = f64_workgroup_sum(fsum, sF);
        if (tid == 0) frob[((size_t)s * 3 + p) * nb + band] = fsum;
    }
}

// the three Frobenius sums of a subset: its bands' shares in band order
__global__ __launch_bounds__(64) void kid_finish_kernel(const double* __restrict__ frob, int m, int nb,
                                                        double* __restrict__ out) {
    const int s = blockIdx.x, p = threadIdx.x;
    if (p >= 3) return;
    const double* f = frob + ((size_t)s * 3 + p) * nb;
    double v = 0.0;
    for (int b = 0; b < nb; ++b) v += f[b];
    out[(size_t)s * (6 * (size_t)m + 3) + 6 * (size_t)m + p] = v;
}

inline int kid_bands(int m) { return (m + F64_TILE - 1) / F64_TILE; }

}  // namespace gz

using namespace gz;

extern "C" {

size_t gz_kid_workspace_bytes(int S, int m, int d) {
    (void)d;
    if (S < 1 || m < 1) return 0;
    return (size_t)S * 3 * kid_bands(m) * sizeof(double);
}

int gz_kid_sums(const double* codes_g, int n_g, const double* codes_r, int n_r, int d, const int* idx, int S, int m,
                double gamma, double coef0, int degree, double* out, void* workspace, size_t ws_bytes,
                hipStream_t stream) {
    gz::clear_stale_error();
    if (S < 1 || m < 1 || d < 1 || degree < 1 || n_g < 1 || n_r < 1) return GZ_ERR_BAD_SHAPE;
    if (m > n_g || m > n_r) return GZ_ERR_BAD_SHAPE;
    if (!codes_g || !codes_r || !idx || !out || !workspace) return GZ_ERR_BAD_SHAPE;
    if (ws_bytes < gz_kid_workspace_bytes(S, m, d)) return GZ_ERR_WORKSPACE;
    const int nb = kid_bands(m);
    const long long blocks = (long long)S * 4 * nb;
    if (blocks > 0x7fffffffll) return GZ_ERR_TOO_LARGE;
    double* frob = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(kid_band_kernel, dim3((unsigned)blocks), dim3(F64_THREADS), 0, stream, codes_g, codes_r, d, idx, m,
                       nb, gamma, coef0, degree, out, frob);
    const int rc = launch_status();
    if (rc != GZ_OK) return rc;
    hipLaunchKernelGGL(kid_finish_kernel, dim3(S), dim3(64), 0, stream, (const double*)frob, m, nb, out);
    return launch_status();
}

}  // extern "C"
