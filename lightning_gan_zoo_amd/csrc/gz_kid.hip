// KID (reference core/callback_inception_metrics.py:15-133): everything `_mmd2_and_variance` reads of the three
// polynomial-kernel matrices of every subset, in fp64, without a kernel matrix ever existing in memory.
//
//     K_AB = (gamma * A B^T + coef0)^degree,   G = codes_g[idx[s][0]],   R = codes_r[idx[s][1]]      (rows gathered on load)
//
// One workgroup per (subset, product, band of 64 rows); the four products are GG, RR, GR and RG, the last one only for
// its row sums, which are the column sums of K_GR.  The workgroup walks every 64-column tile of its band, so each row
// sum, the band's diagonal and the band's share of the Frobenius sum finish inside it:
//   * wave w owns rows 16w .. 16w+15 of the band and four 16x16 accumulators (the tile's 64 columns) on
//     v_mfma_f64_16x16x4_f64, whose C/D layout is col = lane & 15, row = (lane >> 4) + 4 * reg;
//   * a lane adds the entries it holds to its four row accumulators tile after tile, 16-column block after block; at
//     the end the 16 lanes of a row are folded by an xor butterfly (8 after 4 after 2 after 1);
//   * the Frobenius share is summed per lane in the same order, folded over the wave by the xor butterfly, over the four
//     waves in wave order, and written to the workspace; a second, tiny launch adds the bands in band order.
// No floating-point atomics, no dependence on the previous content of `out` or the workspace: two calls give equal bits.
// Feature chunks of 32 travel global -> registers -> LDS one chunk ahead of the MFMAs; a lane's four MFMA k-slots of a
// chunk are (lane >> 4) * 8 + step, the same on both operands, so a dot product is summed in a fixed, permuted order.
// Tails: rows and columns >= m read row m-1 and are masked in the epilogue; features >= d are zero in LDS.
#include "gz_common.h"
#include "../../include/gz_ops.h"

namespace gz {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int KID_THREADS = 256;
constexpr int KID_BAND = 64;                 // rows per workgroup = columns per tile
constexpr int KID_KC = 32;                   // features per LDS chunk
constexpr int KID_LD = KID_KC + 2;           // LDS row stride in doubles: 16-byte aligned rows, 16 rows span all banks
constexpr int KID_LOADS = KID_BAND * KID_KC / KID_THREADS;      // doubles per thread, operand and chunk

__device__ __forceinline__ void kid_fetch(const double* __restrict__ codes, const long long (&off)[KID_LOADS], int k,
                                          int d, double (&v)[KID_LOADS]) {
#pragma unroll
    for (int i = 0; i < KID_LOADS; ++i) v[i] = k < d ? codes[off[i] + k] : 0.0;
}

__global__ __launch_bounds__(KID_THREADS) void kid_band_kernel(const double* __restrict__ codes_g,
                                                               const double* __restrict__ codes_r, int d,
                                                               const int* __restrict__ idx, int m, int nb, double gamma,
                                                               double coef0, int degree, double* __restrict__ out,
                                                               double* __restrict__ frob) {
    __shared__ __attribute__((aligned(16))) double sA[KID_BAND * KID_LD];
    __shared__ __attribute__((aligned(16))) double sB[KID_BAND * KID_LD];
    __shared__ int rowA[KID_BAND], rowB[KID_BAND];
    __shared__ double sF[KID_THREADS / 64];

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

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lk = tid & 31, lr = tid >> 5;              // loader: feature within the chunk, first of its 8 rows
    const int fr = lane & 15, fg = lane >> 4;            // MFMA fragment: row / column within the 16-block, k group

    if (tid < KID_BAND) rowA[tid] = ia[min(band * KID_BAND + tid, m - 1)];
    __syncthreads();
    long long offA[KID_LOADS], offB[KID_LOADS];
#pragma unroll
    for (int i = 0; i < KID_LOADS; ++i) offA[i] = (long long)rowA[lr + 8 * i] * d;

    double rs[4] = {0.0, 0.0, 0.0, 0.0};
    double fsum = 0.0;
    const int nchunks = (d + KID_KC - 1) / KID_KC;

    for (int ct = 0; ct < nb; ++ct) {
        __syncthreads();
        if (tid < KID_BAND) rowB[tid] = ib[min(ct * KID_BAND + tid, m - 1)];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KID_LOADS; ++i) offB[i] = (long long)rowB[lr + 8 * i] * d;

        f64x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
        double pa[KID_LOADS], pb[KID_LOADS];
        kid_fetch(A, offA, lk, d, pa);
        kid_fetch(B, offB, lk, d, pb);
        for (int c = 0; c < nchunks; ++c) {
            __syncthreads();                             // the previous chunk's readers are done with sA / sB
#pragma unroll
            for (int i = 0; i < KID_LOADS; ++i) {
                sA[(lr + 8 * i) * KID_LD + lk] = pa[i];
                sB[(lr + 8 * i) * KID_LD + lk] = pb[i];
            }
            __syncthreads();
            if (c + 1 < nchunks) {
                kid_fetch(A, offA, (c + 1) * KID_KC + lk, d, pa);
                kid_fetch(B, offB, (c + 1) * KID_KC + lk, d, pb);
            }
            const f64x2* qa = reinterpret_cast<const f64x2*>(&sA[(wave * 16 + fr) * KID_LD + fg * 8]);
            f64x2 a2[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) a2[h] = qa[h];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f64x2* qb = reinterpret_cast<const f64x2*>(&sB[(j * 16 + fr) * KID_LD + fg * 8]);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const f64x2 b2 = qb[h];
                    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[h][0], b2[0], acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[h][1], b2[1], acc[j], 0, 0, 0);
                }
            }
        }
        // epilogue of the tile: acc[j][r] is the dot product of band row wave*16 + fg + 4r and tile column j*16 + fr
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = ct * KID_BAND + j * 16 + fr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = band * KID_BAND + wave * 16 + fg + 4 * r;
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
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
        const int row = band * KID_BAND + wave * 16 + fg + 4 * r;
        if (fr == 0 && row < m) out_rows[row] = v;
    }
    if (p < 3) {                                          // (uniform over the workgroup)
        fsum = wave_sum_d(fsum);
        if (lane == 0) sF[wave] = fsum;
        __syncthreads();
        if (tid == 0) frob[((size_t)s * 3 + p) * nb + band] = ((sF[0] + sF[1]) + sF[2]) + sF[3];
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

inline int kid_bands(int m) { return (m + KID_BAND - 1) / KID_BAND; }

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
    hipLaunchKernelGGL(kid_band_kernel, dim3((unsigned)blocks), dim3(KID_THREADS), 0, stream, codes_g, codes_r, d, idx, m,
                       nb, gamma, coef0, degree, out, frob);
    const int rc = launch_status();
    if (rc != GZ_OK) return rc;
    hipLaunchKernelGGL(kid_finish_kernel, dim3(S), dim3(64), 0, stream, (const double*)frob, m, nb, out);
    return launch_status();
}

}  // extern "C"
