// Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) from the fp64 codes the
// evaluation pass leaves on the device (eval.prdc_device).  Everything is decided on SQUARED Euclidean
// distances in the Gram form
//
//     D_ij = max(0, s_i + s_j - 2 <x_i, x_j>),   s_i = |x_i|^2
//
// whose 64 x 64 tiles come from the fp64 tile core (gz_f64_tile.h; both operands are [row][feature] images, F64RowK, the
// blocked k-slot map like KID's walk).  No distance matrix ever exists in memory.
//
//   prdc_sqnorm_kernel   s: one row per wave, lane l adds features l, l + 64, .. in order, then the xor butterfly.
//   knn_partial_kernel   gz_knn_radii.  A workgroup owns a band of 64 rows at a time and a slice of the column tiles.  A thread
//                        keeps the K smallest distances it has seen for each of its four accumulator rows as a sorted
//                        list in registers (one compare against the list's tail per entry once it is full); the diagonal
//                        j == i and the tail j >= n are skipped by INDEX.  At the end the 16 lanes that share a row merge
//                        by K rounds of a 16-lane minimum in which the lowest lane that holds the minimum pops its head.
//                        -> part[slice][row][K], ascending, +inf where a slice had fewer than K candidates.
//   knn_finish_kernel    the K-th smallest of a row's slices * K values.  Selection by value: the result does not depend
//                        on how the columns were sliced or walked, so it is the same bits for every slicing.
//   prdc_counts_kernel   gz_prdc_counts.  A workgroup owns a group of row tiles (generated rows) and a slice of column
//                        tiles (real rows) and computes each of its tiles once:
//                          row-wise     in_real[j] += #{i in tile : D_ji <= rad_r[i]}   in registers over the slice, folded
//                                       over the row's 16 lanes, stored to pr[slice][j];
//                          column-wise  in_fake[i] += #{j in tile : D_ji <= rad_g[j]},  near[i] = min_j D_ji: folded over
//                                       a wave's four k groups by shuffles, over the four waves through 3 KB of LDS, then
//                                       accumulated by thread i - col0 into pf / pn[group][i], which this workgroup alone
//                                       touches and writes (not adds) on its first row tile.
//   prdc_finish_kernel   in_real = sum over slices, in_fake = sum over groups, near = min over groups, in slice / group
//                        order, and each block's four integer totals -> the workspace; prdc_totals_kernel adds the
//                        blocks.  All counts are integers and near is a minimum: every fold is order-free.
// No floating-point atomics (no atomics at all), nothing read from an output or the workspace before this call wrote it:
// two calls give equal bits.  Tails: a row >= n or a feature >= d is never dereferenced and is zero in LDS; the epilogues
// mask by index.  Row offsets are 64-bit.
//
// Slicing (prdc_plan; gz_prdc_plan shows it): at most PRDC_MAX_GROUPS row groups of equal size up to one tile, so that
// the column-wise partials stay [groups][n_r] whatever n_g is; then as many column slices as fit with them into ONE round
// of PRDC_WG_PER_CU workgroups per CU of the budget (gz_set_cu_budget; what the registers allow), at most one per column
// tile.  gz_knn_radii takes the plan of (n, n): its workgroup walks the bands of its row group one after the other.
#include "gz_f64_tile.h"
#include "gz_knobs.h"
#include "../../include/gz_ops.h"

namespace gz {

constexpr int PRDC_MAX_K = 8;
constexpr int PRDC_MAX_GROUPS = 128;
constexpr int PRDC_WG_PER_CU = 2;
constexpr int PRDC_FINISH_THREADS = 256;

// the thread's 8 elements of chunk c of rows index0 .. of a row-major [count][d] operand, zero outside it
__device__ __forceinline__ void prdc_fetch(const double* __restrict__ a, long long count, int d, long long index0, int c,
                                           double (&v)[F64_LOADS]) {
    const int tid = threadIdx.x, k = c * F64_KC + F64RowK::own_k(tid, 0);
#pragma unroll
    for (int i = 0; i < F64_LOADS; ++i) {
        const long long index = index0 + F64RowK::own_index(tid, i);
        v[i] = (index < count && k < d) ? a[index * d + k] : 0.0;
    }
}

__global__ __launch_bounds__(F64_THREADS) void prdc_sqnorm_kernel(const double* __restrict__ codes, long long n, int d,
                                                                  double* __restrict__ sq) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (F64_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n) return;                                 // (a whole wave; no barrier below)
    const double* __restrict__ x = codes + row * d;
    double v = 0.0;
    for (int k = lane; k < d; k += 64) v += x[k] * x[k];
    v = wave_sum_d(v);
    if (lane == 0) sq[row] = v;
}

// the one expression of a squared distance, for radii and counts alike
__device__ __forceinline__ double prdc_dist(double s_row, double s_col, double dot) {
    return fmax(0.0, (s_row + s_col) - 2.0 * dot);
}

// v into the ascending list b if it is below its tail
template <int K>
__device__ __forceinline__ void prdc_insert(double (&b)[K], double v) {
    if (v < b[K - 1]) {
        b[K - 1] = v;
#pragma unroll
        for (int i = K - 1; i > 0; --i) {
            const double lo = fmin(b[i - 1], b[i]), hi = fmax(b[i - 1], b[i]);
            b[i - 1] = lo;
            b[i] = hi;
        }
    }
}

// tiles [first, last) of slice `part` of `parts` over `tiles` tiles (parts <= tiles: never empty)
__device__ __forceinline__ void prdc_slice(long long tiles, int parts, int part, long long& first, long long& last) {
    first = tiles * part / parts;
    last = tiles * (part + 1) / parts;
}

template <int K>
__global__ __launch_bounds__(F64_THREADS) void knn_partial_kernel(const double* __restrict__ codes, long long n, int d,
                                                                  const double* __restrict__ sq, int groups,
                                                                  int slices, long long tiles,
                                                                  double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double sA[F64RowK::SIZE];
    __shared__ __attribute__((aligned(16))) double sB[F64RowK::SIZE];

    const int tid = threadIdx.x, fr = tid & 15;
    const int g = (int)(blockIdx.x / (unsigned)slices), sl = (int)(blockIdx.x % (unsigned)slices);
    long long b0, b1, t0, t1;
    prdc_slice(tiles, groups, g, b0, b1);
    prdc_slice(tiles, slices, sl, t0, t1);
    const int nchunks = (d + F64_KC - 1) / F64_KC;

    for (long long band = b0; band < b1; ++band) {
        const long long row0 = band * F64_TILE;
        long long rows[4];
        double srow[4], best[4][K];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rows[r] = row0 + f64_acc_row(tid, r);
            srow[r] = rows[r] < n ? sq[rows[r]] : 0.0;
#pragma unroll
            for (int i = 0; i < K; ++i) best[r][i] = INFINITY;
        }
        for (long long t = t0; t < t1; ++t) {
            const long long col0 = t * F64_TILE;
            f64x4 acc[4];
            f64_tile_mainloop<F64RowK, F64RowK, F64SlotBlocked>(
                sA, sB, nchunks, [&](long long c, double (&v)[F64_LOADS]) { prdc_fetch(codes, n, d, row0, (int)c, v); },
                [&](long long c, double (&v)[F64_LOADS]) { prdc_fetch(codes, n, d, col0, (int)c, v); }, acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long col = col0 + f64_acc_col(tid, j);
                const double scol = col < n ? sq[col] : 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col < n && col != rows[r]) prdc_insert<K>(best[r], prdc_dist(srow[r], scol, acc[j][r]));
            }
        }
        // a row's 16 columns sit in 16 consecutive lanes: K rounds of their minimum, the lowest lane that holds it pops
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const double head = best[r][0];
                double m = head;
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) m = fmin(m, __shfl_xor(m, o, 64));
                int who = head == m ? fr : 16;
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) who = min(who, __shfl_xor(who, o, 64));
                if (fr == who) {
#pragma unroll
                    for (int i = 0; i + 1 < K; ++i) best[r][i] = best[r][i + 1];
                    best[r][K - 1] = INFINITY;
                }
                if (fr == 0 && rows[r] < n) part[((size_t)sl * (size_t)n + (size_t)rows[r]) * K + t] = m;
            }
        }
    }
}

template <int K>
__global__ __launch_bounds__(PRDC_FINISH_THREADS) void knn_finish_kernel(const double* __restrict__ part, long long n,
                                                                         int slices, double* __restrict__ radii) {
    const long long row = (long long)blockIdx.x * PRDC_FINISH_THREADS + threadIdx.x;
    if (row >= n) return;
    double b[K];
#pragma unroll
    for (int i = 0; i < K; ++i) b[i] = INFINITY;
    for (int sl = 0; sl < slices; ++sl) {
        const double* __restrict__ p = part + ((size_t)sl * (size_t)n + (size_t)row) * K;
#pragma unroll
        for (int t = 0; t < K; ++t) prdc_insert<K>(b, p[t]);
    }
    radii[row] = b[K - 1];
}

__global__ __launch_bounds__(F64_THREADS) void prdc_counts_kernel(
    const double* __restrict__ codes_g, long long n_g, const double* __restrict__ rad_g, const double* __restrict__ sq_g,
    const double* __restrict__ codes_r, long long n_r, const double* __restrict__ rad_r, const double* __restrict__ sq_r,
    int d, int groups, int slices, long long rtiles, long long ctiles, int* pr, int* pf, double* pn) {
    __shared__ __attribute__((aligned(16))) double sA[F64RowK::SIZE];
    __shared__ __attribute__((aligned(16))) double sB[F64RowK::SIZE];
    __shared__ int sC[F64_THREADS / 64][F64_TILE];
    __shared__ double sN[F64_THREADS / 64][F64_TILE];

    const int tid = threadIdx.x, wave = tid >> 6, fr = tid & 15, fg = (tid & 63) >> 4;
    const int g = (int)(blockIdx.x / (unsigned)slices), sl = (int)(blockIdx.x % (unsigned)slices);
    long long rt0, rt1, ct0, ct1;
    prdc_slice(rtiles, groups, g, rt0, rt1);
    prdc_slice(ctiles, slices, sl, ct0, ct1);
    const int nchunks = (d + F64_KC - 1) / F64_KC;

    for (long long rt = rt0; rt < rt1; ++rt) {
        const long long row0 = rt * F64_TILE;
        long long rows[4];
        double srow[4], rg[4];
        int cr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rows[r] = row0 + f64_acc_row(tid, r);
            const bool in = rows[r] < n_g;
            srow[r] = in ? sq_g[rows[r]] : 0.0;
            rg[r] = in ? rad_g[rows[r]] : 0.0;
            cr[r] = 0;
        }
        for (long long ct = ct0; ct < ct1; ++ct) {
            const long long col0 = ct * F64_TILE;
            f64x4 acc[4];
            f64_tile_mainloop<F64RowK, F64RowK, F64SlotBlocked>(
                sA, sB, nchunks,
                [&](long long c, double (&v)[F64_LOADS]) { prdc_fetch(codes_g, n_g, d, row0, (int)c, v); },
                [&](long long c, double (&v)[F64_LOADS]) { prdc_fetch(codes_r, n_r, d, col0, (int)c, v); }, acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long col = col0 + f64_acc_col(tid, j);
                const bool cin = col < n_r;
                const double scol = cin ? sq_r[col] : 0.0, rr = cin ? rad_r[col] : 0.0;
                int cc = 0;
                double nn = INFINITY;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double dist = prdc_dist(srow[r], scol, acc[j][r]);
                    if (cin && rows[r] < n_g) {
                        cr[r] += dist <= rr ? 1 : 0;
                        cc += dist <= rg[r] ? 1 : 0;
                        nn = fmin(nn, dist);
                    }
                }
                // a column's 16 rows of this wave: 4 registers (above) times the 4 k groups, 16 and 32 lanes apart
                cc += __shfl_xor(cc, 16, 64);
                nn = fmin(nn, __shfl_xor(nn, 16, 64));
                cc += __shfl_xor(cc, 32, 64);
                nn = fmin(nn, __shfl_xor(nn, 32, 64));
                if (fg == 0) {
                    sC[wave][16 * j + fr] = cc;
                    sN[wave][16 * j + fr] = nn;
                }
            }
            __syncthreads();        // (the next tile writes sC / sN after its main loop's barriers: behind these reads)
            if (tid < F64_TILE && col0 + tid < n_r) {
                int c = ((sC[0][tid] + sC[1][tid]) + sC[2][tid]) + sC[3][tid];
                double m = fmin(fmin(sN[0][tid], sN[1][tid]), fmin(sN[2][tid], sN[3][tid]));
                const size_t at = (size_t)g * (size_t)n_r + (size_t)(col0 + tid);
                if (rt != rt0) {    // this thread wrote it on the row tile before
                    c += pf[at];
                    m = fmin(m, pn[at]);
                }
                pf[at] = c;
                pn[at] = m;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int v = cr[r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
            if (fr == 0 && rows[r] < n_g) pr[(size_t)sl * (size_t)n_g + (size_t)rows[r]] = v;
        }
    }
}

// thread t: generated row t and real row t.  block totals: #in_real > 0, #in_fake > 0, sum in_real, #near <= rad_r
__global__ __launch_bounds__(PRDC_FINISH_THREADS) void prdc_finish_kernel(
    const int* __restrict__ pr, const int* __restrict__ pf, const double* __restrict__ pn,
    const double* __restrict__ rad_r, long long n_g, long long n_r, int groups, int slices, int* __restrict__ in_real,
    int* __restrict__ in_fake, double* __restrict__ near, long long* __restrict__ blocktot) {
    __shared__ long long sT[PRDC_FINISH_THREADS / 64][4];
    const long long t = (long long)blockIdx.x * PRDC_FINISH_THREADS + threadIdx.x;
    long long tot[4] = {0, 0, 0, 0};
    if (t < n_g) {
        int c = 0;
        for (int s = 0; s < slices; ++s) c += pr[(size_t)s * (size_t)n_g + (size_t)t];
        in_real[t] = c;
        tot[0] = c > 0;
        tot[2] = c;
    }
    if (t < n_r) {
        int c = 0;
        double m = INFINITY;
        for (int g = 0; g < groups; ++g) {
            c += pf[(size_t)g * (size_t)n_r + (size_t)t];
            m = fmin(m, pn[(size_t)g * (size_t)n_r + (size_t)t]);
        }
        in_fake[t] = c;
        near[t] = m;
        tot[1] = c > 0;
        tot[3] = m <= rad_r[t];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot[q] += __shfl_xor(tot[q], o, 64);
        if ((threadIdx.x & 63) == 0) sT[threadIdx.x >> 6][q] = tot[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        long long v = 0;
        for (int w = 0; w < PRDC_FINISH_THREADS / 64; ++w) v += sT[w][threadIdx.x];
        blocktot[(size_t)blockIdx.x * 4 + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void prdc_totals_kernel(const long long* __restrict__ blocktot, long long blocks,
                                                         long long* __restrict__ totals) {
    const int q = threadIdx.x & 3;
    long long v = 0;
    for (long long b = threadIdx.x >> 2; b < blocks; b += 16) v += blocktot[b * 4 + q];
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    if (threadIdx.x < 4) totals[q] = v;
}

inline long long prdc_tiles(long long n) { return n / F64_TILE + (n % F64_TILE != 0); }

// the column slices that fit beside `groups` row groups into one round of PRDC_WG_PER_CU workgroups per CU (a grid just
// above a round would run a second, nearly empty one), at most one per column tile
inline int prdc_col_slices(long long groups, long long ctiles) {
    const long long target = (long long)PRDC_WG_PER_CU * cus();
    long long s = target / groups;
    if (s > ctiles) s = ctiles;
    return (int)(s < 1 ? 1 : s);
}

inline void prdc_plan(long long n_rows, long long n_cols, int& groups, int& slices) {
    const long long rt = prdc_tiles(n_rows), ct = prdc_tiles(n_cols);
    const long long cap = rt < PRDC_MAX_GROUPS ? rt : PRDC_MAX_GROUPS;
    const long long per = (rt + cap - 1) / cap;           // row tiles per group, the last groups one fewer
    groups = (int)((rt + per - 1) / per);
    slices = prdc_col_slices(groups, ct);
}

inline bool prdc_fits(unsigned __int128 bytes) { return bytes <= (unsigned __int128)PTRDIFF_MAX; }

// gz_knn_radii's workspace in doubles: sq [n] | part [slices][n][k]
struct KnnPlan {
    long long tiles;
    int groups, slices;
    size_t part, total;
};
inline bool knn_plan(long long n, int d, int k, KnnPlan& p) {
    if (!prdc_fits((unsigned __int128)n * (unsigned)d * sizeof(double))) return false;
    p.tiles = prdc_tiles(n);
    prdc_plan(n, n, p.groups, p.slices);
    const unsigned __int128 total = (unsigned __int128)n + (unsigned __int128)n * p.slices * k;
    if (!prdc_fits(total * sizeof(double))) return false;
    p.part = (size_t)n;
    p.total = (size_t)total;
    return true;
}

// gz_prdc_counts' workspace in bytes: sq_g [n_g] | sq_r [n_r] | pn [groups][n_r] doubles | blocktot [blocks][4] int64 |
// pr [slices][n_g] | pf [groups][n_r] int32
struct CountsPlan {
    long long rtiles, ctiles, blocks;
    int groups, slices;
    size_t sq_r, pn, blocktot, pr, pf, total;             // byte offsets, and the size
};
inline bool counts_plan(long long n_g, long long n_r, int d, CountsPlan& p) {
    if (!prdc_fits((unsigned __int128)n_g * (unsigned)d * sizeof(double)) ||
        !prdc_fits((unsigned __int128)n_r * (unsigned)d * sizeof(double)))
        return false;
    p.rtiles = prdc_tiles(n_g);
    p.ctiles = prdc_tiles(n_r);
    prdc_plan(n_g, n_r, p.groups, p.slices);
    const long long rows = n_g > n_r ? n_g : n_r;
    p.blocks = rows / PRDC_FINISH_THREADS + (rows % PRDC_FINISH_THREADS != 0);
    if (p.blocks > 0x7fffffffll || (n_g + 3) / 4 > 0x7fffffffll || (n_r + 3) / 4 > 0x7fffffffll) return false;
    unsigned __int128 at = (unsigned __int128)n_g * 8;
    const unsigned __int128 sq_r = at;
    at += (unsigned __int128)n_r * 8;
    const unsigned __int128 pn = at;
    at += (unsigned __int128)p.groups * n_r * 8;
    const unsigned __int128 blocktot = at;
    at += (unsigned __int128)p.blocks * 4 * 8;
    const unsigned __int128 pr = at;
    at += (unsigned __int128)p.slices * n_g * 4;
    const unsigned __int128 pf = at;
    at += (unsigned __int128)p.groups * n_r * 4;
    at = (at + 7) / 8 * 8;
    if (!prdc_fits(at)) return false;
    p.sq_r = (size_t)sq_r;
    p.pn = (size_t)pn;
    p.blocktot = (size_t)blocktot;
    p.pr = (size_t)pr;
    p.pf = (size_t)pf;
    p.total = (size_t)at;
    return true;
}

inline int prdc_sqnorm(const double* codes, long long n, int d, double* sq, hipStream_t stream) {
    hipLaunchKernelGGL(prdc_sqnorm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(F64_THREADS), 0, stream, codes, n, d, sq);
    return launch_status();
}

template <int K>
inline int knn_launch(const double* codes, long long n, int d, const KnnPlan& p, const double* sq, double* part,
                      double* radii, hipStream_t stream) {
    hipLaunchKernelGGL(knn_partial_kernel<K>, dim3((unsigned)(p.groups * p.slices)), dim3(F64_THREADS), 0, stream, codes, n,
                       d, sq, p.groups, p.slices, p.tiles, part);
    const int rc = launch_status();
    if (rc != GZ_OK) return rc;
    const long long blocks = n / PRDC_FINISH_THREADS + (n % PRDC_FINISH_THREADS != 0);
    hipLaunchKernelGGL(knn_finish_kernel<K>, dim3((unsigned)blocks), dim3(PRDC_FINISH_THREADS), 0, stream,
                       (const double*)part, n, p.slices, radii);
    return launch_status();
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_prdc_plan(long long n_rows, long long n_cols, int* row_groups, int* col_slices) {
    if (n_rows < 1 || n_cols < 1 || !row_groups || !col_slices) return GZ_ERR_BAD_SHAPE;
    prdc_plan(n_rows, n_cols, *row_groups, *col_slices);
    return GZ_OK;
}

size_t gz_knn_radii_workspace_bytes(long long n, int d, int k) {
    KnnPlan p;
    if (k < 1 || k > PRDC_MAX_K || k >= n || d < 1 || !knn_plan(n, d, k, p)) return 0;
    return p.total * sizeof(double);
}

int gz_knn_radii(const double* codes, long long n, int d, int k, double* radii, void* workspace, size_t ws_bytes,
                 hipStream_t stream) {
    gz::clear_stale_error();
    if (k < 1 || k > PRDC_MAX_K || k >= n || d < 1 || !codes || !radii || !workspace) return GZ_ERR_BAD_SHAPE;
    KnnPlan p;
    if (!knn_plan(n, d, k, p) || (n + 3) / 4 > 0x7fffffffll) return GZ_ERR_TOO_LARGE;
    if (ws_bytes < p.total * sizeof(double)) return GZ_ERR_WORKSPACE;
    double* sq = reinterpret_cast<double*>(workspace);
    double* part = sq + p.part;
    const int rc = prdc_sqnorm(codes, n, d, sq, stream);
    if (rc != GZ_OK) return rc;
    switch (k) {
        case 1: return knn_launch<1>(codes, n, d, p, sq, part, radii, stream);
        case 2: return knn_launch<2>(codes, n, d, p, sq, part, radii, stream);
        case 3: return knn_launch<3>(codes, n, d, p, sq, part, radii, stream);
        case 4: return knn_launch<4>(codes, n, d, p, sq, part, radii, stream);
        case 5: return knn_launch<5>(codes, n, d, p, sq, part, radii, stream);
        case 6: return knn_launch<6>(codes, n, d, p, sq, part, radii, stream);
        case 7: return knn_launch<7>(codes, n, d, p, sq, part, radii, stream);
        default: return knn_launch<8>(codes, n, d, p, sq, part, radii, stream);
    }
}

size_t gz_prdc_counts_workspace_bytes(long long n_g, long long n_r, int d) {
    CountsPlan p;
    if (n_g < 1 || n_r < 1 || d < 1 || !counts_plan(n_g, n_r, d, p)) return 0;
    return p.total;
}

int gz_prdc_counts(const double* codes_g, long long n_g, const double* rad_g, const double* codes_r, long long n_r,
                   const double* rad_r, int d, int* in_real, int* in_fake, double* near, long long* totals,
                   void* workspace, size_t ws_bytes, hipStream_t stream) {
    gz::clear_stale_error();
    if (n_g < 1 || n_r < 1 || d < 1) return GZ_ERR_BAD_SHAPE;
    if (!codes_g || !rad_g || !codes_r || !rad_r || !in_real || !in_fake || !near || !totals || !workspace)
        return GZ_ERR_BAD_SHAPE;
    CountsPlan p;
    if (!counts_plan(n_g, n_r, d, p)) return GZ_ERR_TOO_LARGE;
    if (ws_bytes < p.total) return GZ_ERR_WORKSPACE;
    char* ws = reinterpret_cast<char*>(workspace);
    double *sq_g = reinterpret_cast<double*>(ws), *sq_r = reinterpret_cast<double*>(ws + p.sq_r);
    double* pn = reinterpret_cast<double*>(ws + p.pn);
    long long* blocktot = reinterpret_cast<long long*>(ws + p.blocktot);
    int *pr = reinterpret_cast<int*>(ws + p.pr), *pf = reinterpret_cast<int*>(ws + p.pf);
    int rc;
    if ((rc = prdc_sqnorm(codes_g, n_g, d, sq_g, stream)) != GZ_OK) return rc;
    if ((rc = prdc_sqnorm(codes_r, n_r, d, sq_r, stream)) != GZ_OK) return rc;
    hipLaunchKernelGGL(prdc_counts_kernel, dim3((unsigned)(p.groups * p.slices)), dim3(F64_THREADS), 0, stream, codes_g,
                       n_g, rad_g, (const double*)sq_g, codes_r, n_r, rad_r, (const double*)sq_r, d, p.groups, p.slices,
                       p.rtiles, p.ctiles, pr, pf, pn);
    if ((rc = launch_status()) != GZ_OK) return rc;
    hipLaunchKernelGGL(prdc_finish_kernel, dim3((unsigned)p.blocks), dim3(PRDC_FINISH_THREADS), 0, stream, (const int*)pr,
                       (const int*)pf, (const double*)pn, rad_r, n_g, n_r, p.groups, p.slices, in_real, in_fake, near,
                       blocktot);
    if ((rc = launch_status()) != GZ_OK) return rc;
    hipLaunchKernelGGL(prdc_totals_kernel, dim3(1), dim3(64), 0, stream, (const long long*)blocktot, p.blocks, totals);
    return launch_status();
}

}  // extern "C"
