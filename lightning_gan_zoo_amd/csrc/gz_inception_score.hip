// Inception Score on the device from the classifier head of the FID network (eval.inception_score_device; DESIGN.md
// 3.4.8), in fp64: the statistic of the reference's core/submodules/gan_stability/metrics/inception_score.py -- softmax
// over all classes, contiguous splits of n / splits rows, entropy(p_i, p_y) per row, exp(mean) per split -- on
//
//     logits = codes W^T + b                  gz_classifier_logits: a non-square product on v_mfma_f64_16x16x4_f64
//     scores[s] = exp(mean_i KL(p_i || py))   gz_inception_score: fixed-order reductions
//
// Product: one workgroup per 64 x 64 tile of logits, the whole reduction index inside it, on the fp64 tile core
// (gz_f64_tile.h).  codes [n][d] and weight [classes][d] (nn.Linear's layout) both have the reduction index contiguous
// in memory, so both LDS images are the [index][k] form (F64RowK): half a wave loads 256 contiguous bytes of one row.
//   * slot map: F64SlotInterleaved, k = 4 s + (lane >> 4).  It is the map under which an entry is summed over k in k
//     order (four at a time inside an MFMA), which this product promises, and on the [index][k] image its fragment read
//     is 8 bytes per lane whose 32-lane halves touch all 64 banks once (pitch 68 dwords = 4 mod 64; the derivation is in
//     gz_f64_tile.h): conflict-free as ds_read_b64, which moves as many bytes per LDS cycle as ds_read_b128.  The blocked
//     map (KID's) would trade that for a quarter of the read instructions and sum k = 0, 8, 16, 24 first: not k order.
//     (The compiler pairs most of these reads, steps s and s + 1 of one row, into ds_read2_b64: 20 of them and 6
//     ds_read_b128 per 32 MFMAs, the mix it makes of sqrtm_product_kernel's [row][k] operand)
//   * tails: a row >= n, a class >= classes or a reduction index >= d is never dereferenced and is zero in LDS, so
//     n, d and classes need no multiple of anything; the epilogue stores only rows < n and classes < classes;
//   * tiles are numbered with the class tile fastest: workgroups that run together share a row tile of codes, the
//     large operand, and the weight matrix stays in cache;
//   * epilogue: acc + bias[class] (bias may be null), the 16 lanes of a row write 128 contiguous bytes.
//
// Score, over the first m * splits rows (m = n / splits; the trailing n % splits rows are ignored like the
// reference's), five launches:
//   1. is_rowstat_kernel   per row the maximum M_i and Z_i = sum_c exp(l_ic - M_i): a workgroup walks IS_ROWS rows, a
//                          thread its classes tid, tid + 256, .. in order, then f64_workgroup_sum -> rowstat[row][2];
//   2. is_colsum_kernel    p_ic = exp(l_ic - M_i) / Z_i summed over the IS_ROWS rows of one block of one split, a
//                          thread per class, rows in order -> colpart[split][block][class].  A block never spans two
//                          splits;
//   3. is_logpy_kernel     py_c = (sum over the blocks in block order) / m -> logpy[split][class] = log py_c;
//   4. is_kl_kernel        sum over a block's rows and classes of p_ic (log p_ic - log py_c), p_ic = 0 contributing 0
//                          like scipy's rel_entr: a thread walks rows in order and its classes in order, then
//                          f64_workgroup_sum -> klpart[split][block];
//   5. is_finish_kernel    scores[split] = exp((sum over the blocks in block order) / m).
// The KL term is taken directly, not through the entropy identity: p_ic and py_c go through the same log(), so a split
// of one row (py = p) scores exactly 1.  No row is kept in LDS: classes has no cap.  Logits of +-800 give exp(-1600) =
// 0, p = 0, no NaN.
// No floating-point atomics, a fixed order for every sum, nothing read from scores or the workspace before this call
// wrote it: two calls give equal bits.
#include "gz_f64_tile.h"
#include "../../include/gz_ops.h"

namespace gz {

constexpr int IS_THREADS = F64_THREADS;
constexpr int IS_ROWS = 64;                   // rows per workgroup of the reductions

// the thread's 8 elements of chunk c of rows index0 .. of a row-major [count][d] operand, zero outside it
__device__ __forceinline__ void is_fetch(const double* __restrict__ a, long long count, int d, long long index0, int c,
                                         double (&v)[F64_LOADS]) {
    const int tid = threadIdx.x, k = c * F64_KC + F64RowK::own_k(tid, 0);
#pragma unroll
    for (int i = 0; i < F64_LOADS; ++i) {
        const long long index = index0 + F64RowK::own_index(tid, i);
        v[i] = (index < count && k < d) ? a[index * d + k] : 0.0;
    }
}

__global__ __launch_bounds__(IS_THREADS) void classifier_logits_kernel(const double* __restrict__ codes, long long n,
                                                                       int d, const double* __restrict__ weight,
                                                                       const double* __restrict__ bias, int classes,
                                                                       double* __restrict__ logits, int ctiles) {
    __shared__ __attribute__((aligned(16))) double sA[F64RowK::SIZE];
    __shared__ __attribute__((aligned(16))) double sB[F64RowK::SIZE];

    const int tid = threadIdx.x;
    const long long row0 = (long long)(blockIdx.x / (unsigned)ctiles) * F64_TILE;
    const int col0 = (int)(blockIdx.x % (unsigned)ctiles) * F64_TILE;

    f64x4 acc[4];
    f64_tile_mainloop<F64RowK, F64RowK, F64SlotInterleaved>(
        sA, sB, (d + F64_KC - 1) / F64_KC,
        [&](long long c, double (&v)[F64_LOADS]) { is_fetch(codes, n, d, row0, (int)c, v); },
        [&](long long c, double (&v)[F64_LOADS]) { is_fetch(weight, classes, d, col0, (int)c, v); }, acc);

    // acc[j][r] is the dot product of row row0 + f64_acc_row(r) of codes and row col0 + f64_acc_col(j) of weight
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + f64_acc_col(tid, j);
        const double b = (bias && col < classes) ? bias[col] : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long row = row0 + f64_acc_row(tid, r);
            if (row < n && col < classes) logits[row * classes + col] = acc[j][r] + b;
        }
    }
}

// Maximum of v over the workgroup (f64_workgroup_sum's shape).  sW: IS_THREADS / 64 doubles of this maximum's own.
__device__ __forceinline__ double is_workgroup_max(double v, double* sW) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(sW[0], sW[1]), fmax(sW[2], sW[3]));
}

// the one expression of a softmax entry, for the column sums and the KL terms alike (equal bits in both)
__device__ __forceinline__ double is_softmax(double l, double mx, double z) { return exp(l - mx) / z; }

// The reductions' blocks: split s is rows s m .. (s + 1) m - 1, cut into nblk blocks of IS_ROWS rows (the last one
// shorter); workgroup id -> split id / nblk, block id % nblk.
struct IsBlock {
    long long row0;
    int rows;
};
__device__ __forceinline__ IsBlock is_block(long long id, long long m, long long nblk) {
    const long long s = id / nblk, b = id % nblk;
    const long long left = m - b * IS_ROWS;
    return IsBlock{s * m + b * IS_ROWS, (int)(left < IS_ROWS ? left : IS_ROWS)};
}

__global__ __launch_bounds__(IS_THREADS) void is_rowstat_kernel(const double* __restrict__ logits, long long rows,
                                                                int classes, double* __restrict__ rowstat) {
    __shared__ double sM[IS_THREADS / 64], sZ[IS_THREADS / 64];
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * IS_ROWS;
    const long long r1 = r0 + IS_ROWS < rows ? r0 + IS_ROWS : rows;
    // (the barriers of one row's two folds separate the next row's writes of sM / sZ from this row's reads)
    for (long long row = r0; row < r1; ++row) {
        const double* __restrict__ l = logits + row * classes;
        double mx = -INFINITY;
        for (int c = tid; c < classes; c += IS_THREADS) mx = fmax(mx, l[c]);
        mx = is_workgroup_max(mx, sM);
        double z = 0.0;
        for (int c = tid; c < classes; c += IS_THREADS) z += exp(l[c] - mx);
        z = f64_workgroup_sum(z, sZ);
        if (tid == 0) {
            rowstat[2 * row] = mx;
            rowstat[2 * row + 1] = z;
        }
    }
}

// workgroup = (split, block, 256 classes): colpart[split][block][class] = sum of p over the block's rows, in row order
__global__ __launch_bounds__(IS_THREADS) void is_colsum_kernel(const double* __restrict__ logits, int classes,
                                                               long long m, long long nblk, int cblocks,
                                                               const double* __restrict__ rowstat,
                                                               double* __restrict__ colpart) {
    const long long id = (long long)(blockIdx.x / (unsigned)cblocks);
    const int c = (int)(blockIdx.x % (unsigned)cblocks) * IS_THREADS + (int)threadIdx.x;
    if (c >= classes) return;
    const IsBlock blk = is_block(id, m, nblk);
    double sum = 0.0;
    for (int i = 0; i < blk.rows; ++i) {
        const long long row = blk.row0 + i;
        sum += is_softmax(logits[row * classes + c], rowstat[2 * row], rowstat[2 * row + 1]);
    }
    colpart[id * classes + c] = sum;
}

// thread = (split, class): logpy[split][class] = log(sum of the split's blocks in block order / m)
__global__ __launch_bounds__(IS_THREADS) void is_logpy_kernel(const double* __restrict__ colpart, int classes,
                                                              long long m, long long nblk, int cblocks,
                                                              double* __restrict__ logpy) {
    const long long s = (long long)(blockIdx.x / (unsigned)cblocks);
    const int c = (int)(blockIdx.x % (unsigned)cblocks) * IS_THREADS + (int)threadIdx.x;
    if (c >= classes) return;
    double sum = 0.0;
    for (long long b = 0; b < nblk; ++b) sum += colpart[(s * nblk + b) * classes + c];
    logpy[s * classes + c] = log(sum / (double)m);
}

// workgroup = (split, block): klpart[split][block] = sum over the block of p (log p - log py)
__global__ __launch_bounds__(IS_THREADS) void is_kl_kernel(const double* __restrict__ logits, int classes, long long m,
                                                           long long nblk, const double* __restrict__ rowstat,
                                                           const double* __restrict__ logpy,
                                                           double* __restrict__ klpart) {
    __shared__ double sK[IS_THREADS / 64];
    const int tid = threadIdx.x;
    const long long id = blockIdx.x;
    const IsBlock blk = is_block(id, m, nblk);
    const double* __restrict__ lp = logpy + (id / nblk) * classes;
    double kl = 0.0;
    for (int i = 0; i < blk.rows; ++i) {
        const long long row = blk.row0 + i;
        const double mx = rowstat[2 * row], z = rowstat[2 * row + 1];
        for (int c = tid; c < classes; c += IS_THREADS) {
            const double p = is_softmax(logits[row * classes + c], mx, z);
            if (p > 0.0) kl += p * (log(p) - lp[c]);
        }
    }
    kl = f64_workgroup_sum(kl, sK);
    if (tid == 0) klpart[id] = kl;
}

__global__ __launch_bounds__(64) void is_finish_kernel(const double* __restrict__ klpart, long long m, long long nblk,
                                                       int splits, double* __restrict__ scores) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= splits) return;
    double sum = 0.0;
    for (long long b = 0; b < nblk; ++b) sum += klpart[(long long)s * nblk + b];
    scores[s] = exp(sum / (double)m);
}

// [p, p + count doubles) and [q, q + qcount doubles) share a byte
inline bool is_overlap(const double* p, size_t count, const double* q, size_t qcount) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)qcount * sizeof(double) && b < a + (uintptr_t)count * sizeof(double);
}

// rows * cols doubles is a size a pointer can span
inline bool is_addressable(long long rows, long long cols) {
    return (unsigned __int128)rows * (unsigned __int128)cols * sizeof(double) <= (unsigned __int128)PTRDIFF_MAX;
}

// The workspace in doubles: rowstat [m splits][2] | colpart [splits][nblk][classes] | logpy [splits][classes] |
// klpart [splits][nblk].  -> false when a count leaves 64 bits or a grid leaves int.
struct IsPlan {
    long long m, nblk, rows, cblocks;
    size_t rowstat, colpart, logpy, klpart, total;      // offsets in doubles, and the size
};
inline bool is_plan(long long n, int classes, int splits, IsPlan& p) {
    if (!is_addressable(n, classes)) return false;      // (n < 2^60 from here on)
    p.m = n / splits;
    p.rows = p.m * splits;
    p.nblk = (p.m + IS_ROWS - 1) / IS_ROWS;
    p.cblocks = ((long long)classes + IS_THREADS - 1) / IS_THREADS;
    const unsigned __int128 groups = (unsigned __int128)splits * p.nblk;           // (split, block) pairs
    if (groups * p.cblocks > 0x7fffffffull) return false;
    if ((p.rows + IS_ROWS - 1) / IS_ROWS > 0x7fffffffll) return false;
    const unsigned __int128 total = (unsigned __int128)p.rows * 2 + groups * classes + (unsigned __int128)splits * classes
                                    + groups;
    if (total * sizeof(double) > (unsigned __int128)PTRDIFF_MAX) return false;
    p.rowstat = 0;
    p.colpart = (size_t)p.rows * 2;
    p.logpy = p.colpart + (size_t)groups * classes;
    p.klpart = p.logpy + (size_t)splits * classes;
    p.total = (size_t)total;
    return true;
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_classifier_logits(const double* codes, long long n, int d, const double* weight, const double* bias,
                         int classes, double* logits, hipStream_t stream) {
    gz::clear_stale_error();
    if (n < 1 || d < 1 || classes < 1 || !codes || !weight || !logits) return GZ_ERR_BAD_SHAPE;
    const long long rtiles = n / F64_TILE + (n % F64_TILE != 0);
    const long long ctiles = ((long long)classes + F64_TILE - 1) / F64_TILE;
    if ((unsigned __int128)rtiles * ctiles > 0x7fffffffull) return GZ_ERR_TOO_LARGE;
    if (!is_addressable(n, d) || !is_addressable(n, classes)) return GZ_ERR_TOO_LARGE;
    const size_t out = (size_t)n * (size_t)classes;
    if (is_overlap(logits, out, codes, (size_t)n * (size_t)d) ||
        is_overlap(logits, out, weight, (size_t)classes * (size_t)d))
        return GZ_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(classifier_logits_kernel, dim3((unsigned)(rtiles * ctiles)), dim3(IS_THREADS), 0, stream, codes, n,
                       d, weight, bias, classes, logits, (int)ctiles);
    return launch_status();
}

size_t gz_inception_score_workspace_bytes(long long n, int classes, int splits) {
    IsPlan p;
    if (n < 1 || classes < 1 || splits < 1 || splits > n || !is_plan(n, classes, splits, p)) return 0;
    return p.total * sizeof(double);
}

int gz_inception_score(const double* logits, long long n, int classes, int splits, double* scores, void* workspace,
                       size_t ws_bytes, hipStream_t stream) {
    gz::clear_stale_error();
    if (n < 1 || classes < 1 || splits < 1 || splits > n || !logits || !scores || !workspace) return GZ_ERR_BAD_SHAPE;
    IsPlan p;
    if (!is_plan(n, classes, splits, p)) return GZ_ERR_TOO_LARGE;
    if (ws_bytes < p.total * sizeof(double)) return GZ_ERR_WORKSPACE;
    double* ws = reinterpret_cast<double*>(workspace);
    double *rowstat = ws + p.rowstat, *colpart = ws + p.colpart, *logpy = ws + p.logpy, *klpart = ws + p.klpart;
    const unsigned groups = (unsigned)(splits * p.nblk), cblocks = (unsigned)p.cblocks;
    const dim3 threads(IS_THREADS);
    int rc;
    hipLaunchKernelGGL(is_rowstat_kernel, dim3((unsigned)((p.rows + IS_ROWS - 1) / IS_ROWS)), threads, 0, stream, logits,
                       p.rows, classes, rowstat);
    if ((rc = launch_status()) != GZ_OK) return rc;
    hipLaunchKernelGGL(is_colsum_kernel, dim3(groups * cblocks), threads, 0, stream, logits, classes, p.m, p.nblk,
                       (int)cblocks, (const double*)rowstat, colpart);
    if ((rc = launch_status()) != GZ_OK) return rc;
    hipLaunchKernelGGL(is_logpy_kernel, dim3((unsigned)splits * cblocks), threads, 0, stream, (const double*)colpart,
                       classes, p.m, p.nblk, (int)cblocks, logpy);
    if ((rc = launch_status()) != GZ_OK) return rc;
    hipLaunchKernelGGL(is_kl_kernel, dim3(groups), threads, 0, stream, logits, classes, p.m, p.nblk,
                       (const double*)rowstat, (const double*)logpy, klpart);
    if ((rc = launch_status()) != GZ_OK) return rc;
    hipLaunchKernelGGL(is_finish_kernel, dim3((unsigned)((splits + 63) / 64)), dim3(64), 0, stream,
                       (const double*)klpart, p.m, p.nblk, splits, scores);
    return launch_status();
}

}  // extern "C"
