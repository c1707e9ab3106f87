// The two primitives of the coupled Newton-Schulz matrix square root behind the device Frechet distance
// (eval.sqrtm_psd_device / eval.frechet_distance_device), in fp64:
//
//     C = alpha * (A B) + beta * I            square product of row-major d x d matrices on v_mfma_f64_16x16x4_f64
//     out = { trace(A), |A|_F^2 }             a fixed-order reduction
//
// Product: one workgroup per 64 x 64 tile of C, the whole reduction index inside it; blockIdx.y picks one of up to two
// independent problems of one size (the iteration's Y T and T Z share a launch).  No symmetry is assumed.  The tile
// runs on the fp64 tile core (gz_f64_tile.h, the interleaved k-slot map) with one image of each form:
//   * A is read with the reduction index contiguous: the [row][k] image;
//   * B is read with the output column contiguous: the [k][column] image;
//   * tails: an index >= d, row, column or reduction index, is never dereferenced and is zero in LDS, so d needs no
//     multiple of anything; the epilogue stores only rows and columns < d.  An entry is summed over k in k order (four
//     at a time inside an MFMA);
//   * epilogue: alpha * acc + (row == column ? beta : 0), stored from the accumulators: the 16 lanes of a row write
//     128 contiguous bytes.
// Reduction: sqrtm_partial_kernel sums SQ_RROWS rows per workgroup (a thread walks its elements in index order, then the
// core's fixed-order fold over the workgroup) into the workspace; sqrtm_finish_kernel adds the workgroups' shares in
// workgroup order.
// No floating-point atomics, a fixed order for every sum, nothing read from an output or the workspace before this call
// wrote it: two calls give equal bits.
#include "gz_f64_tile.h"
#include "../../include/gz_ops.h"

namespace gz {

constexpr int SQ_THREADS = F64_THREADS;
constexpr int SQ_TILE = F64_TILE;             // rows = columns per tile
constexpr int SQ_RROWS = 8;                   // rows per workgroup of the reduction

struct SqProblem {
    const double* a;
    const double* b;
    double* c;
    double alpha, beta;
};
struct SqProblems {
    SqProblem p[2];
};

// the thread's 8 elements of chunk c of A's rows row0 .. and of B's columns col0 .., zero outside the matrix
__device__ __forceinline__ void sq_fetch_a(const double* __restrict__ a, int d, int row0, int c,
                                           double (&v)[F64_LOADS]) {
    const int tid = threadIdx.x, k = c * F64_KC + F64RowK::own_k(tid, 0);
#pragma unroll
    for (int i = 0; i < F64_LOADS; ++i) {
        const int row = row0 + F64RowK::own_index(tid, i);
        v[i] = (row < d && k < d) ? a[(long long)row * d + k] : 0.0;
    }
}

__device__ __forceinline__ void sq_fetch_b(const double* __restrict__ b, int d, int col0, int c,
                                           double (&v)[F64_LOADS]) {
    const int tid = threadIdx.x, col = col0 + F64KCol::own_index(tid, 0);
#pragma unroll
    for (int i = 0; i < F64_LOADS; ++i) {
        const int k = c * F64_KC + F64KCol::own_k(tid, i);
        v[i] = (k < d && col < d) ? b[(long long)k * d + col] : 0.0;
    }
}

__global__ __launch_bounds__(SQ_THREADS) void sqrtm_product_kernel(SqProblems probs, int d, int tiles) {
    __shared__ __attribute__((aligned(16))) double sA[F64RowK::SIZE];
    __shared__ __attribute__((aligned(16))) double sB[F64KCol::SIZE];

    const SqProblem& pr = probs.p[blockIdx.y];
    const double* __restrict__ A = pr.a;
    const double* __restrict__ B = pr.b;
    const int ti = (int)blockIdx.x / tiles, tj = (int)blockIdx.x % tiles;
    const int tid = threadIdx.x;
    const int row0 = ti * SQ_TILE, col0 = tj * SQ_TILE;

    f64x4 acc[4];
    f64_tile_mainloop<F64RowK, F64KCol, F64SlotInterleaved>(
        sA, sB, (d + F64_KC - 1) / F64_KC,
        [&](long long c, double (&v)[F64_LOADS]) { sq_fetch_a(A, d, row0, (int)c, v); },
        [&](long long c, double (&v)[F64_LOADS]) { sq_fetch_b(B, d, col0, (int)c, v); }, acc);

    // acc[j][r] is the dot product of row row0 + f64_acc_row(r) of A and column col0 + f64_acc_col(j) of B
    double* __restrict__ C = pr.c;
    const double alpha = pr.alpha, beta = pr.beta;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + f64_acc_col(tid, j);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + f64_acc_row(tid, r);
            if (row < d && col < d) {
                C[(long long)row * d + col] = alpha * acc[j][r] + (row == col ? beta : 0.0);
            }
        }
    }
}

// the share of rows SQ_RROWS * block .. of trace(A) and |A|_F^2 -> partial[block][2]
__global__ __launch_bounds__(SQ_THREADS) void sqrtm_partial_kernel(const double* __restrict__ a, int d,
                                                                   double* __restrict__ partial) {
    __shared__ double sT[SQ_THREADS / 64], sF[SQ_THREADS / 64];
    const int tid = threadIdx.x;
    const int r0 = (int)blockIdx.x * SQ_RROWS;
    const int rows = d - r0 < SQ_RROWS ? d - r0 : SQ_RROWS;
    const long long count = (long long)rows * d;
    const double* p = a + (long long)r0 * d;
    double f = 0.0;
    for (long long i = tid; i < count; i += SQ_THREADS) {
        const double v = p[i];
        f += v * v;
    }
    double t = tid < rows ? a[(long long)(r0 + tid) * d + r0 + tid] : 0.0;
    f = f64_workgroup_sum(f, sF);
    t = f64_workgroup_sum(t, sT);
    if (tid == 0) {
        partial[2 * (size_t)blockIdx.x] = t;
        partial[2 * (size_t)blockIdx.x + 1] = f;
    }
}

__global__ __launch_bounds__(64) void sqrtm_finish_kernel(const double* __restrict__ partial, int nblk,
                                                          double* __restrict__ out) {
    const int q = threadIdx.x;
    if (q >= 2) return;
    double v = 0.0;
    for (int b = 0; b < nblk; ++b) v += partial[2 * (size_t)b + q];
    out[q] = v;
}

inline int sq_row_blocks(int d) { return (d + SQ_RROWS - 1) / SQ_RROWS; }

// [p, p + count doubles) and [q, q + count doubles) share a byte
inline bool sq_overlap(const double* p, const double* q, size_t count) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    const uintptr_t bytes = (uintptr_t)count * sizeof(double);
    return a < b + bytes && b < a + bytes;
}

inline int sq_launch(const SqProblems& probs, int count, int d, hipStream_t stream) {
    const long long tiles = ((long long)d + SQ_TILE - 1) / SQ_TILE;
    if (tiles * tiles > 0x7fffffffll) return GZ_ERR_TOO_LARGE;
    hipLaunchKernelGGL(sqrtm_product_kernel, dim3((unsigned)(tiles * tiles), (unsigned)count), dim3(SQ_THREADS), 0, stream,
                       probs, d, (int)tiles);
    return launch_status();
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_sqrtm_product(const double* a, const double* b, double* c, int d, double alpha, double beta,
                     hipStream_t stream) {
    gz::clear_stale_error();
    if (d < 1 || !a || !b || !c) return GZ_ERR_BAD_SHAPE;
    const size_t count = (size_t)d * (size_t)d;
    if (sq_overlap(c, a, count) || sq_overlap(c, b, count)) return GZ_ERR_BAD_SHAPE;
    SqProblems probs;
    probs.p[0] = SqProblem{a, b, c, alpha, beta};
    probs.p[1] = probs.p[0];
    return sq_launch(probs, 1, d, stream);
}

int gz_sqrtm_product_pair(const double* a0, const double* b0, double* c0, double alpha0, double beta0,
                          const double* a1, const double* b1, double* c1, double alpha1, double beta1, int d,
                          hipStream_t stream) {
    gz::clear_stale_error();
    if (d < 1 || !a0 || !b0 || !c0 || !a1 || !b1 || !c1) return GZ_ERR_BAD_SHAPE;
    const size_t count = (size_t)d * (size_t)d;
    if (sq_overlap(c0, c1, count)) return GZ_ERR_BAD_SHAPE;
    for (const double* c : {(const double*)c0, (const double*)c1})
        for (const double* in : {a0, b0, a1, b1})
            if (sq_overlap(c, in, count)) return GZ_ERR_BAD_SHAPE;
    SqProblems probs;
    probs.p[0] = SqProblem{a0, b0, c0, alpha0, beta0};
    probs.p[1] = SqProblem{a1, b1, c1, alpha1, beta1};
    return sq_launch(probs, 2, d, stream);
}

size_t gz_sqrtm_trace_norm_workspace_bytes(int d) {
    if (d < 1) return 0;
    return (size_t)sq_row_blocks(d) * 2 * sizeof(double);
}

int gz_sqrtm_trace_norm(const double* a, int d, double* out, void* workspace, size_t ws_bytes, hipStream_t stream) {
    gz::clear_stale_error();
    if (d < 1 || !a || !out || !workspace) return GZ_ERR_BAD_SHAPE;
    if (ws_bytes < gz_sqrtm_trace_norm_workspace_bytes(d)) return GZ_ERR_WORKSPACE;
    const int nblk = sq_row_blocks(d);
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(sqrtm_partial_kernel, dim3((unsigned)nblk), dim3(SQ_THREADS), 0, stream, a, d, partial);
    const int rc = launch_status();
    if (rc != GZ_OK) return rc;
    hipLaunchKernelGGL(sqrtm_finish_kernel, dim3(1), dim3(64), 0, stream, (const double*)partial, nblk, out);
    return launch_status();
}

}  // extern "C"
