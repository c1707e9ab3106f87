// The two primitives of the coupled Newton-Schulz matrix square root behind the device Frechet distance
// (eval.sqrtm_psd_device / eval.frechet_distance_device), in fp64:
//
//     C = alpha * (A B) + beta * I            square product of row-major d x d matrices on v_mfma_f64_16x16x4_f64
//     out = { trace(A), |A|_F^2 }             a fixed-order reduction
//
// Product: one workgroup per 64 x 64 tile of C, the whole reduction index inside it; blockIdx.y picks one of up to two
// independent problems of one size (the iteration's Y T and T Z share a launch).  No symmetry is assumed.
//   * A is read with the reduction index contiguous, as gz_kid.hip reads codes: a thread owns k = tid & 31 of eight rows,
//     so half a wave's global load is 256 contiguous bytes of one row.  LDS image [row][k], pitch SQ_LDA = 32 + 2
//     doubles = 68 dwords = 4 (mod 64).  At MFMA step t a lane reads image[16 wave + (lane & 15)][4 t + (lane >> 4)]: inside a
//     32-lane half the banks are 4 (lane & 15) + 2 (k slot parity) + 8 t, two dwords each -- all 64 banks once.  The
//     writes are half a wave storing 32 consecutive doubles of one row;
//   * B is read with the output column contiguous, as gz_moments.hip reads sample rows: a thread owns column tid & 63 of
//     eight k rows, a wave's global load is 512 contiguous bytes.  LDS image [k][column], pitch SQ_LDB = 64 + 16 doubles
//     = 32 (mod 64) dwords: the 16 lanes of a k slot read 16 consecutive doubles, the next slot lands on the other 32
//     banks;
//   * tails: an index >= d, row, column or reduction index, is never dereferenced and is zero in LDS, so d needs no
//     multiple of anything; the epilogue stores only rows and columns < d;
//   * wave w owns tile rows 16w .. 16w+15 and four 16 x 16 accumulators (the tile's 64 columns); C/D layout:
//     col = lane & 15, row = (lane >> 4) + 4 * reg.  Chunks of SQ_KC reduction indices travel global -> registers -> LDS
//     one chunk ahead of the MFMAs; an entry is summed over k in k order (four at a time inside an MFMA);
//   * epilogue: alpha * acc + (row == column ? beta : 0), stored from the accumulators: the 16 lanes of a row write
//     128 contiguous bytes.
// Reduction: sqrtm_partial_kernel sums SQ_RROWS rows per workgroup (a thread walks its elements in index order, the
// lanes fold by the xor butterfly, the four waves in wave order) into the workspace; sqrtm_finish_kernel adds the
// workgroups' shares in workgroup order.
// No floating-point atomics, a fixed order for every sum, nothing read from an output or the workspace before this call
// wrote it: two calls give equal bits.
#include "gz_common.h"
#include "../../include/gz_ops.h"

namespace gz {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SQ_THREADS = 256;
constexpr int SQ_TILE = 64;                   // rows = columns per tile
constexpr int SQ_KC = 32;                     // reduction indices per LDS chunk
constexpr int SQ_LDA = SQ_KC + 2;             // pitch of A's image [row][k] in doubles (see above)
constexpr int SQ_LDB = SQ_TILE + 16;          // pitch of B's image [k][column] in doubles (see above)
constexpr int SQ_LOADS = SQ_TILE * SQ_KC / SQ_THREADS;          // doubles per thread, operand and chunk
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

// A[row0 + lr + 8 i][k], zero outside the matrix
__device__ __forceinline__ void sq_fetch_a(const double* __restrict__ a, int d, int row0, int lr, int k,
                                           double (&v)[SQ_LOADS]) {
#pragma unroll
    for (int i = 0; i < SQ_LOADS; ++i) {
        const int row = row0 + lr + 8 * i;
        v[i] = (row < d && k < d) ? a[(long long)row * d + k] : 0.0;
    }
}

// B[k0 + lr + 4 i][col], zero outside the matrix
__device__ __forceinline__ void sq_fetch_b(const double* __restrict__ b, int d, int k0, int lr, int col,
                                           double (&v)[SQ_LOADS]) {
#pragma unroll
    for (int i = 0; i < SQ_LOADS; ++i) {
        const int k = k0 + lr + 4 * i;
        v[i] = (k < d && col < d) ? b[(long long)k * d + col] : 0.0;
    }
}

__global__ __launch_bounds__(SQ_THREADS) void sqrtm_product_kernel(SqProblems probs, int d, int tiles) {
    __shared__ __attribute__((aligned(16))) double sA[SQ_TILE * SQ_LDA];
    __shared__ __attribute__((aligned(16))) double sB[SQ_KC * SQ_LDB];

    const SqProblem& pr = probs.p[blockIdx.y];
    const double* __restrict__ A = pr.a;
    const double* __restrict__ B = pr.b;
    const int ti = (int)blockIdx.x / tiles, tj = (int)blockIdx.x % tiles;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ak = tid & 31, ar = tid >> 5;              // A loader: k within the chunk, first of its 8 rows
    const int bc = tid & 63, br = tid >> 6;              // B loader: column within the tile, first of its 8 k rows
    const int fr = lane & 15, fg = lane >> 4;            // MFMA fragment: row / column within the 16-block, k slot
    const int row0 = ti * SQ_TILE, col0 = tj * SQ_TILE;

    f64x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    double pa[SQ_LOADS], pb[SQ_LOADS];
    sq_fetch_a(A, d, row0, ar, ak, pa);
    sq_fetch_b(B, d, 0, br, col0 + bc, pb);
    const int nchunks = (d + SQ_KC - 1) / SQ_KC;
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();                                 // the previous chunk's readers are done with sA / sB
#pragma unroll
        for (int i = 0; i < SQ_LOADS; ++i) {
            sA[(ar + 8 * i) * SQ_LDA + ak] = pa[i];
            sB[(br + 4 * i) * SQ_LDB + bc] = pb[i];
        }
        __syncthreads();
        if (c + 1 < nchunks) {
            sq_fetch_a(A, d, row0, ar, (c + 1) * SQ_KC + ak, pa);
            sq_fetch_b(B, d, (c + 1) * SQ_KC, br, col0 + bc, pb);
        }
#pragma unroll
        for (int t = 0; t < SQ_KC / 4; ++t) {
            const double a = sA[(wave * 16 + fr) * SQ_LDA + 4 * t + fg];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double b = sB[(4 * t + fg) * SQ_LDB + j * 16 + fr];
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
            }
        }
    }

    // acc[j][r] is the dot product of row row0 + wave*16 + fg + 4r of A and column col0 + j*16 + fr of B
    double* __restrict__ C = pr.c;
    const double alpha = pr.alpha, beta = pr.beta;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + j * 16 + fr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + wave * 16 + fg + 4 * r;
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    f = wave_sum_d(f);
    t = wave_sum_d(t);
    if (lane == 0) {
        sF[wave] = f;
        sT[wave] = t;
    }
    __syncthreads();
    if (tid == 0) {
        partial[2 * (size_t)blockIdx.x] = ((sT[0] + sT[1]) + sT[2]) + sT[3];
        partial[2 * (size_t)blockIdx.x + 1] = ((sF[0] + sF[1]) + sF[2]) + sF[3];
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
