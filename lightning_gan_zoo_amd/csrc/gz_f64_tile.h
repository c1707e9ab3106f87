// The fp64 MFMA tile core of gz_kid.hip (KID sums), gz_moments.hip (covariance) and gz_sqrtm.hip (Newton-Schulz
// product): the one place that knows the layout.  A kernel over it keeps its tile or band walk, its
// two fetch callables, its epilogue and its launcher.
//
//   * 256 threads compute a 64 x 64 tile of  sum_k A[row][k] B[k][col]  on v_mfma_f64_16x16x4_f64.  Wave w owns tile
//     rows 16w .. 16w+15 and four 16 x 16 accumulators (the tile's 64 columns).  The instruction takes A as
//     row = lane & 15, k = lane >> 4 and B as k = lane >> 4, col = lane & 15, one double per lane each, and returns C/D as
//     col = lane & 15, row = (lane >> 4) + 4 * reg -- NOT the f32 kernels' map (f64_acc_row / f64_acc_col).
//   * The reduction index travels in chunks of 32: global -> registers -> LDS, one chunk ahead of the MFMAs
//     (f64_tile_mainloop).  A thread owns 8 doubles per operand and chunk; which ones is the image's loader map.
//   * An operand's LDS image has one of two forms, chosen by which index is contiguous in global memory:
//       F64RowK  [index][k], pitch 32 + 2 doubles.  The loader owns k = tid & 31 of rows (tid >> 5) + 8 i: half a
//                wave's global load is 256 contiguous bytes of one row, its LDS write 32 consecutive doubles of one
//                row.  The pitch is 68 dwords = 4 (mod 64) and keeps rows 16-byte aligned.  With the interleaved slot
//                map a lane reads image[16 block + (lane & 15)][4 s + (lane >> 4)] by ds_read_b64, whose banks are
//                (byte / 4) % 64 and whose conflicts count inside a 32-lane half: there the banks are
//                4 (lane & 15) + 2 (k slot parity) + 8 s, two dwords each -- all 64 banks once.  With the blocked slot
//                map a lane's 8 k of a chunk are 64 contiguous, 16-byte aligned bytes, which the compiler reads as
//                four ds_read_b128; 16 rows span all banks.
//       F64KCol  [k][index], pitch 64 + 16 doubles.  The loader owns index = tid & 63 of k rows (tid >> 6) + 4 i: a
//                wave's global load is 512 contiguous bytes, its LDS write 64 consecutive doubles of one k row.  At
//                step s a lane reads image[4 s + (lane >> 4)][16 block + (lane & 15)]: the 16 lanes of a k slot read
//                16 consecutive doubles, 32 consecutive banks; inside a 32-lane half the two k slots (4s and 4s+1, or
//                4s+2 and 4s+3) are one pitch apart, and 160 dwords = 32 (mod 64) puts the second on the other 32
//                banks: conflict-free.
//   * The k slot of MFMA step s (s = 0..7 per chunk) is a policy, the same on both operands of a kernel:
//     F64SlotInterleaved 4 s + (lane >> 4), F64SlotBlocked 8 (lane >> 4) + s.  Per accumulator the steps run s = 0..7
//     inside a chunk and the chunks in order; with the slot map this fixes the order in which every dot product is
//     summed, hence every bit of it (tests/test_f64_tile_parent_bits_gpu.py holds the kernels to recorded bits).
//   * Tails belong to the fetch callables: an element outside the operand must arrive as 0.0 (or be masked in the
//     kernel's epilogue); the core never sees a shape.
//   * No floating-point atomics; a sum over the workgroup is folded in a fixed order (f64_workgroup_sum).
#pragma once
#include "gz_common.h"

namespace gz {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int F64_THREADS = 256;
constexpr int F64_TILE = 64;                  // rows = columns per tile
constexpr int F64_KC = 32;                    // reduction indices per LDS chunk
constexpr int F64_LOADS = F64_TILE * F64_KC / F64_THREADS;      // doubles per thread, operand and chunk

// The two LDS images.  own_index / own_k: the element of a chunk that thread `tid` fetches as load i and stores;
// at: the offset of element (index, k) in doubles, for that store and for the fragment reads.
struct F64RowK {
    static constexpr int PITCH = F64_KC + 2;
    static constexpr int SIZE = F64_TILE * PITCH;
    static __device__ __forceinline__ int own_index(int tid, int i) { return (tid >> 5) + 8 * i; }
    static __device__ __forceinline__ int own_k(int tid, int) { return tid & 31; }
    static __device__ __forceinline__ int at(int index, int k) { return index * PITCH + k; }
};
struct F64KCol {
    static constexpr int PITCH = F64_TILE + 16;
    static constexpr int SIZE = F64_KC * PITCH;
    static __device__ __forceinline__ int own_index(int tid, int) { return tid & 63; }
    static __device__ __forceinline__ int own_k(int tid, int i) { return (tid >> 6) + 4 * i; }
    static __device__ __forceinline__ int at(int index, int k) { return k * PITCH + index; }
};

// k within the chunk that lanes of k group fg = lane >> 4 feed to MFMA step s
struct F64SlotInterleaved {
    static __device__ __forceinline__ int k(int s, int fg) { return 4 * s + fg; }
};
struct F64SlotBlocked {
    static __device__ __forceinline__ int k(int s, int fg) { return 8 * fg + s; }
};

// tile coordinates of acc[j][r] in thread tid
__device__ __forceinline__ int f64_acc_row(int tid, int r) { return 16 * (tid >> 6) + ((tid & 63) >> 4) + 4 * r; }
__device__ __forceinline__ int f64_acc_col(int tid, int j) { return 16 * j + (tid & 15); }

// acc[j][r] = sum over nchunks chunks of A[f64_acc_row][k] * B[k][f64_acc_col].  fetch_a / fetch_b(chunk, v) load the
// calling thread's 8 elements of a chunk (the image's own_index / own_k) into v.  Every thread of the workgroup calls it;
// it starts with a barrier, so sA / sB may have been read until the call, and ends without one: a caller that reuses
// sA / sB afterwards synchronises first.
template <class ImgA, class ImgB, class Slot, class FetchA, class FetchB>
__device__ __forceinline__ void f64_tile_mainloop(double* sA, double* sB, long long nchunks, FetchA fetch_a,
                                                  FetchB fetch_b, f64x4 (&acc)[4]) {
    const int tid = threadIdx.x, wave = tid >> 6;
    const int fr = tid & 15, fg = (tid & 63) >> 4;       // MFMA fragment: row / column within the 16-block, k group
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    double pa[F64_LOADS], pb[F64_LOADS];
    fetch_a(0, pa);
    fetch_b(0, pb);
    for (long long c = 0; c < nchunks; ++c) {
        __syncthreads();                                 // the previous chunk's readers are done with sA / sB
#pragma unroll
        for (int i = 0; i < F64_LOADS; ++i) {
            sA[ImgA::at(ImgA::own_index(tid, i), ImgA::own_k(tid, i))] = pa[i];
            sB[ImgB::at(ImgB::own_index(tid, i), ImgB::own_k(tid, i))] = pb[i];
        }
        __syncthreads();
        if (c + 1 < nchunks) {
            fetch_a(c + 1, pa);
            fetch_b(c + 1, pb);
        }
#pragma unroll
        for (int s = 0; s < F64_KC / 4; ++s) {
            const double a = sA[ImgA::at(wave * 16 + fr, Slot::k(s, fg))];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double b = sB[ImgB::at(j * 16 + fr, Slot::k(s, fg))];
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
            }
        }
    }
}

// Sum of v over the workgroup in a fixed order: the lanes of a wave by the xor butterfly, the four waves in wave order.
// sW: F64_THREADS / 64 doubles of LDS of this sum's own.  Every thread calls it (it holds a barrier) and gets the sum.
__device__ __forceinline__ double f64_workgroup_sum(double v, double* sW) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sW[0] + sW[1]) + sW[2]) + sW[3];
}

}  // namespace gz
