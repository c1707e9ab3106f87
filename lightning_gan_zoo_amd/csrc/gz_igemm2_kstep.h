// Part of the fp32 implicit-GEMM core (see gz_igemm.h), igemm2 skeleton: the pieces a hand-ordered k-step is written from
// (LDS reads, MFMA rows, the wait that closes a k-step), the unroll helper and the diagnostics of the three kernels.
#pragma once
#include "gz_igemm_core.h"
#include <utility>

namespace gz {

// f(integral_constant<int, FIRST>{}), ..., f(integral_constant<int, FIRST + N - 1>{}): the k-steps of a loop body, written out
template <int FIRST, class F, int... I>
__device__ __forceinline__ void static_for_seq(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, FIRST + I>{}), ...);
}
template <int N, int FIRST = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_seq<FIRST>(f, std::make_integer_sequence<int, N>{});
}

// ---- diagnostics: nothing of this is in a product build ----------------------------------------------------------------
// Timing experiments of igemm2_kernel (-DGZ2_EXP_* builds: tools/Makefile; wrong results): what each takes out of the loop
#ifdef GZ2_EXP_NODMA      // LDS-DMA pieces past the prologue's
constexpr bool GZ2_NODMA = true;
#else
constexpr bool GZ2_NODMA = false;
#endif
#ifdef GZ2_EXP_SAMECHUNK      // ... re-load the first chunk (cache-resident)
constexpr bool GZ2_SAMECHUNK = true;
#else
constexpr bool GZ2_SAMECHUNK = false;
#endif
#ifdef GZ2_EXP_NOFETCH      // the fragment reads
constexpr bool GZ2_NOFETCH = true;
#else
constexpr bool GZ2_NOFETCH = false;
#endif
#ifdef GZ2_EXP_NO_LGKM_PROLOGUE      // lgkmcnt(0) in front of the first barrier
constexpr bool GZ2_NO_LGKM_PROLOGUE = true;
#else
constexpr bool GZ2_NO_LGKM_PROLOGUE = false;
#endif
#ifdef GZ2_EXP_NOVMWAIT      // the counted wait of the last k-step
constexpr bool GZ2_NOVMWAIT = true;
#else
constexpr bool GZ2_NOVMWAIT = false;
#endif
#ifdef GZ2_EXP_NOBARRIER      // ... and its s_barrier
constexpr bool GZ2_NOBARRIER = true;
#else
constexpr bool GZ2_NOBARRIER = false;
#endif
#ifdef GZ2_EXP_NOSTORE      // the epilogue (one store kept: live accumulators)
constexpr bool GZ2_NOSTORE = true;
#else
constexpr bool GZ2_NOSTORE = false;
#endif
#ifdef GZ2_STEP_STAMPS      // with GZ2_STAMPS: cycles per k-step position, at the counted wait and at the barrier
constexpr bool GZ2_STEP = true;
#else
constexpr bool GZ2_STEP = false;
#endif

// In-kernel stamps of igemm2_kernel (s_memtime), read back by gz_debug_read_stamps / tools/conv_bench2.py --stamps.
// gz2_stamps row blockIdx.x (< 8192): entry, loop start, loop end, exit, s_memrealtime at entry and exit, chunks, TM * TN.
// With GZ2_STEP_STAMPS also, for blockIdx.x < 64: row 8192-64+blockIdx.x = cycles per k-step position summed over the
// chunks (the first 8), row 8192-128+blockIdx.x = cycles in the counted vmcnt wait (the DMA), in the s_barrier (the other
// wavefronts), chunks of wave group 0.  (Those rows are the main rows of a grid above 8064 workgroups too, and every
// z-slab with blockIdx.x < 64 writes them: the last writer stays -- fine for a diagnostic of grids of a few hundred.)
#ifdef GZ2_STAMPS
__device__ unsigned long long gz2_stamps[8192 * 8];
// (a device array per unit that includes this header: launch_igemm2 notes here which unit's array its kernel writes, and
// gz_debug_read_stamps reads that one -- the stamps of the last igemm2 launch, whichever unit launched it)
inline const void*& gz2_last_stamps() {
    static const void* last = nullptr;
    return last;
}
template <int STEPS>
struct Igemm2Probe {
    static constexpr bool STEP = GZ2_STEP;
    unsigned long long st0, st1, st2, sr0;
    unsigned long long step_cyc[STEPS] = {}, step_t = 0, wait_cyc[2] = {0, 0}, tw0 = 0, tw1 = 0;
    __device__ __forceinline__ void entry() {
        st0 = __builtin_amdgcn_s_memtime();
        sr0 = __builtin_amdgcn_s_memrealtime();
        st1 = st2 = st0;
    }
    __device__ __forceinline__ void loop_start() {
        st1 = __builtin_amdgcn_s_memtime();
        if constexpr (STEP) step_t = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void wait_begin() {
        if constexpr (STEP) tw0 = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void wait_end() {
        if constexpr (STEP) tw1 = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void barrier_end() {
        if constexpr (STEP) {
            const unsigned long long tw2 = __builtin_amdgcn_s_memtime();
            wait_cyc[0] += tw1 - tw0;
            wait_cyc[1] += tw2 - tw1;
        }
    }
    template <int S>
    __device__ __forceinline__ void kstep_end() {
        if constexpr (STEP) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            step_cyc[S % STEPS] += t - step_t;
            step_t = t;
        }
    }
    __device__ __forceinline__ void loop_end(int tid, int kg, int chunks) {
        st2 = __builtin_amdgcn_s_memtime();
        if constexpr (STEP) {
            if (tid == 0 && blockIdx.x < 64)
                for (int q = 0; q < 8; ++q) gz2_stamps[(size_t)(8192 - 64 + blockIdx.x) * 8 + q] = step_cyc[q];
            if (tid == 0 && kg == 0 && blockIdx.x < 64) {
                gz2_stamps[(size_t)(8192 - 128 + blockIdx.x) * 8 + 0] = wait_cyc[0];
                gz2_stamps[(size_t)(8192 - 128 + blockIdx.x) * 8 + 1] = wait_cyc[1];
                gz2_stamps[(size_t)(8192 - 128 + blockIdx.x) * 8 + 2] = (unsigned long long)chunks;
            }
        }
    }
    __device__ __forceinline__ void exit(int tid, int chunks, int mfmas) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0 && blockIdx.x < 8192) {
            unsigned long long* o = gz2_stamps + (size_t)blockIdx.x * 8;
            o[0] = st0; o[1] = st1; o[2] = st2; o[3] = __builtin_amdgcn_s_memtime();
            o[4] = sr0; o[5] = __builtin_amdgcn_s_memrealtime(); o[6] = chunks; o[7] = mfmas;
        }
    }
};
#else
template <int STEPS>
struct Igemm2Probe {
    __device__ __forceinline__ void entry() {}
    __device__ __forceinline__ void loop_start() {}
    __device__ __forceinline__ void wait_begin() {}
    __device__ __forceinline__ void wait_end() {}
    __device__ __forceinline__ void barrier_end() {}
    template <int S>
    __device__ __forceinline__ void kstep_end() {}
    __device__ __forceinline__ void loop_end(int tid, int kg, int chunks) {}
    __device__ __forceinline__ void exit(int tid, int chunks, int mfmas) {}
};
#endif

// ---- hand-ordered instruction stream of one k-step ---------------------------------------------------------------
// hipcc's scheduler is not latency-aware here: it puts the v_cndmask that zeroes a fragment right behind the ds_read
// that fetches it (sched_group_barrier / sched_barrier variants all ended with an exposed LDS latency per k-step:
// 78-90 % of the MFMA-issue bound for a wavefront that has its SIMD to itself).  So the stream is written out:
//   ds_read (next k-step's fragments) ... the TM*TN MFMAs of this k-step ... s_waitcnt lgkmcnt(0) (in the shadow of
//   the last MFMA: the reads are ~1000 cycles old) ... masks of the next k-step.
// Every piece is an `asm volatile`; the wait statement takes the freshly read registers as in/out operands, so no use
// of them can be scheduled above it, and the compiler's own code (LDS-DMA issue, loop control) can only fall between
// pieces.  Accumulators live in AGPRs ("+a").
// (no wait states needed in front of the MFMAs: their A / B registers are written by ds_read only -- the zero column
// replaced the v_cndmask masks -- and s_waitcnt covers that)
#ifndef GZ2_EXP_NOP
#define GZ2_NOP ""
#else
#define GZ2_NOP "s_nop 1\n\t"
#endif
template <int OFF>
__device__ __forceinline__ float lds_rd(uint32_t byte_addr) {
    float v;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(byte_addr), "n"(OFF) : "memory");
    return v;
}
__device__ __forceinline__ void mfma_row(f32x16 (&c)[4], float a, const float (&b)[4]) {
    // s_nop 1: a VALU write (the zeroing v_cndmask) needs two wait states before an MFMA reads the register, and the
    // hazard recognizer does not look inside asm statements
    asm volatile(GZ2_NOP
                 "v_mfma_f32_32x32x2_f32 %0, %5, %4, %0\n\t"
                 "v_mfma_f32_32x32x2_f32 %1, %6, %4, %1\n\t"
                 "v_mfma_f32_32x32x2_f32 %2, %7, %4, %2\n\t"
                 "v_mfma_f32_32x32x2_f32 %3, %8, %4, %3"
                 : "+a"(c[0]), "+a"(c[1]), "+a"(c[2]), "+a"(c[3])
                 : "v"(a), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]));
}
__device__ __forceinline__ void mfma_row(f32x16 (&c)[2], float a, const float (&b)[2]) {
    asm volatile(GZ2_NOP
                 "v_mfma_f32_32x32x2_f32 %0, %3, %2, %0\n\t"
                 "v_mfma_f32_32x32x2_f32 %1, %4, %2, %1"
                 : "+a"(c[0]), "+a"(c[1])
                 : "v"(a), "v"(b[0]), "v"(b[1]));
}
__device__ __forceinline__ void mfma_row(f32x16 (&c)[1], float a, const float (&b)[1]) {
    asm volatile(GZ2_NOP
                 "v_mfma_f32_32x32x2_f32 %0, %2, %1, %0"
                 : "+a"(c[0])
                 : "v"(a), "v"(b[0]));
}
__device__ __forceinline__ void mfma_one(f32x16& c, float a, float b) {      // dual mode, part B: accumulator block 0 only
    asm volatile(GZ2_NOP
                 "v_mfma_f32_32x32x2_f32 %0, %2, %1, %0"
                 : "+a"(c)
                 : "v"(a), "v"(b));
}
// D[m][n] order (lanes along n): row-major outputs (weight gradient slabs)
__device__ __forceinline__ void mfma_row_mn(f32x16 (&c)[4], float a, const float (&b)[4]) {
    asm volatile(GZ2_NOP
                 "v_mfma_f32_32x32x2_f32 %0, %4, %5, %0\n\t"
                 "v_mfma_f32_32x32x2_f32 %1, %4, %6, %1\n\t"
                 "v_mfma_f32_32x32x2_f32 %2, %4, %7, %2\n\t"
                 "v_mfma_f32_32x32x2_f32 %3, %4, %8, %3"
                 : "+a"(c[0]), "+a"(c[1]), "+a"(c[2]), "+a"(c[3])
                 : "v"(a), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]));
}
__device__ __forceinline__ void mfma_row_mn(f32x16 (&c)[2], float a, const float (&b)[2]) {
    asm volatile(GZ2_NOP
                 "v_mfma_f32_32x32x2_f32 %0, %2, %3, %0\n\t"
                 "v_mfma_f32_32x32x2_f32 %1, %2, %4, %1"
                 : "+a"(c[0]), "+a"(c[1])
                 : "v"(a), "v"(b[0]), "v"(b[1]));
}
__device__ __forceinline__ void lgkm_done(float (&a)[4], float (&b)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}
__device__ __forceinline__ void lgkm_done(float (&a)[4], float (&b)[2]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]));
}
__device__ __forceinline__ void lgkm_done(float (&a)[2], float (&b)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}
__device__ __forceinline__ void lgkm_done(float (&a)[4], float (&b)[1]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]));
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int OFF>
__device__ __forceinline__ f32x4 lds_rd4(uint32_t byte_addr) {
    f32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(byte_addr), "n"(OFF) : "memory");
    return v;
}
__device__ __forceinline__ void lgkm_done(float (&b)[2]) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b[0]), "+v"(b[1])); }
__device__ __forceinline__ void lgkm_done(f32x4 (&a)[4], float (&b)[2]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]));
}

}  // namespace gz
