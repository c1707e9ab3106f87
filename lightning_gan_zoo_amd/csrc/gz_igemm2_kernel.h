// Part of the fp32 implicit-GEMM core (see gz_igemm.h), igemm2 skeleton: igemm2_kernel and its launcher.
#pragma once
#include "gz_igemm2_loaders.h"
#include "gz_igemm2_kstep.h"

namespace gz {

// =====================================================================================================================
// Round 3: the one-wavefront-per-SIMD skeleton (igemm2).
//
// Why: four co-resident 128x128 workgroups per CU (igemm_kernel) keep the matrix pipe busy 80-83 % of the time; the
// loop itself (no global loads) tops out at 0.87-0.91 because four wavefronts per SIMD arbitrate for one pipe and each
// of them stalls at a barrier every 32 MFMAs.  Here ONE wavefront per SIMD owns a 128 x 128 (or 128 x 64) accumulator
// tile -- a 256 x 256 / 256 x 128 workgroup tile -- and runs an in-order, software-pipelined stream in which the
// MFMAs issue back to back and everything else sits in their shadow:
//   * operands arrive by LDS-DMA into a ring of D stages (D = 3 unless igemm2_depth() says otherwise); the pieces of
//     chunk t+D-1 are issued one per k-step between the MFMAs of chunk t, waited for with a COUNTED s_waitcnt
//     vmcnt((D-2) * pieces per chunk) (not 0 inside the loop at D >= 3: a chunk's pieces stay in flight across the
//     barrier) and made visible by ONE raw s_barrier per chunk (128 MFMAs per wavefront at TN = 4, 32 at TN = 1) --
//     __syncthreads() would drain the DMA queue.  Where igemm2_interval() is 2: one wait + barrier per TWO chunks, the
//     ring handled in P pairs of stages, the wait vmcnt((P-2) * 2 * pieces per chunk).  With P = 2 (TN = 1, KG = 1:
//     four stages, three workgroups per CU) that IS vmcnt(0) in the loop -- a double buffer of pairs: the next pair's
//     pieces go out in k-steps 0-5 of the pair's 16 and have ten k-steps (2560 cycles of the wavefront's own MFMAs) to
//     land, nothing stays in flight across the barrier.  A loader with more pieces per chunk (PPS > 1, or NP near
//     STEPS) issues later into the pair and should not be given P = 2 without measuring its wait;
//   * the wait + barrier sit inside the LAST k-step of a chunk, in front of its MFMAs, so the first fragments of the
//     next chunk are fetched under those MFMAs;
//   * fragments are double-buffered in registers one k-step ahead (8 ds_read_b32 per 16 MFMAs).
// tools/igemm2_probe.hip is this loop on a plain GEMM: 148-149 TFLOP/s (0.945 of the 157.3 peak) at K = 2048, main
// loop 98.2 % of the MFMA-issue bound (in-kernel s_memtime stamps), against 125-130 for igemm_kernel on the same size.
// Fragment / accumulator maps, LDS images ([k][m], m contiguous), GridMap, split-K slabs and the epilogues are the
// ones of igemm_kernel; the loaders are piece-wise:
//   static constexpr int LD, ROWS (LDS rows per chunk), PIECES (LDS-DMA instructions per wavefront and chunk);
//   void init(const Params&, int tile, int y, int tid);
//   void issue_piece(int kc, float* stage_base, int p, bool live);   // p in [0, PIECES), wave-uniform control flow
// =====================================================================================================================

// Pad-skip loaders: back to pixel order.  Block i of lane (half, l32) holds wavefront pixel (l32 >> 2) * 16 + 4 i + (l32 & 3)
// (i ^ mirror for i: ConvDgA2's reversed rows); block i', lane (half, l') must hold pixel 32 i' + l', which is block
// (l' >> 2) & 3 of lane (half, 8 i' + 4 (l' >> 4) + (l' & 3)).
// Through LDS, eight accumulator registers of the four blocks at a time: slot [q = block * 8 + register][thread], the
// wavefront's own 64 columns of `buf` (32 * NT floats) -- no other wavefront reads or writes them, and a wavefront's
// LDS operations complete in order, so no barrier between the passes.  The lane index is XORed with 8 * block on the
// way in: writes and reads both touch 32 different banks per 32-lane half.
template <int TM, int TN>
__device__ __forceinline__ void unpermute_padskip(f32x16 (&acc)[TM][TN], float* buf, int tid, int mirror) {
    static_assert(TM == 4, "four 32-row blocks per wavefront");
    constexpr int PR = 8;                           // accumulator registers per block and pass
    const int lane = tid & 63;
    float* const col = buf + (tid & ~63);
    const int sb = ((lane >> 2) & 3) ^ mirror;                             // source block
    const int sl = (lane & 32) | ((lane >> 4) & 1) << 2 | (lane & 3);      // source lane, without 8 i'
#pragma unroll
    for (int j = 0; j < TN; ++j) {
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += PR) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < PR; ++r) col[(i * PR + r) * NT + (lane ^ (i << 3))] = acc[i][j][r0 + r];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < PR; ++r) acc[i][j][r0 + r] = col[(sb * PR + r) * NT + ((sl | i << 3) ^ (sb << 3))];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// KG = 2 (round 5): TWO wave groups of four wavefronts in one 512-thread workgroup work on the SAME output tile, each on
// half of the workgroup's reduction range with an LDS ring of its own, and meet in LDS at the end (group 1 parks its
// accumulators, group 0 adds them and runs the epilogue).  For launches whose tiles x reduction splits give a CU only
// one workgroup: the CU then still holds two wavefronts per SIMD -- the second one is what hides the non-MFMA
// instructions of the k-step -- without the slabs + finish pass that a global split of the reduction costs.

template <class Cfg, class AL, class BL, class Epi, int KG = 1>
__global__ __launch_bounds__(NT * KG, KG == 1 ? Cfg::OCC : 2) void igemm2_kernel(typename AL::Params pa, typename BL::Params pb,
                                                                              typename Epi::Params pe, GridMap gm) {
    constexpr int LDA = AL::LD, LDB = BL::LD;
    constexpr int TM = Cfg::TM, TN = Cfg::TN;
    static_assert((TM == 4 || (TM == 2 && AL::DUALMODE)) && (TN == 1 || TN == 2 || TN == 4),
                  "fragment registers of the hand-ordered k-step");
    static_assert(KG == 1 || (KG == 2 && TN <= 2), "two wave groups: the parked accumulators must fit the LDS");
    constexpr bool RS = AL::ROWSHARE;
    constexpr bool FR = AL::FWDROWS;
    // (ConvDg5A2) MODES consecutive chunk ranges, each with its own k-step form: row-shared or plain fragment addressing
    // and the accumulator blocks (output phases) its MFMAs feed -- AL::step_plain, AL::step_mask, al.bound[]
    constexpr bool DM = AL::DUALMODE;
    static_assert(!DM || (RS && KG == 1 && (TN == 2 || TN == 4)), "multi-mode: row-shared loader, phases in the accumulator blocks");
    // pad-skip loaders (4x4 maps): blocks uniform in the map row, (block, k-step) pairs that are padding only left out
    // (AL::skip_mask: compile-time entries; PSB: block 0 in the k-steps of one parity, a wave-uniform branch),
    // accumulators back in pixel order before the epilogue
    constexpr bool PSK = AL::PADSKIP;
    constexpr bool PSB = AL::SKIP_BLOCK0_BY_PARITY;
    static_assert(!PSK || ((RS || FR) && !DM && TM == 4 && TN <= 2 && Cfg::BM == 256 && Cfg::WM == 2),
                  "pad-skip: 128-pixel wave tiles of a 256-pixel workgroup tile");
    static_assert(!PSK || igemm2_lds_bytes_at<Cfg, AL, BL, KG>(igemm2_depth<Cfg, AL, BL, KG>()) >= (size_t)32 * NT * 4,
                  "pad-skip: the un-permute's 32 slots per thread");
    constexpr int A_EXTRA = AL::EXTRA;
    constexpr int A_ELEMS = AL::ROWS * LDA + A_EXTRA, B_ELEMS = BL::ROWS * LDB;
    constexpr int STAGE = A_ELEMS + B_ELEMS;
    constexpr int PAD = 16;
    constexpr int DEPTH = igemm2_depth<Cfg, AL, BL, KG>();      // stages of the ring
    constexpr int BI = igemm2_interval<Cfg, AL, BL, KG>();      // chunks per barrier: the loop body is a GROUP of BI chunks
    constexpr int GROUPS = DEPTH / BI;                          // ... and the ring holds this many groups of stages
    static_assert(DEPTH % BI == 0 && (BI == 1 ? GROUPS >= 3 : GROUPS >= 2) && (BI == 1 || (BI == 2 && !DM)),
                  "group t+GROUPS-1 lands in the stages group t-1 was read from");
    // a deeper ring must not cost a resident workgroup (the gathers' three-stage forms are throttled by their LDS already)
    static_assert(DEPTH == STAGES2 || (KG == 2 ? igemm2_lds_bytes_kg2<Cfg, AL, BL>()
                                               : Cfg::OCC * igemm2_lds_bytes<Cfg, AL, BL>()) <= LDS_PER_CU,
                  "workgroups per CU x LDS per workgroup");
    extern __shared__ __attribute__((aligned(16))) float smem2[];
    const int kg = KG == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);      // wave group
    float* const ring = smem2 + PAD + kg * igemm2_ring_floats<Cfg, AL, BL, KG>();   // stage i: [B image][A image]
    Igemm2Probe<AL::KSTEPS> probe;      // (diagnostic builds: in-kernel stamps; empty otherwise)
    probe.entry();

    const int tid = KG == 1 ? (int)threadIdx.x : ((int)threadIdx.x & (NT - 1));     // inside the wave group
    const int nwg = gridDim.x;
    int bid = blockIdx.x;
    // (experiment, off by default -- see launch_igemm2)  The first-round workgroup in the CU's odd thread-group slot
    // starts a fraction of a tile late; the offset persists, because every later workgroup starts when its predecessor
    // in that slot ends.
    if (gm.stagger > 0 && bid < 512 && blockIdx.z == 0) {
        const unsigned hw = __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (16 << 6) | 4);      // HW_ID.TG_ID
        if (hw & 1u) {
            const unsigned long long t_end = __builtin_amdgcn_s_memtime() + (unsigned long long)gm.stagger;
            while (__builtin_amdgcn_s_memtime() < t_end) __builtin_amdgcn_s_sleep(64);
        }
    }
    int y;
    if (gm.var_chunks) {      // phases of unequal length: longest first over all tiles (see igemm_kernel)
        const int tiles = gm.tiles_m * gm.tiles_n;
        y = gm.phase_order[bid / tiles];
        bid %= tiles;
    } else {
        if (!gm.no_swizzle) {
            const int q = nwg >> 3, rr = nwg & 7, x = bid & 7, i = bid >> 3;
            bid = (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + i;
        }
        y = bid % gm.ny;
        bid /= gm.ny;
    }
    const int tile_n = bid % gm.tiles_n;
    const int tile_m = bid / gm.tiles_n;
    const int z = blockIdx.z;
    const int kcA = z * gm.chunks_per_split;                 // the workgroup's reduction range [kcA, kcB)
    const int kcB = min(gm.var_chunks ? gm.phase_chunks[y] : gm.chunks, kcA + gm.chunks_per_split);
    if (gm.slab && gm.var_chunks && kcA >= kcB) return;      // past this phase's last slab (uniform per workgroup)
    // this wave group's share: chunks [kc0, kc1) are live; the loop runs to kend in BOTH groups (same barrier count),
    // the chunks past kc1 arrive as zeros (out-of-range LDS-DMA) and add nothing
    int kc0 = kcA, kc1 = kcB, kend = kcB;
    if constexpr (KG == 2) {
        const int h = (kcB - kcA + 1) >> 1;
        kc0 = kcA + kg * h;
        kend = kc0 + h;
        kc1 = min(kcB, kend);
    }

    AL al;
    BL bl;
    al.init(pa, tile_m, y, tid);
    bl.init(pb, tile_n, y, tid);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / Cfg::WN, wn = wave % Cfg::WN;
    const int half = lane >> 5, l32 = lane & 31;
    // byte addresses (LDS) of this lane's fragment columns inside stage 0
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring;
    uint32_t a_addr[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
        a_addr[i] = lds0 + (uint32_t)(B_ELEMS + half * (RS ? 0 : LDA) + wm * TM * 32 + i * 32 + l32) * 4u;
    if constexpr (RS) {
        const int sh = al.frag_shift(half);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int b = (tile_m * Cfg::BM + wm * TM * 32 + i * 32 + l32) % pa.AW;
            const bool zero = (sh < 0 && b == 0) || (sh > 0 && b == pa.AW - 1);
            a_addr[i] = zero ? lds0 + (uint32_t)(B_ELEMS + AL::ZERO_COL) * 4u : a_addr[i] + (uint32_t)(sh * 4);
        }
        // the pad columns of every row of every stage
        static_assert(DEPTH * AL::ROWS * 4 <= NT, "one pad float per thread");
        if (tid < DEPTH * AL::ROWS * 4) {
            const int st = tid / (AL::ROWS * 4), q = tid % (AL::ROWS * 4);
            ring[st * STAGE + B_ELEMS + (q >> 2) * LDA + AL::ZERO_COL + (q & 3)] = 0.f;
        }
    }
    uint32_t a_addrB[TM];          // dual mode, part B: half-wave = next LDS row, ONE shift (-1) for both
    if constexpr (DM) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int b = (tile_m * Cfg::BM + wm * TM * 32 + i * 32 + l32) % pa.AW;
            a_addrB[i] = lds0 + (uint32_t)(B_ELEMS + half * LDA + (b == 0 ? AL::ZERO_COL : wm * TM * 32 + i * 32 + l32 - 1)) * 4u;
        }
    }
    uint32_t a_odd[TM];            // forward-row images: the odd k-steps' addresses (a_addr: the even ones)
    if constexpr (FR) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            int e, o;
            al.frag(wm * TM * 32 + i * 32 + l32, half, e, o);
            a_addr[i] = lds0 + (uint32_t)(B_ELEMS + e) * 4u;
            a_odd[i] = lds0 + (uint32_t)(B_ELEMS + o) * 4u;
        }
        for (int q = tid; q < DEPTH * A_EXTRA; q += NT)
            ring[(q / A_EXTRA) * STAGE + B_ELEMS + AL::ZERO + q % A_EXTRA] = 0.f;
    }
    const uint32_t b_addr = lds0 + (uint32_t)(half * LDB + wn * TN * 32 + l32) * 4u;

    constexpr int NPA = AL::PIECES, NPB = BL::PIECES, NP = NPA + NPB, STEPS = AL::KSTEPS;
    static_assert((STEPS == 8 || STEPS == 12) && (BI == 1 || STEPS == 8), "k-steps per chunk, per group 8, 12 or 16");
    constexpr int PPS = (NP + STEPS - 1) / STEPS;          // LDS-DMA pieces per k-step (1 for the 16-byte loaders)
    static_assert(PPS <= 4 && (DEPTH - BI) * NP < 64,
                  "pieces are spread over the k-step's four MFMA rows; vmcnt is 6 bits and DEPTH-BI chunks are in flight");
    constexpr int NWAIT = (DEPTH - 2 * BI) * NP;           // in flight behind the group that the counted wait is for
    constexpr int GSTEPS = BI * STEPS;                     // k-steps of the loop body
    auto issue_piece = [&](int kc, int st, int p, bool live) {
        if (GZ2_NODMA && kc >= kc0 + DEPTH - BI) return;      // (timing experiments: gz_igemm2_kstep.h)
        if (GZ2_SAMECHUNK && kc >= kc0 + DEPTH - BI) kc = kc0;
        float* sb = ring + st * STAGE;
        if (p < NPA) al.issue_piece(kc, sb + B_ELEMS, p, live);
        else bl.issue_piece(kc, sb, p - NPA, live);
    };
    // k-step S of the stage whose byte offset is `so`: raw fragments
    auto fetch_m = [&](auto Sc, auto Mc, uint32_t so, float (&af)[TM], float (&bf)[TN]) {      // multi-mode loaders
        constexpr int S = decltype(Sc)::value, MD = decltype(Mc)::value;
        constexpr bool PL = AL::step_plain(MD, S);
        constexpr unsigned MK = AL::step_mask(MD, S);
        constexpr int AO = LDA * AL::step_arow(MD, S) * 4, BO = AL::step_brow(MD, S) * LDB * 4;
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = lds_rd<AO>((PL ? a_addrB[i] : a_addr[i]) + so);
        if constexpr ((MK & 1u) != 0) bf[0] = lds_rd<BO>(b_addr + so);
        if constexpr (TN >= 2 && (MK & 2u) != 0) bf[1] = lds_rd<BO + 128>(b_addr + so);
        if constexpr (TN == 4 && (MK & 4u) != 0) bf[2] = lds_rd<BO + 256>(b_addr + so);
        if constexpr (TN == 4 && (MK & 8u) != 0) bf[3] = lds_rd<BO + 384>(b_addr + so);
    };
    // the first fragments of chunk `kc`, in that chunk's mode
    auto fetch_first = [&](int kc, uint32_t so, float (&af)[TM], float (&bf)[TN]) {
        if constexpr (DM) {
            if (al.mode_of(kc) == 0) fetch_m(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, so, af, bf);
            else fetch_m(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, so, af, bf);
        }
    };
    auto fetch = [&](auto Sc, auto Kc, uint32_t so, float (&af)[TM], float (&bf)[TN]) {
        // (k-step Sc of the GROUP: chunk JO / (STAGE * 4) of it, that chunk's k-step S; skip mode Kc, < 0: every block)
        constexpr int S = decltype(Sc)::value % STEPS, JO = decltype(Sc)::value / STEPS * STAGE * 4;
        constexpr unsigned SK = decltype(Kc)::value < 0 ? 0u : AL::skip_mask(decltype(Kc)::value, S);
        constexpr int AO = (RS ? LDA : 2 * LDA) * S * 4 + JO, BO = 2 * S * LDB * 4 + JO;
        static_assert(AO + 2 * LDA * 4 < 65536 && BO + 512 < 65536, "ds_read immediate offsets");
        if (GZ2_NOFETCH && so != 0xFFFFFFFFu) return;
        // immediate offsets only: no VALU address arithmetic inside the loop (`a_addr[i] + so` is per-chunk)
        if constexpr (FR) {
            constexpr int FO = (S >> 1) * 2 * AL::OW_C * 4 + JO;
            if constexpr (!(SK & 1u)) af[0] = lds_rd<FO>(((S & 1) ? a_odd[0] : a_addr[0]) + so);
            af[1] = lds_rd<FO>(((S & 1) ? a_odd[1] : a_addr[1]) + so);
            af[2] = lds_rd<FO>(((S & 1) ? a_odd[2] : a_addr[2]) + so);
            if constexpr (!(SK & 8u)) af[3] = lds_rd<FO>(((S & 1) ? a_odd[3] : a_addr[3]) + so);
        } else {
            if constexpr (!(SK & 1u)) af[0] = lds_rd<AO>(a_addr[0] + so);
            af[1] = lds_rd<AO>(a_addr[1] + so);
            af[2] = lds_rd<AO>(a_addr[2] + so);
            if constexpr (!(SK & 8u)) af[3] = lds_rd<AO>(a_addr[3] + so);
        }
        bf[0] = lds_rd<BO>(b_addr + so);
        if constexpr (TN >= 2) bf[1] = lds_rd<BO + 128>(b_addr + so);
        if constexpr (TN == 4) {
            bf[2] = lds_rd<BO + 256>(b_addr + so);
            bf[3] = lds_rd<BO + 384>(b_addr + so);
        }
    };

    if (kcA < kcB) {
        // chunks 0 .. DEPTH-BI-1 into the stages of those numbers; the first group has landed when all but the others'
        // pieces have
#pragma unroll
        for (int d = 0; d < DEPTH - BI; ++d)
#pragma unroll
            for (int p = 0; p < NP; ++p) issue_piece(kc0 + d, d, p, kc0 + d < kc1);
        // lgkmcnt(0) as well: the zeroed pad columns / A_EXTRA region above were plain ds_writes, and gfx950's back-off
        // barrier does not wait for a wavefront's outstanding LDS operations by itself
        if constexpr (GZ2_NO_LGKM_PROLOGUE) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWAIT) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NWAIT) : "memory");
        __builtin_amdgcn_s_barrier();
        probe.loop_start();
        float af[2][TM], bf[2][TN];
        if constexpr (DM) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[q][j] = 0.f;
            fetch_first(kc0, 0u, af[0], bf[0]);
        } else {
            if constexpr (PSK) {          // (a skipped block's fragment register is never read; it must still be a value)
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int i = 0; i < TM; ++i) af[q][i] = 0.f;
            }
            fetch(std::integral_constant<int, 0>{}, std::integral_constant<int, -1>{}, 0u, af[0], bf[0]);
        }
        lgkm_done(af[0], bf[0]);
        int stage = 0;
        // (pad-skip, transposed form: block 0 is padding only in the k-steps of one parity)
        bool b0_odd = true, b0_even = true;
        if constexpr (PSB) {
            b0_odd = al.block0_skip_parity() == 0;
            b0_even = !b0_odd;
        }
        // (dual mode: the row-shared chunks and the plain chunks are TWO loops, one after the other -- a per-chunk branch
        // between the two k-step forms inside one loop made the register allocator spill accumulators in every iteration)
        auto run_chunks = [&](int k_from, int k_to, auto Mc) {
        // (`stage` counts GROUPS of BI stages; a last group that is not full runs its missing chunks as zeros, like the
        // chunks past kc1 of a wave group)
        for (int kc = k_from; kc < k_to; kc += BI) {
            int s1 = stage + 1; if (s1 >= GROUPS) s1 -= GROUPS;
            int s2 = stage - 1; if (s2 < 0) s2 += GROUPS;         // the stages group kc-BI was read from: group kc+DEPTH-BI's
            const uint32_t so = (uint32_t)(stage * BI * STAGE * 4), sno = (uint32_t)(s1 * BI * STAGE * 4);
            const bool more = kc + DEPTH - BI < kc1, more1 = kc + DEPTH - BI + 1 < kc1;
            auto kstep = [&](auto Sc) {
                constexpr int S = decltype(Sc)::value;
                constexpr int MD = decltype(Mc)::value;          // multi-mode loaders: this loop's k-step form
                constexpr int c = S & 1, n = c ^ 1;
                constexpr unsigned SK = AL::skip_mask(MD, S % STEPS);      // pad-skip loaders: blocks left out (0 or 3)
                static_assert((SK & ~9u) == 0, "the k-step leaves out block 0 or block 3");
                auto mfma_row = [&](f32x16 (&cc)[TN], float a, const float (&b)[TN]) {
                    if constexpr (DM) {           // the accumulator blocks (output phases) this mode's taps feed
                        constexpr unsigned MK = AL::step_mask(MD, S);
                        if constexpr (MK == (TN == 4 ? 15u : 3u)) gz::mfma_row(cc, a, b);
                        else {
                            if constexpr ((MK & 1u) != 0) gz::mfma_one(cc[0], a, b[0]);
                            if constexpr (TN >= 2 && (MK & 2u) != 0) gz::mfma_one(cc[1], a, b[1]);
                            if constexpr (TN == 4 && (MK & 4u) != 0) gz::mfma_one(cc[2], a, b[2]);
                            if constexpr (TN == 4 && (MK & 8u) != 0) gz::mfma_one(cc[3], a, b[3]);
                        }
                    } else gz::mfma_row(cc, a, b);
                };
                auto block0 = [&]() {
                    if constexpr (PSB) {
                        if ((S & 1) ? b0_odd : b0_even) mfma_row(acc[0], af[c][0], bf[c]);
                    } else if constexpr (!(SK & 1u)) mfma_row(acc[0], af[c][0], bf[c]);
                };
                auto fetch_same = [&](auto S2c, uint32_t o, float (&fa)[TM], float (&fb)[TN]) {
                    if constexpr (DM) fetch_m(S2c, Mc, o, fa, fb);
                    else fetch(S2c, Mc, o, fa, fb);
                };
                // the pieces of group kc+DEPTH-BI go out in the FIRST k-steps, PPS per step, one behind each MFMA row
                // (the stages they overwrite were last read in group kc-BI, behind its barrier), so that by the last
                // k-step exactly (DEPTH-BI) * NP are in flight: group kc+BI's, the oldest, and NWAIT behind them
                auto pieces = [&](auto Rowc) {        // behind MFMA row `Rowc` (a single piece per k-step: behind row 1)
                    constexpr int row = decltype(Rowc)::value;
                    constexpr int r = PPS == 1 ? (row == 1 ? 0 : -1) : row;
                    constexpr int q = S * PPS + r;
                    if constexpr (r >= 0 && r < PPS && q < BI * NP)
                        issue_piece(kc + DEPTH - BI + q / NP, s2 * BI + q / NP, q % NP, q / NP == 0 ? more : more1);
                };
                if constexpr (S + 1 < GSTEPS) {
                    fetch_same(std::integral_constant<int, S + 1>{}, so, af[n], bf[n]);
                    block0();
                    pieces(std::integral_constant<int, 0>{});
                    mfma_row(acc[1], af[c][1], bf[c]);
                    pieces(std::integral_constant<int, 1>{});
                    if constexpr (TM == 4) mfma_row(acc[2], af[c][2], bf[c]);
                    pieces(std::integral_constant<int, 2>{});
                    if constexpr (TM == 4 && !(SK & 8u)) mfma_row(acc[3], af[c][3], bf[c]);
                    pieces(std::integral_constant<int, 3>{});
                } else {
                    // last k-step: half of its MFMAs, then group kc+BI must have landed (all but the NWAIT pieces of
                    // the groups behind it) and every wavefront must be done with this group's fragments; the first
                    // fragments of chunk kc+BI are fetched under the other half
                    // (pad-skip: the half that loses an MFMA keeps its other one -- blocks 0, 1 in front, 2, 3 behind)
                    block0();
                    pieces(std::integral_constant<int, 0>{});
                    if constexpr (TM == 4) mfma_row(acc[1], af[c][1], bf[c]);
                    static_for<3, 1>(pieces);      // behind rows 1, 2, 3
                    probe.wait_begin();
                    if constexpr (!GZ2_NOVMWAIT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWAIT) : "memory");
                    probe.wait_end();
                    if constexpr (!GZ2_NOBARRIER) __builtin_amdgcn_s_barrier();
                    probe.barrier_end();
                    if constexpr (DM) fetch_first(kc + BI, sno, af[n], bf[n]);     // the next chunk's, in ITS mode
                    else fetch(std::integral_constant<int, 0>{}, Mc, sno, af[n], bf[n]);
                    if constexpr (TM == 4) {
                        mfma_row(acc[2], af[c][2], bf[c]);
                        if constexpr (!(SK & 8u)) mfma_row(acc[3], af[c][3], bf[c]);
                    } else {
                        mfma_row(acc[1], af[c][1], bf[c]);
                    }
                }
                probe.template kstep_end<S>();
                lgkm_done(af[n], bf[n]);
            };
            static_for<GSTEPS>(kstep);
            stage = s1;
        }
        };
        if constexpr (DM) {          // one loop per mode, in order (a mode switch inside ONE loop spilled accumulators)
            run_chunks(kc0, min(kend, al.bound[0]), std::integral_constant<int, 0>{});
            run_chunks(max(kc0, al.bound[0]), kend, std::integral_constant<int, 1>{});
        } else {
            run_chunks(kc0, kend, std::integral_constant<int, 0>{});
        }
        // drain the LDS-DMA queue; MFMA results must have retired before the epilogue's v_accvgpr_read (the hazard
        // recognizer does not look inside the asm statements)
        asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");
        probe.loop_end(tid, kg, kend - kc0);
    }

    if constexpr (KG == 2) {
        // the two halves of the reduction meet: group 1 parks its accumulators in LDS (the rings are done with:
        // [register][thread], conflict-free), group 0 adds them -- a + b, the same bits whichever group held which half
        // -- and alone runs the epilogue
        __syncthreads();
        float* const park = smem2;
        if (kg == 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) park[((i * TN + j) * 16 + r) * NT + tid] = acc[i][j][r];
        }
        __syncthreads();
        if (kg == 1) return;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += park[((i * TN + j) * 16 + r) * NT + tid];
    }
    if constexpr (PSK) {
        // KG = 1: every wavefront is done with the rings.  KG = 2: the slots are columns of the park that only this
        // wavefront's counterpart wrote and only this wavefront read.
        if constexpr (KG == 1) __syncthreads();
        unpermute_padskip<TM, TN>(acc, smem2, tid, al.block_mirror());
    }
    if (GZ2_NOSTORE && acc[0][0][0] != 123456.789f) {      // (timing experiment: one store kept, the accumulators stay live)
    } else if (gm.slab)
        store_slab<Epi::SWAP, TM, TN>(gm, acc, tile_m * Cfg::BM + wm * TM * 32, tile_n * Cfg::BN + wn * TN * 32, lane,
                                      gm.var_chunks ? gm.phase_slab0[y] + z : y * (int)gridDim.z + z);
    else
        Epi::template store<TM, TN>(pe, acc, tile_m * Cfg::BM + wm * TM * 32, tile_n * Cfg::BN + wn * TN * 32,
                                    lane, y, z);
    probe.exit(tid, kc1 - kc0, TM * TN);
}

// Which launches run two wave groups per workgroup (igemm2_kernel<.., KG = 2>): the k4 s2 p1 loaders of the DCGAN
// layers, 128- or 64-wide tiles, when the grid gives a CU at most ONE workgroup and each group still has a reduction
// worth pipelining.  Pure host logic: gz_conv2d_plan reports it, tests/golden/dispatch_plan.json pins it.
template <class Cfg, class AL>
constexpr bool igemm2_kg2_built() {
    return Cfg::TN <= 2 && Cfg::WM * Cfg::WN == 4 && Cfg::WN == 2 && !AL::DUALMODE &&
           (AL::ROWSHARE || AL::FWDROWS || AL::TAPGATHER);
}
inline bool igemm2_use_kg2(long long workgroups, int chunks_per_workgroup) {
    if (knobs().no_kg2) return false;
    return workgroups <= cus() && chunks_per_workgroup >= knobs().kg2_min_chunks;
}

// same contract as launch_igemm
template <class Cfg, class AL, class BL, class Epi>
inline int launch_igemm2(const typename AL::Params& pa, const typename BL::Params& pb, const typename Epi::Params& pe,
                         int M, int N, int K, int ny, int splits, hipStream_t stream, float* slab = nullptr,
                         const int* phase_chunks = nullptr) {
    static_assert(Epi::SWAP, "transposed accumulators (lanes along m)");
    GridPlan g = make_grid(Cfg::BM, Cfg::BN, M, N, K, ny, splits, slab, phase_chunks);
    // stagger (see the kernel), an experiment that stays OFF: GZ_IGEMM2_STAGGER=<percent of a tile>.  Measured (in-kernel
    // stamps): co-resident workgroups drift apart by themselves -- the average workgroup's loop takes 469 k cycles where
    // two in lockstep would take 524 k -- and a forced half-tile offset changes neither the layer (143.3 -> 142.8
    // TFLOP/s) nor the step (21.43 vs 21.40 ms).  What a launch does lose is its ramp: ~19 us until the first
    // round's prologues are through plus the last round's tail, ~6 % of a 1 ms launch.
    const int stagger_pct = knobs().igemm2_stagger;
    g.gm.stagger = (Cfg::OCC == 2 && g.nz == 1 && g.grid.x >= 1536)
                       ? (int)((long long)g.gm.chunks * 8 * Cfg::TM * Cfg::TN * 64 * 2 * stagger_pct / 100) : 0;
    bool kg2 = false, ok = false;
#ifdef GZ2_STAMPS
    gz2_last_stamps() = HIP_SYMBOL(gz2_stamps);      // (this unit's copy of the array)
#endif
    if constexpr (igemm2_kg2_built<Cfg, AL>()) {
        kg2 = igemm2_use_kg2((long long)g.grid.x * g.nz, g.gm.chunks_per_split);
        if (kg2)
            ok = launch_big_lds<igemm2_kernel<Cfg, AL, BL, Epi, 2>>(g.grid, 2 * NT, igemm2_lds_bytes_kg2<Cfg, AL, BL>(), stream,
                                                                   pa, pb, pe, g.gm);
    }
    if (!kg2)      // (knob igemm2_lds, an experiment: extra bytes throttle the workgroups per CU)
        ok = launch_big_lds<igemm2_kernel<Cfg, AL, BL, Epi>>(g.grid, NT, igemm2_lds_bytes<Cfg, AL, BL>() + (size_t)knobs().igemm2_lds,
                                                            stream, pa, pb, pe, g.gm);
    if (ok && g.gm.slab) launch_splitk_finish<Epi>(g, M, N, ny, pe, stream);
    return launch_status();
}

}  // namespace gz
