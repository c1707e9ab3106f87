// Part of the fp32 implicit-GEMM core (see gz_igemm.h), igemm2 skeleton: the weight-gradient kernels igemm2r_kernel (operands
// through registers) and igemm2w_kernel (both operands by LDS-DMA), their loaders and launchers.
#pragma once
#include "gz_igemm2.h"
#include "gz_igemm2_kstep.h"

namespace gz {

// The same skeleton for operands that cannot arrive by LDS-DMA (weight gradient: both operands are
// reduction-contiguous in memory and are transposed on their way into LDS): loaders with the igemm_kernel interface
// issue() (global -> registers, at the top of a chunk) / commit() (registers -> LDS, late in the chunk), TWO stages
// (the stage written in chunk kc was last read in chunk kc-1, behind its barrier).  The compiler places the global
// loads and ds_writes (and the vmcnt wait between them) between the hand-ordered MFMA clusters; the wavefront drains
// its LDS queue (its own ds_writes) in front of the chunk's barrier.  Epilogue: D[m][n], lanes along n.
template <class Cfg, class AL, class BL, class Epi>
__global__ __launch_bounds__(NT, Cfg::OCC) void igemm2r_kernel(typename AL::Params pa, typename BL::Params pb,
                                                               typename Epi::Params pe, GridMap gm) {
    constexpr int LDA = AL::LD, LDB = BL::LD;
    constexpr int TM = Cfg::TM, TN = Cfg::TN;
    static_assert(TM == 4 && (TN == 2 || TN == 4) && !Epi::SWAP, "fragment registers of the hand-ordered k-step");
    constexpr int A_ELEMS = BK * LDA, B_ELEMS = BK * LDB;
    constexpr int STAGE = A_ELEMS + B_ELEMS;
    extern __shared__ __attribute__((aligned(16))) float smem2[];
    float* const ring = smem2;                           // stage i: [B image][A image]

    const int tid = threadIdx.x;
    const int nwg = gridDim.x;
    int bid = blockIdx.x;
    if (!gm.no_swizzle) {
        const int q = nwg >> 3, rr = nwg & 7, x = bid & 7, i = bid >> 3;
        bid = (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + i;
    }
    const int y = bid % gm.ny;
    bid /= gm.ny;
    const int tile_n = bid % gm.tiles_n;
    const int tile_m = bid / gm.tiles_n;
    const int z = blockIdx.z;
    const int kc0 = z * gm.chunks_per_split;
    const int kc1 = min(gm.chunks, kc0 + gm.chunks_per_split);

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
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring;
    const uint32_t a_addr = lds0 + (uint32_t)(B_ELEMS + half * LDA + wm * TM * 32 + l32) * 4u;
    const uint32_t b_addr = lds0 + (uint32_t)(half * LDB + wn * TN * 32 + l32) * 4u;
    constexpr int STEPS = BK / 2;
    auto fetch = [&](auto Sc, uint32_t so, float (&af)[TM], float (&bf)[TN]) {
        constexpr int S = decltype(Sc)::value;
        constexpr int AO = 2 * LDA * S * 4, BO = 2 * LDB * S * 4;
        af[0] = lds_rd<AO>(a_addr + so);
        af[1] = lds_rd<AO + 128>(a_addr + so);
        af[2] = lds_rd<AO + 256>(a_addr + so);
        af[3] = lds_rd<AO + 384>(a_addr + so);
        bf[0] = lds_rd<BO>(b_addr + so);
        if constexpr (TN >= 2) bf[1] = lds_rd<BO + 128>(b_addr + so);
        if constexpr (TN == 4) {
            bf[2] = lds_rd<BO + 256>(b_addr + so);
            bf[3] = lds_rd<BO + 384>(b_addr + so);
        }
    };

    if (kc0 < kc1) {
        al.issue(kc0);
        bl.issue(kc0);
        al.commit(ring + B_ELEMS);
        bl.commit(ring);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        float af[2][TM], bf[2][TN];
        fetch(std::integral_constant<int, 0>{}, 0u, af[0], bf[0]);
        lgkm_done(af[0], bf[0]);
        int stage = 0;
        for (int kc = kc0; kc < kc1; ++kc) {
            const uint32_t so = (uint32_t)(stage * STAGE * 4), sno = (uint32_t)((stage ^ 1) * STAGE * 4);
            float* const nxt = ring + (stage ^ 1) * STAGE;
            const bool more = kc + 1 < kc1;
            auto kstep = [&](auto Sc) {
                constexpr int S = decltype(Sc)::value;
                constexpr int c = S & 1, n = c ^ 1;
                if constexpr (S == 0) {
                    if (more) {
                        al.issue(kc + 1);
                        bl.issue(kc + 1);
                    }
                }
                if constexpr (S + 1 < STEPS) {
                    fetch(std::integral_constant<int, S + 1>{}, so, af[n], bf[n]);
                    mfma_row_mn(acc[0], af[c][0], bf[c]);
                    mfma_row_mn(acc[1], af[c][1], bf[c]);
                    if constexpr (S == STEPS - 3) { if (more) al.commit(nxt + B_ELEMS); }
                    if constexpr (S == STEPS - 2) { if (more) bl.commit(nxt); }
                    mfma_row_mn(acc[2], af[c][2], bf[c]);
                    mfma_row_mn(acc[3], af[c][3], bf[c]);
                    lgkm_done(af[n], bf[n]);
                } else {
                    mfma_row_mn(acc[0], af[c][0], bf[c]);
                    mfma_row_mn(acc[1], af[c][1], bf[c]);
                    // this wavefront's ds_writes of the next stage are done (lgkm_done of the previous k-step waited
                    // for the whole LDS queue); every wavefront is past its last fragment read of this stage
                    __builtin_amdgcn_s_barrier();
                    fetch(std::integral_constant<int, 0>{}, sno, af[n], bf[n]);
                    mfma_row_mn(acc[2], af[c][2], bf[c]);
                    mfma_row_mn(acc[3], af[c][3], bf[c]);
                    lgkm_done(af[n], bf[n]);
                }
            };
            static_for<STEPS>(kstep);
            stage ^= 1;
        }
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    }
    Epi::template store<TM, TN>(pe, acc, tile_m * Cfg::BM + wm * TM * 32, tile_n * Cfg::BN + wn * TN * 32, lane, y, z);
}

// ---- weight gradient of the k4 s2 p1 convolution with BOTH operands arriving by LDS-DMA (igemm2w) -----------------------
// dW[ko][(c, ky, kx)] = sum over pixels (n, oy, ox) of  dy[n][ko][oy][ox] * x[n][c][2*oy - 1 + ky][2*ox - 1 + kx].
// Both operands are reduction-contiguous in memory, which is why igemm2r_kernel transposes them through registers
// (16 + 8 dword loads, 12 ds_writes and their address / mask VALU per wavefront and chunk, all paid in MFMA issue
// slots).  Here nothing is transposed on the way in:
//   A  the chunk's 16 consecutive pixels of a dy channel are 64 contiguous bytes: the LDS image is [m][16 k] (four
//      16-byte quads per row, the quad order XOR-swizzled with (m >> 2) & 3 so that the 16 lanes of a ds_read_b128
//      group hit 16 different slots), and the lane (m, half) takes its operands with ONE ds_read_b128 per four
//      k-steps.  The reduction index inside a chunk is enumerated so that this works: k-step s = 4*g + t of
//      half-wave h multiplies pixel k = 8*g + 4*h + t (the order of a sum's terms is free as long as A and B agree);
//   B  the raw input rows the chunk's pixels touch -- per input channel 2*R + 2 rows of 2*CW + 8 columns (R x CW =
//      the chunk's pixel rectangle: 1 x 16, 2 x 8 or 4 x 4; four columns either side so that every 16-byte quad is
//      entirely inside or entirely outside the image, outside = out-of-range lanes = zeros) -- land as they are, and
//      the lane (c, ky, kx) reads  image[c][2*r + ky][2*x + kx + 3]  with r, x from k: row / channel pitches are chosen
//      so that the 32 (c, ky, kx) lanes of a half-wave fall on 32 different banks, and every k-step's offset is an
//      immediate.
// No VALU and no ds_write in the k-steps (per chunk: a dozen VALU instructions for the stage offsets and the halo
// flags of the two B pieces); 24 LDS reads per chunk and wavefront instead of 48.  Ring, counted vmcnt,
// barrier placement and the epilogue (D[m][n], lanes along n, split-K slabs through the epilogue) as above.

struct Wg2Params {
    const float* x;          // image side  [N, C, H, W], H = 2*OH, W = 2*OW
    const float* y;          // feature side [N, K, OH, OW]
    ConvShape s;
    FastDiv div_ohw, div_ow;
};

template <int BM>
struct WgDyA2 {
    static constexpr int PIECES = BM / 64;                 // per wavefront and chunk (BM rows x 4 quads / 64 lanes / 4)
    static constexpr int ELEMS = BM * BK;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff[PIECES];
    int wave;
    __device__ __forceinline__ void init(const Wg2Params& p, int tile, int tid) {
        const ConvShape& s = p.s;
        rsrc = make_rsrc(p.y, (uint32_t)s.N * s.K * s.OH * s.OW * 4u);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            const int gq = (wave * PIECES + j) * 64 + lane;       // LDS quad
            const int ml = gq >> 2, qk = (gq & 3) ^ ((ml >> 2) & 3);
            const int m = tile * BM + ml;
            voff[j] = m < s.K ? (uint32_t)(m * s.OH * s.OW + 4 * qk) * 4u : OOB;
        }
    }
    __device__ __forceinline__ void issue_piece(float* stage, int j, uint32_t soff) {
        bload_lds16(rsrc, stage + (wave * PIECES + j) * 256, voff[j], soff);
    }
};

template <int BN, int CW>
struct WgImgB2 {
    static_assert(CW == 4 || CW == 8 || CW == 16, "chunk rectangles 4 x 4, 2 x 8, 1 x 16");
    static constexpr int R = 16 / CW, IMG_ROWS = 2 * R + 2;
    static constexpr int RQ = CW == 4 ? 5 : (2 * CW + 8) / 4;              // quads per image row (CW 4: one pad quad)
    static constexpr int CHQ = CW == 16 ? 41 : CW == 8 ? 37 : 52;           // quads per channel (pad quads at its end)
    static constexpr int RP = RQ * 4, CHP = CHQ * 4;                        // pitches in floats: (8*ky + 4*c + kx) mod 32,
                                                                            // (24*ky + 20*c + kx), (20*ky + 16*c + kx)
                                                                            // are 32 different banks
    static constexpr int NCH = BN / 16;
    static constexpr int PIECES = (NCH * CHQ + 255) / 256;                  // per wavefront and chunk
    static constexpr int ELEMS = PIECES * 4 * 256;
    // float offsets of the fragment read of k-step s = 4*g + t, half-wave h: pixel k = 8*g + 4*h + t = (r, x)
    static constexpr int HOFF = CW == 4 ? 2 * RP : 8, GOFF = CW == 16 ? 16 : CW == 8 ? 2 * RP : 4 * RP, TOFF = 2;
    static constexpr int ROWS_PER_CHUNK = R, TAPS = 16;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff[PIECES], flags[PIECES];
    int wave;
    // float offset (inside the B image) of the lane that owns column `col` of the tile: (c, ky, kx) at pixel (0, 0)
    __device__ __forceinline__ int lane_base(int tile, int col) const {
        return (col >> 4) * CHP + ((col >> 2) & 3) * RP + (col & 3) + 3;
    }
    __device__ __forceinline__ void init(const Wg2Params& p, int tile, int tid) {
        const ConvShape& s = p.s;
        // per-lane offsets are relative to the chunk's first input pixel (2*oy0, 2*ox0) and reach one row up and four
        // columns left: the descriptor's base is moved back by that much (never dereferenced there: flagged lanes)
        const int shift = s.W + 4;
        rsrc = make_rsrc(p.x - shift, (uint32_t)(s.N * s.C * s.H * s.W + shift) * 4u);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            const int gq = (wave * PIECES + j) * 64 + lane;
            const int cl = gq / CHQ, rem = gq - cl * CHQ;
            const int row = rem / RQ, q = rem - row * RQ;
            const int c = tile * NCH + cl;
            const int col0 = 4 * q - 4;
            const bool inside = cl < NCH && c < s.C && row < IMG_ROWS && col0 <= 2 * CW;
            voff[j] = inside ? (uint32_t)((c * s.H + row - 1) * s.W + col0 + shift) * 4u : OOB;
            flags[j] = (row == 0 ? 1u : 0u) | (row == IMG_ROWS - 1 ? 2u : 0u) | (col0 < 0 ? 4u : 0u) |
                       (col0 >= 2 * CW ? 8u : 0u);
        }
    }
    __device__ __forceinline__ void issue_piece(float* stage, int j, uint32_t soff, uint32_t cond) {
        bload_lds16(rsrc, stage + (wave * PIECES + j) * 256, (flags[j] & cond) ? OOB : voff[j], soff);
    }
};

// The same raw-row image for any geometry with W = S * OW, H = S * OH (5x5 s2 p2, 3x3 s1 p1): S * (R - 1) + KH rows per
// channel, the column origin LP = P rounded up to a quad left of the chunk's first input column.  A 32-column block is
// no longer a whole number of channels (25 or 9 taps each), so a lane's (c, ky, kx) differs from block to block: the
// kernel keeps one base address per block.  Pitches from tools/wg_banks.py: 25 + 7 taps of two channels cannot tile the
// 32 banks with quad-aligned rows, the best layouts are 2-way on a few lanes.
template <int BN, int CW, int KH, int KW, int S, int P>
struct WgImgBG {
    static_assert(CW == 4 || CW == 8 || CW == 16, "chunk rectangles 4 x 4, 2 x 8, 1 x 16");
    static constexpr int R = 16 / CW, TAPS = KH * KW;
    static constexpr int LP = (P + 3) / 4 * 4;
    static constexpr int IMG_ROWS = S * (R - 1) + KH;
    static constexpr int RQ0 = (S * (CW - 1) + KW - 1 - P + LP) / 4 + 1;
    static constexpr bool K5 = KH == 5 && KW == 5 && S == 2 && P == 2, K3 = KH == 3 && KW == 3 && S == 1 && P == 1;
    static_assert(K5 || K3, "pitches are tabulated per geometry (tools/wg_banks.py)");
    static constexpr int RQ = RQ0 + ((K5 && CW == 4) ? 1 : 0);
    static constexpr int RP = RQ * 4;
    static constexpr int CHP = IMG_ROWS * RP + 4 * (K5 ? (CW == 16 ? 0 : CW == 8 ? 4 : 2) : (CW == 16 ? 3 : CW == 8 ? 1 : 0));
    static constexpr int CHQ = CHP / 4;
    static constexpr int NCH = (BN % TAPS == 0) ? BN / TAPS : (BN - 1) / TAPS + 2;      // channels a tile's columns can touch
    static constexpr int PIECES = (NCH * CHQ + 255) / 256;
    static constexpr int ELEMS = PIECES * 4 * 256;
    static constexpr int TOFF = S, HOFF = CW == 4 ? S * RP : 4 * S, GOFF = CW == 16 ? 8 * S : CW == 8 ? S * RP : 2 * S * RP;
    static constexpr int ROWS_PER_CHUNK = R;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff[PIECES], flags[PIECES];
    int wave;
    __device__ __forceinline__ int lane_base(int tile, int col) const {
        const int n = tile * BN + col;
        const int c = n / TAPS, tap = n - c * TAPS;
        int cl = c - (tile * BN) / TAPS;
        if (cl > NCH - 1) cl = NCH - 1;                  // columns past N (masked by the epilogue) stay inside the image
        const int ky = tap / KW, kx = tap - ky * KW;
        return cl * CHP + ky * RP + kx - P + LP;
    }
    __device__ __forceinline__ void init(const Wg2Params& p, int tile, int tid) {
        const ConvShape& s = p.s;
        const int shift = P * s.W + LP;
        rsrc = make_rsrc(p.x - shift, (uint32_t)(s.N * s.C * s.H * s.W + shift) * 4u);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int c_lo = (tile * BN) / TAPS;
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            const int gq = (wave * PIECES + j) * 64 + lane;
            const int cl = gq / CHQ, rem = gq - cl * CHQ;
            const int row = rem / RQ, q = rem - row * RQ;
            const int c = c_lo + cl;
            const int col0 = 4 * q - LP;
            const bool inside = cl < NCH && c < s.C && row < IMG_ROWS && col0 <= S * CW;
            voff[j] = inside ? (uint32_t)((c * s.H + row - P) * s.W + col0 + shift) * 4u : OOB;
            flags[j] = (row < P ? 1u : 0u) | (row >= S * R + P ? 2u : 0u) | (col0 < 0 ? 4u : 0u) |
                       (col0 >= S * CW ? 8u : 0u);
        }
    }
    __device__ __forceinline__ void issue_piece(float* stage, int j, uint32_t soff, uint32_t cond) {
        bload_lds16(rsrc, stage + (wave * PIECES + j) * 256, (flags[j] & cond) ? OOB : voff[j], soff);
    }
};

template <class Cfg, class BL, class Epi>
__global__ __launch_bounds__(NT, Cfg::OCC) void igemm2w_kernel(Wg2Params p, typename Epi::Params pe, GridMap gm) {
    using AL = WgDyA2<Cfg::BM>;
    constexpr int CW = 16 / BL::ROWS_PER_CHUNK;
    constexpr int TM = Cfg::TM, TN = Cfg::TN;
    static_assert(TM == 4 && TN == 2 && !Epi::SWAP, "fragment registers of the hand-ordered k-step");
    constexpr int A_ELEMS = AL::ELEMS, B_ELEMS = BL::ELEMS, STAGE = A_ELEMS + B_ELEMS;
    extern __shared__ __attribute__((aligned(16))) float smem2[];
    float* const ring = smem2;                           // stage i: [B image][A image]

    const int tid = threadIdx.x;
    const int nwg = gridDim.x;
    int bid = blockIdx.x;
    if (!gm.no_swizzle) {
        const int q = nwg >> 3, rr = nwg & 7, x = bid & 7, i = bid >> 3;
        bid = (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + i;
    }
    const int tile_n = bid % gm.tiles_n;
    const int tile_m = bid / gm.tiles_n;
    const int z = blockIdx.z;
    const int kc0 = z * gm.chunks_per_split;
    const int kc1 = min(gm.chunks, kc0 + gm.chunks_per_split);

    AL al;
    BL bl;
    al.init(p, tile_m, tid);
    bl.init(p, tile_n, tid);

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
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring;
    // A: row m = 16 floats, quad (2*g + half) ^ swizzle; the swizzle (m >> 2) & 3 only depends on the lane
    const int swz = (l32 >> 2) & 3;
    uint32_t a_addr[2];
#pragma unroll
    for (int g = 0; g < 2; ++g)
        a_addr[g] = lds0 + (uint32_t)(B_ELEMS + (wm * TM * 32 + l32) * BK + (((2 * g + half) ^ swz) << 2)) * 4u;
    // B: this lane's (c, ky, kx) in each of its two 32-column blocks
    uint32_t b_addr[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
        b_addr[j] = lds0 + (uint32_t)(bl.lane_base(tile_n, wn * TN * 32 + j * 32 + l32) + half * BL::HOFF) * 4u;

    constexpr int NPA = AL::PIECES, NPB = BL::PIECES, NP = NPA + NPB, STEPS = BK / 2;
    static_assert(NP <= STEPS, "at most one LDS-DMA piece per k-step");
    const ConvShape& s = p.s;
    const int OHW = s.OH * s.OW;
    uint32_t soff_a = 0, soff_b = 0, cond = 0;          // of the chunk being issued
    auto locate = [&](int kc, bool live) {
        const uint32_t p0 = (uint32_t)kc * BK;
        const uint32_t n = fdiv(p0, p.div_ohw);
        const uint32_t rem = p0 - n * (uint32_t)OHW;
        const uint32_t oy0 = fdiv(rem, p.div_ow);
        const uint32_t ox0 = rem - oy0 * (uint32_t)s.OW;
        soff_a = live ? (n * (uint32_t)(s.K * OHW) + rem) * 4u : SOFF_OOB;
        const uint32_t st = (uint32_t)(s.H / s.OH);           // stride (H = S * OH)
        soff_b = live ? (n * (uint32_t)(s.C * s.H * s.W) + st * oy0 * (uint32_t)s.W + st * ox0) * 4u : SOFF_OOB;
        cond = (oy0 == 0 ? 1u : 0u) | ((int)oy0 + BL::ROWS_PER_CHUNK == s.OH ? 2u : 0u) | (ox0 == 0 ? 4u : 0u) |
               ((int)ox0 + CW == s.OW ? 8u : 0u);
    };
    auto issue_piece = [&](int st, int q) {
        float* sb = ring + st * STAGE;
        if (q < NPA) al.issue_piece(sb + B_ELEMS, q, soff_a);
        else bl.issue_piece(sb, q - NPA, soff_b, cond);
    };
    auto fetch_a = [&](auto Gc, uint32_t so, f32x4 (&af)[TM]) {
        constexpr int G = decltype(Gc)::value;
        af[0] = lds_rd4<0>(a_addr[G] + so);
        af[1] = lds_rd4<32 * BK * 4>(a_addr[G] + so);
        af[2] = lds_rd4<64 * BK * 4>(a_addr[G] + so);
        af[3] = lds_rd4<96 * BK * 4>(a_addr[G] + so);
    };
    auto fetch_b = [&](auto Sc, uint32_t so, float (&bf)[TN]) {
        constexpr int S = decltype(Sc)::value;
        constexpr int BO = ((S >> 2) * BL::GOFF + (S & 3) * BL::TOFF) * 4;
        bf[0] = lds_rd<BO>(b_addr[0] + so);
        bf[1] = lds_rd<BO>(b_addr[1] + so);
    };

    if (kc0 < kc1) {
        locate(kc0, true);
#pragma unroll
        for (int q = 0; q < NP; ++q) issue_piece(0, q);
        locate(kc0 + 1, kc0 + 1 < kc1);
#pragma unroll
        for (int q = 0; q < NP; ++q) issue_piece(1, q);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP) : "memory");
        __builtin_amdgcn_s_barrier();
        f32x4 af[2][TM];
        float bf[2][TN];
        fetch_a(std::integral_constant<int, 0>{}, 0u, af[0]);
        fetch_b(std::integral_constant<int, 0>{}, 0u, bf[0]);
        lgkm_done(af[0], bf[0]);
        int stage = 0;
        for (int kc = kc0; kc < kc1; ++kc) {
            int s1 = stage + 1; if (s1 >= STAGES2) s1 -= STAGES2;
            int s2 = s1 + 1; if (s2 >= STAGES2) s2 -= STAGES2;
            const uint32_t so = (uint32_t)(stage * STAGE * 4), sno = (uint32_t)(s1 * STAGE * 4);
            locate(kc + 2, kc + 2 < kc1);
            auto kstep = [&](auto Sc) {
                constexpr int S = decltype(Sc)::value;
                constexpr int c = S & 1, n = c ^ 1, g = S >> 2, t = S & 3;
                if constexpr (S + 1 < STEPS) {
                    fetch_b(std::integral_constant<int, S + 1>{}, so, bf[n]);
                    if constexpr (S == 0) fetch_a(std::integral_constant<int, 1>{}, so, af[1]);
                    mfma_row_mn(acc[0], af[g][0][t], bf[c]);
                    mfma_row_mn(acc[1], af[g][1][t], bf[c]);
                    if constexpr (S < NP) issue_piece(s2, S);
                    mfma_row_mn(acc[2], af[g][2][t], bf[c]);
                    mfma_row_mn(acc[3], af[g][3][t], bf[c]);
                    if constexpr (S == 0) lgkm_done(af[1], bf[n]);
                    else lgkm_done(bf[n]);
                } else {
                    mfma_row_mn(acc[0], af[g][0][t], bf[c]);
                    mfma_row_mn(acc[1], af[g][1][t], bf[c]);
                    if constexpr (S < NP) issue_piece(s2, S);
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP) : "memory");
                    __builtin_amdgcn_s_barrier();
                    fetch_b(std::integral_constant<int, 0>{}, sno, bf[n]);
                    fetch_a(std::integral_constant<int, 0>{}, sno, af[0]);
                    mfma_row_mn(acc[2], af[g][2][t], bf[c]);
                    mfma_row_mn(acc[3], af[g][3][t], bf[c]);
                    lgkm_done(af[0], bf[n]);
                }
            };
            static_for<STEPS>(kstep);
            stage = s1;
        }
        asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    }
    Epi::template store<TM, TN>(pe, acc, tile_m * Cfg::BM + wm * TM * 32, tile_n * Cfg::BN + wn * TN * 32, lane, 0, z);
}

template <class Cfg, class BL>
constexpr size_t igemm2w_lds_bytes() {
    return (size_t)STAGES2 * (WgDyA2<Cfg::BM>::ELEMS + BL::ELEMS) * 4;
}

template <class Cfg, class BL, class Epi>
inline int launch_igemm2w(const Wg2Params& p, const typename Epi::Params& pe, int M, int N, int K, int splits,
                          hipStream_t stream) {
    const GridPlan g = make_grid(Cfg::BM, Cfg::BN, M, N, K, 1, splits, nullptr, nullptr);
    constexpr size_t lds = igemm2w_lds_bytes<Cfg, BL>();
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    launch_big_lds<igemm2w_kernel<Cfg, BL, Epi>>(g.grid, NT, lds, stream, p, pe, g.gm);
    return launch_status();
}

// split-K through the epilogue's own slabs (pe.slab_stride), as launch_igemm does for the weight gradient
template <class Cfg, class AL, class BL, class Epi>
inline int launch_igemm2r(const typename AL::Params& pa, const typename BL::Params& pb, const typename Epi::Params& pe,
                          int M, int N, int K, int splits, hipStream_t stream) {
    const GridPlan g = make_grid(Cfg::BM, Cfg::BN, M, N, K, 1, splits, nullptr, nullptr);
    constexpr size_t lds = (size_t)2 * BK * (AL::LD + BL::LD) * 4;
    launch_big_lds<igemm2r_kernel<Cfg, AL, BL, Epi>>(g.grid, NT, lds, stream, pa, pb, pe, g.gm);
    return launch_status();
}

}  // namespace gz
