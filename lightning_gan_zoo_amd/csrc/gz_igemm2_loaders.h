// Part of the fp32 implicit-GEMM core (see gz_igemm.h), igemm2 skeleton: the LDS-DMA operand loaders of igemm2_kernel
// (piece-wise interface: see gz_igemm2_kernel.h).
#pragma once
#include "gz_igemm2.h"

namespace gz {

// B operand [K rows][ld], N contiguous (packed weights; plain GEMM): a piece is 256 consecutive floats of the
// [BK][BN] image = one k row (BN = 256) or two (BN = 128).  Rows past K are out of the descriptor's range (zeros).
template <int BN>
struct MContigB2 : LoaderDefaults {
    static_assert(BN == 64 || BN == 128 || BN == 256, "piece mapping");
    using Params = typename MContigLoader<BN>::Params;
    static constexpr int LD = BN, ROWS = BK;
    static constexpr int PIECES = BK * BN / 256 / 4;      // per wavefront: 4 (BN 256), 2 (128), 1 (64: four k rows each)
    static constexpr int RPP = 256 / BN;                  // k rows per piece
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff, ldb;
    int wave;
    __device__ __forceinline__ void init(const Params& p, int tile, int y, int tid) {
        rsrc = make_rsrc(p.base + (long long)y * p.batch_stride, (uint32_t)p.K * p.ld * 4u);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int f = lane * 4, r = f / BN, col = f % BN;
        const int n = tile * BN + col;
        ldb = (uint32_t)p.ld * 4u;
        voff = n < p.MN ? (uint32_t)(r * p.ld + n) * 4u : OOB;
    }
    __device__ __forceinline__ void issue_piece(int kc, float* stage, int p, bool live) {
        const int piece = wave * PIECES + p;
        bload_lds16(rsrc, stage + piece * 256, voff, live ? (uint32_t)(kc * BK + piece * RPP) * ldb : SOFF_OOB);
    }
};

// ---- pad-skip forms of the two k4 s2 p1 row loaders on 4x4 maps (ConvFwdA2<256, 4, true>, ConvDgA2<256, true>) -------
// Vertical padding arrives as zero LDS rows (out-of-range LDS-DMA lanes) and flows through the matrix pipe.  With
// m = (image, row, column) and 16 pixels per image, a 32-row MFMA block is two whole images: padded rows in every block
// for every vertical tap, no block that is padding only.  These forms stage a wavefront's 128 pixels (8 images) in the
// order (row, image, column): LDS position  wm*128 + i*32 + g*4 + b  holds pixel  (8*wm + g)*16 + 4*i + b  -- block i of a
// wavefront is map row i of its eight images -- by permuting which 16-byte quad a lane of a piece FETCHES (a quad is one
// map row at width 4; where it lands in LDS, the fragment addresses and their banks stay what they were).  A (block,
// k-step) whose vertical tap lies outside the map is then a compile-time entry (skip_mask: bit i = block i): its
// fragment read and its MFMAs are not issued, one in eight.  igemm2_kernel puts the accumulators back in pixel order
// (unpermute_padskip) before anything reads them, so every output is the same products in the same order; the dropped
// terms are +-0 added to an accumulator that is never -0.  (One deviation: a non-finite weight no longer meets the
// padding's zero, 0 * Inf = NaN, on those taps.)
__device__ __forceinline__ int padskip_quad(int q) {       // LDS quad (= forward-row segment) position -> the one staged there
    return (((q >> 5) << 3 | (q & 7)) << 2) | ((q >> 3) & 3);
}

// A operand of the k4 s2 p1 TRANSPOSED convolution, row-shared like ConvDgALoaderRow4 (a chunk's image is 8 rows =
// 4 feature channels x 2 vertical taps of UNSHIFTED feature rows; the horizontal tap is applied on the fragment
// read, the one column a shifted read takes from the neighbouring row is zeroed in the register).  One piece = one
// LDS row of 256 pixels; wavefront w stages channel w of the chunk, its two vertical taps.
// PS: the pad-skip form above (AH = AW = 4, chosen by the launcher).
template <int BM, bool PS = false>
struct ConvDgA2 : LoaderDefaults {
    static_assert(BM == 256 || BM == 512, "whole 256-pixel pieces per LDS row");
    static_assert(!PS || BM == 256, "pad-skip: a wavefront's 128 pixels are 8 whole 4x4 maps");
    static constexpr bool PADSKIP = PS;
    // k-step S has vertical tap ty = S & 1, feature row a + (py + 1) / 2 - ty: output rows of parity py = 0 have no row
    // above a = 0 (ty = 1), those of parity 1 none below a = 3 (ty = 0).  py is a launch-time fact of the workgroup, so
    // parity 1 stages its map rows in REVERSE order (block i = row 3 - i): it is block 0 either way, in the odd k-steps
    // for py = 0 and in the even ones for py = 1 -- a wave-uniform branch around block 0's MFMA (one loop per parity
    // spilled in the epilogue; igemm2_kernel).
    static constexpr bool SKIP_BLOCK0_BY_PARITY = PS;
    __device__ __forceinline__ int block0_skip_parity() const { return 1 - py_; }      // k-steps with S & 1 == this
    __device__ __forceinline__ int block_mirror() const { return py_ ? 3 : 0; }         // block i holds map row i ^ this
    using Params = typename ConvDgALoader<BM, 4, 4, 2, 1>::Params;
    // LDS rows carry 4 pad floats that are zeroed once and never written again: a lane whose shifted read would take
    // its value from the neighbouring image row reads that column instead (no v_cndmask in the loop -- an f32 MFMA
    // holds the SIMD's vector issue for its whole duration, so every VALU instruction between MFMAs costs its full
    // issue time)
    static constexpr int PPR = BM / 256;                   // pieces per LDS row
    static constexpr int LD = BM + 4, ROWS = BK / 2, PIECES = 2 * PPR;
    static constexpr int ZERO_COL = BM;
    static constexpr bool ROWSHARE = true;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff[2 * PPR];       // [vertical tap][256-pixel block]
    int wave, K, OHW, shift_half1, py_;
    __device__ __forceinline__ void init(const Params& p, int tile, int phase, int tid) {
        const ConvShape& s = p.s;
        rsrc = make_rsrc(p.y, (uint32_t)s.N * s.K * s.OH * s.OW * 4u);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        K = s.K; OHW = s.OH * s.OW;
        const int py = phase / 2, px = phase % 2;
        shift_half1 = (px + 1) / 2 - 1;
        py_ = py;
#pragma unroll
        for (int hb = 0; hb < PPR; ++hb) {
            const uint32_t m = (uint32_t)tile * BM + hb * 256 + (PS ? padskip_quad(lane) ^ (py ? 3 : 0) : lane) * 4;
            const bool m_ok = m < (uint32_t)s.N * p.AH * p.AW;
            const uint32_t n = fdiv(m, p.div_ahw);
            const uint32_t pix = m - n * (uint32_t)(p.AH * p.AW);
            const uint32_t a = fdiv(pix, p.div_aw);
            const uint32_t b = pix - a * (uint32_t)p.AW;
#pragma unroll
            for (int ty = 0; ty < 2; ++ty) {
                const int oy = (int)a + (py + 1) / 2 - ty;
                const bool ok = m_ok && (unsigned)oy < (unsigned)s.OH;
                voff[ty * PPR + hb] = ok ? (n * (uint32_t)(s.K * OHW) + (uint32_t)(oy * s.OW) + b) * 4u : OOB;
            }
        }
    }
    __device__ __forceinline__ int frag_shift(int half) const { return half ? shift_half1 : shift_half1 + 1; }
    __device__ __forceinline__ void issue_piece(int kc, float* stage, int p, bool live) {     // p = ty * PPR + block
        const int kol = kc * (BK / 4) + wave;
        bload_lds16(rsrc, stage + (wave * 2 + p / PPR) * LD + (p % PPR) * 256, voff[p],
                    (live && kol < K) ? (uint32_t)kol * (uint32_t)OHW * 4u : SOFF_OOB);
    }
};

// A operand of the k4 s2 p1 FORWARD convolution: the raw input rows the tile touches (ConvFwdALoaderRow4's image:
// per segment of OW output pixels its four input rows of 2*OW columns, 8*BM floats per input channel = one chunk),
// taps applied on the fragment read:  lane (segment, ox), k = (ky, kx) reads  image[seg][ky][2*ox + kx - 1].
// OW is a template parameter so that the row step 2*OW sits in the ds_read's immediate offset (no VALU in the loop);
// the column left of the image (ox = 0, kx = 0) and right of it (ox = OW-1, kx = 3) are read from a zeroed region
// behind the image instead of being masked in registers.  Needs W = 2*OW, H = 2*OH, BM % OW == 0, 16-byte alignment.
// PS: the pad-skip form above (OH = OW = 4, chosen by the launcher).
template <int BM, int OWC, bool PS = false>
struct ConvFwdA2 : LoaderDefaults {
    static_assert(BM == 256 && BM % OWC == 0 && OWC >= 2, "piece mapping");
    static_assert(!PS || OWC == 4, "pad-skip: a wavefront's 128 pixels are 8 whole 4x4 maps");
    static constexpr bool PADSKIP = PS;
    // k-step S has ky = S >> 1, input row 2 * oy - 1 + ky: above the image for (oy = 0, ky = 0), below it for (3, 3)
    static constexpr unsigned skip_mask(int mode, int S) { return PS ? (S < 2 ? 1u : 0u) | (S >= 6 ? 8u : 0u) : 0u; }
    __device__ __forceinline__ int block_mirror() const { return 0; }
    using Params = typename ConvFwdALoader<BM, 4, 4, 2, 1>::Params;
    static constexpr int LD = BM, ROWS = BK / 2, PIECES = 2;
    static constexpr int OW_C = OWC;
    static constexpr int EXTRA = (6 * OWC + 4 + 3) & ~3;     // zeroed floats behind the image: every immediate row offset
                                                             // (up to 3 * 2*OW) of a redirected read stays inside
    static constexpr bool FWDROWS = true;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff[2];
    int wave, HW, C;
    __device__ __forceinline__ void init(const Params& p, int tile, int y, int tid) {
        const ConvShape& s = p.s;
        rsrc = make_rsrc(p.x, (uint32_t)(s.N * s.C * s.H * s.W) * 4u);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        HW = s.H * s.W; C = s.C;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int f = ((wave * 2 + q) * 64 + lane) * 4;
            const int seg = f / (8 * OWC), rem = f - seg * 8 * OWC;
            const int ky = rem / (2 * OWC), col = rem - ky * 2 * OWC;
            const uint32_t m = (uint32_t)tile * BM + (PS ? padskip_quad(seg) : seg) * OWC;       // first pixel of the segment
            const bool m_ok = m < (uint32_t)s.N * s.OH * s.OW;
            const uint32_t n = fdiv(m, p.div_ohw);
            const uint32_t oy = fdiv(m - n * (uint32_t)(s.OH * s.OW), p.div_ow);
            const int iy = (int)oy * 2 - 1 + ky;
            const bool ok = m_ok && (unsigned)iy < (unsigned)s.H;
            voff[q] = ok ? (n * (uint32_t)(s.C * HW) + (uint32_t)(iy * s.W + col)) * 4u : OOB;
        }
    }
    // float offsets (inside the A image) of the lane that owns tile pixel m_local, half-wave `half` (kx = 2*(s&1) +
    // half): even k-steps read `even`, odd ones `odd`, both plus (s >> 1) * 2*OW; ZERO = the zeroed region
    static constexpr int ZERO = ROWS * LD;
    __device__ __forceinline__ void frag(int m_local, int half, int& even, int& odd) const {
        const int seg = m_local / OWC, ox = m_local - seg * OWC;
        const int base = seg * 8 * OWC + 2 * ox - 1 + half;
        even = (half == 0 && ox == 0) ? ZERO : base;                  // kx = 0 left of the image
        odd = (half == 1 && ox == OWC - 1) ? ZERO : base + 2;         // kx = 3 right of it
    }
    __device__ __forceinline__ void issue_piece(int kc, float* stage, int p, bool live) {
        bload_lds16(rsrc, stage + (wave * 2 + p) * 256, voff[p], (live && kc < C) ? (uint32_t)kc * (uint32_t)HW * 4u : SOFF_OOB);
    }
};

// A operand of every tap-major gather (geometries and the reduction order: gz_igemm_loaders.h, "Tap-major gathers"):
// a chunk is 16 channels at ONE tap, its LDS image [16 channels][BM pixels] a plain gather -- pixel m of channel c is a
// fixed per-lane offset (geo.locate) plus a per-(channel, tap) scalar.  The elements of a row are S floats apart in
// memory (and a transposed phase's rows start anywhere), so the pieces are 4-BYTE LDS-DMA instructions (64 pixels of
// one channel each; 16 per wavefront and chunk at BM = 256, three per k-step).  Taps that fall into the padding are
// out-of-range lanes (zeros), re-evaluated per lane only when the tap changes (once every chans/16 chunks), and so are
// the channels past the end of a padded block.  Fragment reads are igemm_kernel's plain [k][m] ones: no VALU in the loop.
template <class Geo_>
struct TapGatherA2 : LoaderDefaults {
    using Geo = Geo_;
    static constexpr bool TAPGATHER = Geo::TAPGATHER;      // (a property of the geometry)
    using Params = typename Geo::Params;
    static constexpr int BM = Geo::BM, LD = BM, ROWS = BK;
    static constexpr int G = BM / 64;                      // 64-pixel groups per LDS row
    static constexpr int PIECES = BK * G / 4;              // per wavefront and chunk: its 4 channel rows x G groups
    Geo geo;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t vbase[G], veff[G];
    typename Geo::Pix pix[G];
    int wave, blocks, last_tap, last_kc, cb;
    uint32_t tap_soff;
    __device__ __forceinline__ void init(const Params& p, int tile, int y, int tid) {
        rsrc = geo.init(p, y);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        blocks = round_bk(geo.chans) / BK;
        last_tap = -1; last_kc = -1; cb = 0; tap_soff = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            vbase[g] = geo.locate(p, (uint32_t)tile * BM + g * 64 + lane, pix[g]);
            veff[g] = OOB;
        }
    }
    __device__ __forceinline__ void issue_piece(int kc, float* stage, int p, bool live) {
        if (p == 0) {        // (p is a literal at every call site) chunk -> (tap, channel block), wave-uniform;
                             // chunks arrive in increasing order, so only the first one costs a division
            int tap = last_tap;
            if (kc == last_kc + 1 && last_kc >= 0) {
                cb += BK;
                if (cb >= blocks * BK) { cb = 0; ++tap; }
            } else {
                tap = kc / blocks;
                cb = (kc - tap * blocks) * BK;
            }
            last_kc = kc;
            if (tap != last_tap) {
                last_tap = tap;
                const auto tp = geo.tap(tap);
                tap_soff = geo.tap_bytes(tp);
#pragma unroll
                for (int g = 0; g < G; ++g) veff[g] = geo.inside(pix[g], tp) ? vbase[g] : OOB;
            }
        }
        const int row = wave * 4 + p / G, g = p % G;
        const int c = cb + row;
        bload_lds4(rsrc, stage + row * LD + g * 64, veff[g],
                   (live && c < geo.chans) ? (uint32_t)c * (uint32_t)geo.plane * 4u + tap_soff : SOFF_OOB);
    }
};

template <int BM, int KH, int KW, int S, int P>
using ConvTapA2 = TapGatherA2<TapGeoFwd<BM, KH, KW, S, P>>;
template <int BM>
using ConvTapAnyA2 = TapGatherA2<TapGeoFwdAny<BM>>;
template <int BM, int KH, int KW, int S, int P>
using ConvDgTapA2 = TapGatherA2<TapGeoDg<BM, KH, KW, S, P>>;
template <int BM, int KS, int S, int P>
using Conv3DTapA2 = TapGatherA2<TapGeoFwd3D<BM, KS, S, P>>;
template <int BM, int KS, int S, int P>
using Conv3DDgTapA2 = TapGatherA2<TapGeoDg3D<BM, KS, S, P>>;

// ---- round 6: the 5x5 s2 p2 TRANSPOSED convolution, row-shared (HoloGAN's critic, input gradients) -------------------
// ConvDgTapA2 above gathers a chunk per (tap, 16 channels): the 9 / 6 / 6 / 4 taps of the four output phases each fetch
// the SAME gradient rows again, 4 bytes per lane and instruction, and every phase stores every other float of a row
// (EXT-128 D.block1: 6.6x its algorithmic bytes).  But along m = (n, a, b) the operand IS contiguous in memory --
//   dx[2a + py][2b + px] = sum_{ty < ny, tx < nx}  dy[a + 1 - ty][b + 1 - tx] . w[py + 2 ty][px + 2 tx],  ny = 3 - py, nx = 3 - px
// -- so the row-shared form of ConvDgA2 applies: an LDS row = 256 consecutive pixels of ONE (feature channel, ty),
// fetched ONCE by a 16-byte LDS-DMA piece, the horizontal taps applied as shifts on the fragment read (zero column for
// the lanes at an image row's edge).  What is new against k4 s2 p1:
//   * ALL FOUR output phases in one workgroup: tile = 256 pixels x 32 channels x (py, px), four wavefronts of 64 pixels
//     (TM = 2), accumulator block j = 2 py + px.  Row a + 1 - ty serves py = 0 as its tap ty and, for ty < 2, py = 1 as ITS
//     tap ty, and the column phases share the shifts (+1, 0): the A fragments are shared outright, the B image is the
//     ordinary 128-column one with columns = (phase, channel), and the epilogue stores a lane's four values as two
//     8-byte pairs (EpiPhaseQuadB: whole 64-byte lines leave the CU);
//   * TWELVE k-steps per chunk of 8 LDS rows: 8 row-shared ones (half-wave = shift +1 / 0) and then 4 PLAIN ones (half-wave
//     = next row, shift -1: px = 0's third tap) on the SAME staged rows -- every dy row is staged once;
//   * two chunk MODES, one loop each (a mode switch inside one loop made the register allocator spill accumulators):
//     rows ty < 2 feed all four phases (8 x 8 + 4 x 4 = 80 MFMAs per wavefront and chunk), rows ty = 2 the py = 0 phases
//     (40).  3 K/8 chunks, 25 K MFMAs per wavefront = exactly the 25 taps, and every workgroup is identical (two earlier
//     forms of the round were not: DESIGN 3.1);
//   * the weights are read from the EXISTING tap-major pack (pack_dgrad_tap: [phase (py, px)][tap = ty * nx + tx][ko][C])
//     by a B loader that picks the rows (DgQuadB2): no second packed image, no pack-cache changes.
// Needs AH = OH, AW = OW a multiple of 4 dividing 256, K % 16 == 0, C % 32 == 0, 16-byte aligned tensors, no bias /
// activation (an input gradient).  Reference: core/models/hologan_discriminator.py:7-23 (Conv2d k5 s2 p2).
template <int BM>
struct ConvDg5A2 : LoaderDefaults {
    static_assert(BM == 256, "one 256-pixel piece per LDS row");
    using Params = typename ConvDgALoaderTap<BM, 5, 5, 2, 2>::Params;
    static constexpr int LD = BM + 4, ROWS = 8, PIECES = 2;
    static constexpr int ZERO_COL = BM;
    static constexpr bool ROWSHARE = true, DUALMODE = true;
    static constexpr int MODES = 2, KSTEPS = 12;
    static constexpr bool step_plain(int m, int S) { return S >= 8; }
    static constexpr unsigned step_mask(int m, int S) {       // accumulator blocks (output phases) the k-step's taps feed
        return m == 0 ? (S < 8 ? 15u : 5u) : (S < 8 ? 3u : 1u);
    }
    static constexpr int step_arow(int m, int S) { return S < 8 ? S : 2 * (S - 8); }
    static constexpr int step_brow(int m, int S) { return S < 8 ? 2 * S : 16 + 2 * (S - 8); }
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff0, voff1, voff2;      // [ty]: this lane's pixel quad in row a + 1 - ty (out of range: outside the image)
    int wave, K, OHW;                  // (three scalars, not an array: a ty-indexed array ends up in scratch)
    int bound[1];                      // first chunk of mode 1 (rows ty = 2)
    __device__ __forceinline__ int mode_of(int kc) const { return kc >= bound[0]; }
    __device__ __forceinline__ void init(const Params& p, int tile, int y, int tid) {
        const ConvShape& s = p.s;
        rsrc = make_rsrc(p.y, (uint32_t)s.N * s.K * s.OH * s.OW * 4u);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        K = s.K; OHW = s.OH * s.OW;
        bound[0] = 2 * K / 8;
        const uint32_t m = (uint32_t)tile * BM + lane * 4;
        const bool m_ok = m < (uint32_t)s.N * p.AH * p.AW;
        const uint32_t n = fdiv(m, p.div_ahw);
        const uint32_t pix = m - n * (uint32_t)(p.AH * p.AW);
        const uint32_t a = fdiv(pix, p.div_aw);
        const uint32_t b = pix - a * (uint32_t)p.AW;
        auto row = [&](int ty) {
            const int oy = (int)a + 1 - ty;
            const bool ok = m_ok && (unsigned)oy < (unsigned)s.OH;
            return ok ? (n * (uint32_t)(s.K * OHW) + (uint32_t)(oy * s.OW) + b) * 4u : OOB;
        };
        voff0 = row(0); voff1 = row(1); voff2 = row(2);
    }
    __device__ __forceinline__ int frag_shift(int half) const { return half ? 0 : 1; }      // row-shared k-steps: tx = half-wave
    __device__ __forceinline__ void issue_piece(int kc, float* stage, int p, bool live) {
        const int row = wave * 2 + p;
        const int r = kc * 8 + row;          // (ty, ko), ty-major: r = ty * K + ko
        const int ty = (r >= K) + (r >= 2 * K);
        const int ko = r - ty * K;
        // (masks, not a select chain: the compiler turns `ty == 0 ? voff0 : ...` into a ty-indexed table in scratch)
        const uint32_t m0 = 0u - (uint32_t)(ty == 0), m1 = 0u - (uint32_t)(ty == 1), m2 = 0u - (uint32_t)(ty == 2);
        const uint32_t v = (voff0 & m0) | (voff1 & m1) | (voff2 & m2);
        bload_lds16(rsrc, stage + row * LD, v, live ? (uint32_t)ko * (uint32_t)OHW * 4u : SOFF_OOB);
    }
};

// B operand of ConvDg5A2: image [24 k rows][128 columns = (phase j = 2 py + px, 32 channels)] per chunk of 8 LDS rows
// r = (ty, ko), gathered row-wise out of the tap-major dgrad pack of a 5x5 s2 p2 weight (gz_pack.hip pack_dgrad_tap_body:
// phase (py, px) at phase * 9 * K * ldc floats, row (ty * nx + tx) * K + ko, nx = 3 - px): rows 0-15 = (r, tx in {0, 1}) of
// every phase that has tap row ty (py = 1 has none at ty = 2: zeros, never multiplied), rows 16-23 = (r, tx = 2) of the
// px = 0 phases.  A piece = two image rows x 128 columns (lane = (image row, 4 columns)); the lane's phase and tap offsets
// are per-lane constants, ty enters through a per-lane stride (nx differs between the column phases).
struct DgQuadB2 : LoaderDefaults {
    struct Params {
        const float* wp;
        int K, C, ldc;                  // feature channels (multiple of 16), image-side channels, row pitch of the pack
    };
    static constexpr int LD = 128, ROWS = 24, PIECES = 3;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t vA, vA_step, vA2, vB, vB2, ldb;
    int wave, K, b0;
    __device__ __forceinline__ void init(const Params& p, int tile, int y, int tid) {
        const uint32_t phase_floats = 9u * (uint32_t)p.K * (uint32_t)p.ldc;
        rsrc = make_rsrc(p.wp, 4u * phase_floats * 4u);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        K = p.K;
        b0 = 2 * K / 8;
        const int t = lane >> 5, q = (lane & 31) * 4;             // image row inside the piece, first of 4 image columns
        const int j = q >> 5, py = j >> 1, px = j & 1;
        const int ch = tile * 32 + (q & 31);
        const bool ok = ch < p.C;
        ldb = (uint32_t)p.ldc * 4u;
        const uint32_t phase = (uint32_t)j * phase_floats;
        const uint32_t kld = (uint32_t)(p.K * p.ldc);
        vA = ok ? (phase + (uint32_t)t * kld + (uint32_t)ch) * 4u : OOB;                 // + ty * vA_step, + ko * ldb
        vA_step = ok ? (uint32_t)(3 - px) * kld * 4u : 0u;
        vA2 = (ok && py == 0) ? vA + 2u * vA_step : OOB;                                    // ty = 2
        vB = (ok && px == 0) ? (phase + (uint32_t)t * (uint32_t)p.ldc + (uint32_t)ch) * 4u : OOB;   // + ((3 ty + 2) K + ko) * ldb
        vB2 = j == 0 ? vB : OOB;                                                             // ty = 2: phase (0, 0) alone
    }
    __device__ __forceinline__ void issue_piece(int kc, float* stage, int p, bool live) {
        const int piece = wave * PIECES + p;                      // 0..11: image rows 2 piece, 2 piece + 1
        const int r0 = kc * 8;                                    // the chunk's first LDS row (all of one ty: K % 8 == 0)
        const int ty = (r0 >= K) + (r0 >= 2 * K);
        uint32_t v, so;
        if (piece < 8) {                     // (LDS row r0 + piece, tx = lane's image row)
            v = kc < b0 ? vA + (uint32_t)ty * vA_step : vA2;
            so = (uint32_t)(r0 + piece - ty * K) * ldb;
        } else {                             // (LDS rows r0 + 2 (piece - 8) + lane's image row, tx = 2)
            v = kc < b0 ? vB : vB2;
            so = (uint32_t)((ty * 3 + 2) * K + (r0 + 2 * (piece - 8) - ty * K)) * ldb;
        }
        bload_lds16(rsrc, stage + piece * 256, v, live ? so : SOFF_OOB);
    }
};

// 1x1 stride-1 layers are plain GEMMs over an NCHW tensor: A[k = channel][m = (n, pixel)], 256 consecutive rows of a
// channel are 1 KB of contiguous memory whenever H*W is a multiple of 4 (a lane's 16-byte quad never straddles two
// samples).  One 16-byte LDS-DMA piece per LDS row instead of the gather's four 4-byte ones (HoloGAN's 1024 -> 1024
// projection, core/models/hologan_generator.py:130: 114 -> see DESIGN.md).
template <int BM>
struct PlaneA2 : LoaderDefaults {
    static_assert(BM % 256 == 0, "whole 256-pixel pieces per LDS row");
    struct Params {
        const float* base;
        int CH, HW, M;
        FastDiv div_hw;
    };
    static constexpr int LD = BM, ROWS = BK;
    static constexpr int PPR = BM / 256;
    static constexpr int PIECES = BK * PPR / 4;
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t voff[PPR], plane;
    int wave, CH;
    __device__ __forceinline__ void init(const Params& p, int tile, int y, int tid) {
        rsrc = make_rsrc(p.base, (uint32_t)(p.M / p.HW) * (uint32_t)p.CH * (uint32_t)p.HW * 4u);
        const int lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        CH = p.CH;
        plane = (uint32_t)p.HW * 4u;
#pragma unroll
        for (int g = 0; g < PPR; ++g) {
            const uint32_t m = (uint32_t)tile * BM + g * 256 + 4 * lane;
            const uint32_t n = fdiv(m, p.div_hw);
            voff[g] = m < (uint32_t)p.M ? (n * (uint32_t)(p.CH * p.HW) + (m - n * (uint32_t)p.HW)) * 4u : OOB;
        }
    }
    __device__ __forceinline__ void issue_piece(int kc, float* stage, int p, bool live) {
        const int row = wave * 4 + p / PPR, g = p % PPR;
        const int c = kc * BK + row;
        bload_lds16(rsrc, stage + row * LD + g * 256, voff[g], (live && c < CH) ? (uint32_t)c * plane : SOFF_OOB);
    }
};

}  // namespace gz
