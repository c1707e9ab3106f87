// The launch decision of the 2-D convolution family {F, Dg, Wg} and of the plain GEMM: the tile and split-K helpers, the
// per-op planners and predicates, and choose_fwd / choose_dgrad / choose_wgrad, which return the Choice (gz_conv_choice.h)
// a launch takes.  Host arithmetic only: nothing here launches or instantiates a kernel, so a unit that includes this
// header and calls choose_* emits no device function.  The units that read it:
//   gz_conv_fwd.hip (+ gz_conv_fwd_igemm.hip) / gz_conv_dgrad.hip / gz_conv_wgrad.hip
//                 launch_* executes the op's Choice (their run_* launchers instantiate the kernels)
//   gz_conv.hip   workspace sizes, statistics rows, gz_conv2d_tile and gz_conv2d_plan read it; the plain GEMM
// gz_igemm.h is included for the constants and traits the planners read (BK, igemm2_use_kg2, WgRowGeom).
#pragma once
#include "gz_conv_choice.h"
#include "gz_conv_direct.h"
#include "gz_igemm.h"

namespace gz {

// (TileId, Kind, Loader, Facts and Choice -- what choose_fwd / choose_dgrad / choose_wgrad, below after the planners
// they read, return -- are in gz_conv_choice.h, shared with gz_conv3d.hip; the tile configurations in gz_igemm.h, which
// also lists the headers of the two skeletons by role)

// Which launches take the igemm2 skeleton: its workgroup is a whole CU's worth of matrix pipes (one wavefront per
// SIMD), so 256 tiles already fill the chip and anything from there up runs at the loop's rate; fewer would leave
// CUs idle (those launches keep igemm_kernel + split-K).  256x128 tiles keep two workgroups per CU, whose prologues /
// epilogues overlap each other's main loops: preferred unless that halves a long reduction's operand reuse for nothing.
inline TileId pick_tile2(long long M, long long N, int ny, int kdim) {
    const bool off = knobs().no_igemm2;
    if (!off && N > 32 && N <= 64 && kdim >= 256) {             // one 64-wide column of 512-pixel tiles
        const long long t = ((M + 511) / 512) * ny;
        if (t >= 2 * cus()) return T512x64;
        // (round 4: fewer than that -- D.block1's input gradient in a bs-128 generator step, 256 tiles of 512x64 -- go to
        // 256x64 tiles when those give every CU a workgroup)
        if (!knobs().no_tile64 && knobs().igemm2_tile == 0 && N == 64 && ((M + 255) / 256) * ny >= cus()) return T256x64;
        return T64x64;
    }
    if (off || N < 128 || kdim < 256) return T64x64;            // "not applicable"
    const long long t128 = ((M + 255) / 256) * ((N + 127) / 128) * ny;
    const long long t256 = ((M + 255) / 256) * ((N + 255) / 256) * ny;
    const int force = knobs().igemm2_tile;
    const int cu = cus();
    // round 4: 256x64 tiles (three workgroups per CU) where 256x128 would put fewer than two workgroups on a CU and
    // 256x64 gives every CU at least one: bs 128, D.block1 forward 95 -> 115 TFLOP/s, D.block2's input gradient 92 ->
    // 111; bs 256 (the stacked discriminator pass of bs 128): D.block2 forward 114 -> 124, D.block3's input gradient
    // 107 -> 119; every launch with >= 512 tiles of 256x128 keeps them (tools/conv_bench2.py, GZ_NO_TILE64=1)
    if (force == 256 && N >= 256 && t256 >= cu) return T256x256;
    if (force == 128 && t128 >= cu) return T256x128;
    if (t128 >= 2 * cu) return T256x128;
    if (N >= 256 && t256 >= cu) return T256x256;        // (round 3's choice where it applies: kept)
    if (t128 >= cu) return T256x128;
    // round 4: 256x64 tiles (three workgroups per CU) where 256x128 tiles would not give every CU a workgroup and the
    // launch would split its reduction instead: bs 128, D.block1 forward 95 -> 115 TFLOP/s, D.block2's input gradient
    // 92 -> 111; bs 256 (the stacked discriminator pass of bs 128): D.block2 forward 114 -> 124, D.block3's input
    // gradient 107 -> 119.  Launches with 256-511 tiles of 256x128 keep them (bs 512: 256x64 measured 2-5 % slower
    // there).  tools/conv_bench2.py, GZ_NO_TILE64=1.
    if (!knobs().no_tile64 && force == 0 && (N & 63) == 0) {
        const long long t64 = ((M + 255) / 256) * ((N + 63) / 64) * ny;
        if (t64 >= cu) return T256x64;
    }
    return T64x64;
}

inline int forced_tile() { return knobs().tile; }

// Tile choice.  Measured on the DCGAN layers at bs 512 (tools/conv_bench.py, round 2, 4 / 6 / 8 co-resident
// workgroups per CU for the three shapes): a launch that fills the chip runs at ~125 (128x128), ~112 (128x64) and
// ~108 TFLOP/s (64x64); one that leaves workgroup slots empty loses in proportion (D.block3's dgrad: 512 tiles of
// 128x128 on 1024 slots -> the 2048 64x64 tiles win), and between one and two rounds part of the second round is
// exposed.  Score = shape efficiency x fill and take the best; narrow N gets narrow tiles.
inline TileId pick_tile(long long M, long long N, int ny, int kdim = 0) {
    int f = forced_tile();
    if (f >= 0 && f <= 3) {
        if (!(f == T128x128 && N <= 64) ) return (TileId)f;
    }
    if (N <= 32) return T128x32;
    auto tiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn) * ny; };
    // A launch with >= 34 GFLOP of work (65536 tile-chunks of 128x128x16) always has enough of it for ~1024 workgroups of
    // the 128x128 shape with >= 64 chunks each once the reduction is split (plan_split), and that beats the smaller
    // shapes whatever the tile count says: bs 128, G.block2's input gradient 0.370 -> 0.305 ms, G.block3's 0.309 ->
    // 0.295, their forward 0.337 -> 0.324 / 0.299 -> 0.293; the 8.6 GFLOP discriminator layers of that batch lose 10 %
    // the same way (16 chunks per workgroup: prologue, slab write and finish dominate) and stay with the score.
    const bool no_big = knobs().no_big_split;
    if (!no_big && kdim > 0 && N > 64 && tiles(128, 128) * ((kdim + BK - 1) / BK) >= 65536) return T128x128;
    if (knobs().min_wgs > 0) {            // round-1 rule, kept for experiments
        const long long want = knobs().min_wgs;
        if (N <= 64) return tiles(128, 64) >= want ? T128x64 : T64x64;
        if (tiles(128, 128) >= want) return T128x128;
        if (tiles(128, 64) >= want) return T128x64;
        return T64x64;
    }
    auto score = [&](int bm, int bn, double eff, int per_cu) {
        const double rounds = (double)tiles(bm, bn) / ((double)cus() * per_cu);
        double fill = 1.0;
        if (rounds <= 1.0) fill = rounds;
        else if (rounds < 2.0) fill = 0.5 + 0.5 * rounds / 2.0;      // 1 < rounds < 2: half of the tail is hidden
        return eff * fill;
    };
    const double s64 = score(64, 64, 0.86, 8), s128x64 = score(128, 64, 0.90, 6);
    if (N <= 64) return s128x64 >= s64 ? T128x64 : T64x64;
    const double s128 = score(128, 128, 1.0, 4);
    if (s128 >= s128x64 && s128 >= s64) return T128x128;
    return s128x64 >= s64 ? T128x64 : T64x64;
}

// Split-K for F / Dg / GEMM launches whose output has too few tiles to fill 256 CUs (deep 4x4 / 8x8 feature
// maps at small batch, the nn.Linear heads: M = batch rows, K = 8192).  Such a launch runs one workgroup per
// CU or less and is bound by the per-chunk load -> LDS -> barrier latency, which only other resident workgroups
// can hide.  Keep the tile pick_tile chose and cut the reduction so that ~1024 workgroups are in flight, each
// with >= 8 chunks (128 reduction steps); the raw partial tiles go to workspace slabs, splitk_finish_kernel
// sums them in a fixed order and applies the epilogue.
struct SplitPlan {
    TileId tile;
    int splits;
};

inline long long tile_count(TileId t, long long M, long long N, int ny) {
    if (t == T256x256 || t == T256x128) return ((M + 255) / 256) * ((N + (t == T256x256 ? 255 : 127)) / (t == T256x256 ? 256 : 128)) * ny;
    if (t == T512x64) return ((M + 511) / 512) * ((N + 63) / 64) * ny;
    if (t == T256x64) return ((M + 255) / 256) * ((N + 63) / 64) * ny;
    const int bm = t == T64x64 ? 64 : 128;
    const int bn = t == T128x128 ? 128 : (t == T128x32 ? 32 : 64);
    return ((M + bm - 1) / bm) * ((N + bn - 1) / bn) * ny;
}

inline SplitPlan plan_split(long long M, long long N, int Kdim, int ny, TileId normal) {
    SplitPlan none{normal, 1};
    const int target = knobs().split_target * cus() / 256, below = knobs().split_below * cus() / 256;
    if (knobs().no_splitk) return none;
    const int chunks = (Kdim + BK - 1) / BK;
    const long long tiles = tile_count(normal, M, N, ny);
    if (chunks < 16 || tiles >= below) return none;
    long long want = (target + tiles - 1) / tiles, cap = chunks / 8;
    int splits = (int)(want < cap ? want : cap);
    if (splits < 2) return none;
    return SplitPlan{normal, splits};
}

inline size_t split_bytes(const SplitPlan& sp, long long M, long long N, int Kdim, int ny) {
    if (sp.splits <= 1) return 0;
    return (size_t)split_nz(Kdim, sp.splits) * ny * M * N * 4;
}

template <int KH, int KW, int S, int P>
struct Geo {
    static constexpr int kh = KH, kw = KW, s = S, p = P;
};

// the four geometries with kernels of their own (GZ_GEOM_DISPATCH, at the end of this header)
typedef Geo<4, 4, 2, 1> G4421;
typedef Geo<5, 5, 2, 2> G5522;
typedef Geo<3, 3, 1, 1> G3311;
typedef Geo<1, 1, 1, 0> G1110;

// ---------------------------------------------------------------------------
// F
// ---------------------------------------------------------------------------
template <class G>
inline bool fwd2_ok(const ConvShape& s) {
    return G::kh == 4 && G::kw == 4 && G::s == 2 && G::p == 1 && s.H == 2 * s.OH && s.W == 2 * s.OW &&
           (s.OW == 4 || s.OW == 8 || s.OW == 16 || s.OW == 32 || s.OW == 64);
}

template <class G>
inline int fwd_kdim(const ConvShape& s) {
    return G::kh * G::kw * (fwd_tap_major(s.C, G::kh, G::kw) ? round_bk(s.C) : s.C);
}

// Forward tile.  One correction to the score: k4 s2 p1 with output rows shorter than 16 pixels runs on the K4V gather
// loader, whose 64x64 form is its weak spot (bs 128, G.block2's input gradient: 93 vs 107 TFLOP/s; bs 512, D.block2
// forward: 110 vs 113) -- with >= 512 tiles of 128x128 the chip is half full and that kernel still wins.
inline TileId pick_tile_fwd(long long M, int K, int OW, int kh, int kw, int stride, int kdim) {
    TileId t = pick_tile(M, K, 1, kdim);
    if (forced_tile() < 0 && kh == 4 && kw == 4 && stride == 2 && OW < 16 && t == T64x64 && K > 64 &&
        tile_count(T128x128, M, K, 1) >= 2 * cus())
        t = T128x128;
    return t;
}

// igemm2 plan of a forward launch: tile and reduction splits (few M tiles: the reduction is cut so that >= 256
// workgroups exist, each with >= 32 chunks)
// tap-major geometries on the igemm2 skeleton (ConvTapA2): >= 128 output channels, and enough tiles x reduction
// splits to give every CU a workgroup, each with >= 32 chunks
template <class G>
inline SplitPlan fwdtap2_plan(const ConvShape& s) {
    const bool off = knobs().no_igemm2 || knobs().no_igemm2_tap;
    if constexpr (BK % (G::kh * G::kw) == 0 && G::kh * G::kw != 1) return SplitPlan{T64x64, 1};
    if (off || !(G::kh * G::kw == 1 ? s.C >= BK : fwd_tap_major(s.C, G::kh, G::kw)) || s.K < 128 || (s.K & 3))
        return SplitPlan{T64x64, 1};
    const long long M = (long long)s.N * s.OH * s.OW;
    const long long tiles = ((M + 255) / 256) * ((s.K + 127) / 128);
    const int chunks = G::kh * G::kw * round_bk(s.C) / BK;
    const int cu = cus();
    if (tiles >= cu * 7 / 8) return SplitPlan{T256x128, 1};
    // split launches pay off from ~64 chunks per workgroup (HoloGAN EXT-128's blocks: 100 -> 115-118 TFLOP/s against
    // 80-94 on the 64x64 tiles; the 64x64-image blocks would get 33 chunks each and lose 5 %)
    if (tiles >= 8 && chunks >= 128) {
        int splits = (int)((cu + tiles - 1) / tiles);
        while (splits > 1 && chunks / splits < 64) --splits;
        if (splits > 1 && tiles * splits >= cu * 3 / 4) return SplitPlan{T256x128, splits};
    }
    // round 4: 256x64 tiles for the launches too small for the rule above (HoloGAN's 5x5 s2 p2 critic blocks at 64x64,
    // 6.7 GFLOP each, bs 64: 76 / 77 / 65 -> 92 / 92 / 76 TFLOP/s; 16, 32 or 48 chunks per piece measure the same)
    const int mc = knobs().tap64_min_chunks;
    if (mc > 0 && !knobs().no_tile64 && (s.K & 63) == 0 && chunks >= mc) {
        const long long t64 = ((M + 255) / 256) * ((s.K + 63) / 64);
        if (t64 >= cu * 7 / 8) return SplitPlan{T256x64, 1};
        int splits = (int)((cu + t64 - 1) / t64);
        while (splits > 1 && chunks / splits < mc) --splits;
        if (t64 >= 8 && t64 * splits >= cu * 3 / 4) return SplitPlan{T256x64, splits};
    }
    return SplitPlan{T64x64, 1};
}

template <class G>
inline SplitPlan fwd2_plan(const ConvShape& s) {
    if (!fwd2_ok<G>(s)) return fwdtap2_plan<G>(s);
    const long long M = (long long)s.N * s.OH * s.OW;
    TileId t = s.K > 64 ? pick_tile2(M, s.K, 1, s.C * 16) : T64x64;
    if (t == T256x256 || t == T256x128 || t == T256x64) return SplitPlan{t, 1};
    const bool off = knobs().no_igemm2;
    if (off || s.K < 128) return SplitPlan{T64x64, 1};
    // split launches take the 256x64 tile when the channel count allows: twice the tiles, half the slabs
    const bool t64 = !knobs().no_tile64 && (s.K & 63) == 0;
    const long long tiles = ((M + 255) / 256) * (t64 ? (s.K + 63) / 64 : (s.K + 127) / 128);
    const int chunks = s.C;
    const int min_tiles = knobs().fwd2_min_tiles * (t64 ? 2 : 1);
    if (tiles >= min_tiles && chunks >= 64) {
        int splits = (int)((cus() + tiles - 1) / tiles);
        while (splits > 1 && chunks / splits < 32) --splits;
        if (splits > 1 && tiles * splits >= cus()) return SplitPlan{t64 ? T256x64 : T256x128, splits};
    }
    return SplitPlan{T64x64, 1};
}

template <class G>
inline SplitPlan fwd_plan(const ConvShape& s) {
    long long M = (long long)s.N * s.OH * s.OW;
    {
        const SplitPlan p2 = fwd2_plan<G>(s);
        if (p2.tile == T256x256 || p2.tile == T256x128 || p2.tile == T256x64) return p2;
    }
    return plan_split(M, s.K, fwd_kdim<G>(s), 1, pick_tile_fwd(M, s.K, s.OW, G::kh, G::kw, G::s, fwd_kdim<G>(s)));
}

template <class G>
inline size_t fwd_ws_bytes(const ConvShape& s) {
    return split_bytes(fwd_plan<G>(s), (long long)s.N * s.OH * s.OW, s.K, fwd_kdim<G>(s), 1);
}

// ---------------------------------------------------------------------------
// F with run-time geometry (evaluation path: InceptionV3).  Always tap-major, channels padded to a chunk.
// ---------------------------------------------------------------------------
struct AnyGeom {
    int KH, KW, SH, SW, PH, PW;
};

inline bool any_shape_ok(const ConvShape& s, const AnyGeom& g) {
    if (s.N <= 0 || s.C <= 0 || s.K <= 0 || s.H <= 0 || s.W <= 0 || g.KH <= 0 || g.KW <= 0 || g.SH <= 0 || g.SW <= 0 ||
        g.PH < 0 || g.PW < 0)
        return false;
    return s.OH == (s.H + 2 * g.PH - g.KH) / g.SH + 1 && s.OW == (s.W + 2 * g.PW - g.KW) / g.SW + 1 && s.OH > 0 &&
           s.OW > 0;
}

// the run-time geometries on the igemm2 skeleton (run_fwd_any2, gz_conv_fwd.hip):
// 0: not applicable; 64: the tile's column count (256x64 tiles, three workgroups per CU: the 256x128 instantiation with
// the bias + ReLU epilogue needed 256 registers + 180 bytes of scratch and was not kept)
inline int fwd_any2_cols(const ConvShape& s, const AnyGeom& g, const float* bias, int act) {
    if (knobs().no_igemm2 || knobs().no_any2 || !bias || !(act == ACT_NONE || act == ACT_RELU)) return 0;
    // (output channels: any multiple of 16 from 48 up -- a ragged last column tile stores through EpiNCHW's element-wise
    // path: 80, 96 and 48 of InceptionV3 fill 63-75 % of their last tile and still beat the 64x64 igemm_kernel tiles)
    if (s.C < BK || (s.K & 15) || s.K < 48 || g.KH * g.KW * (round_bk(s.C) / BK) < 8) return 0;
    const long long M = (long long)s.N * s.OH * s.OW;
    const long long t64 = ((M + 255) / 256) * ((s.K + 63) / 64);
    return t64 >= cus() * 7 / 8 ? 64 : 0;
}

inline SplitPlan fwd_any_plan(const ConvShape& s, const AnyGeom& g) {
    long long M = (long long)s.N * s.OH * s.OW;
    return plan_split(M, s.K, g.KH * g.KW * round_bk(s.C), 1, pick_tile(M, s.K, 1));
}

// ---------------------------------------------------------------------------
// Dg
// ---------------------------------------------------------------------------
template <class G>
inline SplitPlan dgradtap2_plan(const ConvShape& s) {
    const bool off = knobs().no_igemm2 || knobs().no_igemm2_tap;
    constexpr int TY = (G::kh + G::s - 1) / G::s, TX = (G::kw + G::s - 1) / G::s;
    constexpr bool one_by_one = G::kh * G::kw == 1;
    if constexpr (G::s * G::s > 8 || (!one_by_one && G::kh % G::s == 0 && G::kw % G::s == 0 && BK % (TY * TX) == 0))
        return SplitPlan{T64x64, 1};        // (k4 s2 p1 has its own loaders)
    // round 4: 256x64 tiles for the launches too small for 256x128; they also admit 64 image-side channels (tools/
    // tap_bench.py 64, TFLOP/s: HoloGAN 64x64 D.block2 / D.block3 input gradients 60 / 52 -> 77 / 67; EXT-128's
    // D.block1, 64 channels, 102 -> 123; with 48 instead of 32 chunks per piece 57 / 53 -- worse than the old kernel)
    const int mc64 = (!knobs().no_tile64 && G::s != 1 && (s.C & 63) == 0) ? knobs().tap64_min_chunks : 0;
    if (off || !(one_by_one ? s.K >= BK : dgrad_tap_major(s.K, G::kh, G::kw, G::s)) || s.C < (mc64 > 0 ? 64 : 128) ||
        (s.C & 3) || s.H % G::s || s.W % G::s)
        return SplitPlan{T64x64, 1};
    const long long M = (long long)s.N * (s.H / G::s) * (s.W / G::s);
    const long long tiles = ((M + 255) / 256) * ((s.C + 127) / 128);
    const int kblocks = round_bk(s.K) / BK;
    long long total = 0;
    for (int ph = 0; ph < G::s * G::s; ++ph)
        total += (long long)dg_taps(G::kh, G::s, G::p, ph / G::s) * dg_taps(G::kw, G::s, G::p, ph % G::s) * kblocks;
    const int maxchunks = TY * TX * kblocks;
    // one phase (stride 1): nothing to balance -- split only when the tiles alone do not fill the chip
    if (G::s == 1) {
        if (tiles >= cus() * 7 / 8 && maxchunks >= 8) return SplitPlan{T256x128, 1};
        if (tiles * total < 2LL * cus() * 32) return SplitPlan{T64x64, 1};
        int splits = (int)((cus() + tiles - 1) / tiles);
        while (splits > 1 && maxchunks / splits < 64) --splits;
        return (splits > 1 && tiles * splits >= cus() * 3 / 4) ? SplitPlan{T256x128, splits} : SplitPlan{T64x64, 1};
    }
    if (tiles * total < 2LL * cus() * 32 || s.C < 128) {       // too little work for the big tile
        if (mc64 > 0) {
            const long long t64 = ((M + 255) / 256) * (s.C / 64);
            // (64 channels = one column of tiles: only with enough of them -- the 64x64-image D.block1 has 64 tiles and
            // loses, 84 -> 76, on this skeleton)
            if (t64 * total >= 1LL * cus() * mc64 && (s.C >= 128 || t64 >= cus() * 3 / 4)) {
                const int wgs64 = knobs().tap_wgs * cus() / 256;
                long long cps = (t64 * total + wgs64 - 1) / wgs64;
                if (cps < mc64) cps = mc64;
                if (cps > knobs().tap_cps_max) cps = knobs().tap_cps_max;
                const int splits = (int)((maxchunks + cps - 1) / cps);
                return SplitPlan{T256x64, splits < 1 ? 1 : splits};
            }
        }
        return SplitPlan{T64x64, 1};
    }
    // ~384 workgroups of <= 96 chunks (measured on HoloGAN EXT-128's blocks, TFLOP/s of D.block2 / D.block3:
    // 256 workgroups 84 / 67, 384: 99 / 99, 512: 99 / 89, 768: 90 / 86; the round-2 kernels: 89 / 74)
    const int wgs = knobs().tap_wgs * cus() / 256, cps_max = knobs().tap_cps_max;
    long long cps = (tiles * total + wgs - 1) / wgs;
    if (cps < 32) cps = 32;
    if (cps > cps_max) cps = cps_max;
    const int splits = (int)((maxchunks + cps - 1) / cps);
    return SplitPlan{T256x128, splits < 1 ? 1 : splits};
}

// ---- 5x5 s2 p2 transposed convolution on row-shared LDS rows, all four output phases per workgroup (gz_igemm2_loaders.h:
// ConvDg5A2, DgQuadB2, EpiPhaseQuadB; round 6; launcher: run_dgrad5, gz_conv_dgrad.hip).  Tile = 256 pixels x 32 channels
// x (py, px); columns N = 4 C, one grid phase; 3 K/8 chunks of 12 k-steps, every workgroup identical.
// Unsplit when every CU gets a workgroup, else the
// reduction is cut for ~512 workgroups (slabs + the finish pass).  Launches with little work per CU stay on the gather
// loader: measured (tools/tap_bench.py 64 / 128, TFLOP/s, this kernel vs the gather loader): EXT-128's critic at bs 64
// D.block1 125 vs 123, D.block2 111 vs 99, D.block3 102 vs 99, at bs 128 128 / 128 / 117; the 6.7-GFLOP layers of the
// 64 x 64 critic 65-72 vs 67-84.
struct Dg5Plan {
    bool ok;
    int splits, nz;
};
template <class G>
inline bool dgrad5_shape_ok(const ConvShape& s) {
    return G::kh == 5 && G::kw == 5 && G::s == 2 && G::p == 2 && !knobs().no_igemm2 && !knobs().no_dg5 && s.H == 2 * s.OH &&
           s.W == 2 * s.OW && s.OW % 4 == 0 && 256 % s.OW == 0 && s.K % 16 == 0 && s.K >= 32 && s.C % 32 == 0 &&
           dgrad_tap_major(s.K, 5, 5, 2) && (long long)s.N * s.OH * s.OW >= 256;
}
template <class G>
inline Dg5Plan dgrad5_plan(const ConvShape& s) {
    Dg5Plan p{false, 1, 1};
    if (!dgrad5_shape_ok<G>(s)) return p;
    const long long M = (long long)s.N * s.OH * s.OW;
    const long long tiles = ((M + 255) / 256) * (s.C / 32);
    const int chunks = 3 * s.K / 8;          // chunks of 8 LDS rows, 12 k-steps each
    if (tiles * chunks < 1LL * cus() * knobs().dg5_min_units) return p;
    p.ok = true;
    if (tiles >= cus()) return p;                                  // unsplit: every CU has a workgroup
    const long long want = (long long)knobs().dg5_wgs * cus() / 256;
    long long cps = (tiles * chunks + want - 1) / want;
    if (cps < knobs().dg5_min_chunks) cps = knobs().dg5_min_chunks;
    if (cps >= chunks) return p;
    p.splits = (int)((chunks + cps - 1) / cps);
    const int per = (chunks + p.splits - 1) / p.splits;           // (= launch_igemm2's chunks_per_split)
    p.nz = (chunks + per - 1) / per;
    if (p.nz <= 1) p.splits = p.nz = 1;
    return p;
}
template <class G>
inline size_t dgrad5_ws_bytes(const ConvShape& s) {
    const Dg5Plan p = dgrad5_plan<G>(s);
    if (!p.ok || p.nz <= 1) return 0;
    return (size_t)p.nz * (size_t)s.N * s.OH * s.OW * (size_t)(4 * s.C) * 4;
}

template <class G>
inline bool dgrad2_ok(const ConvShape& s) {
    // ConvDgA2: 16-byte pieces of whole pixel quads; a tile's first pixel starts an image row (256 % AW == 0)
    // (the 512-pixel tile: 512 % AW == 0 follows)
    return G::kh == 4 && G::kw == 4 && G::s == 2 && G::p == 1 && s.H == 2 * s.OH && s.W == 2 * s.OW && s.OW % 4 == 0 &&
           256 % s.OW == 0 && s.K % 4 == 0;
}

template <class G>
inline bool dgrad_direct(const ConvShape& s) {          // (and an 8-byte aligned x: choose_dgrad)
    return G::kh == 4 && G::kw == 4 && G::s == 2 && G::p == 1 && s.C <= 4 && s.H == 2 * s.OH && s.W == 2 * s.OW &&
           !knobs().no_smallc;
}

template <class G>
inline SplitPlan dgrad_plan(const ConvShape& s) {
    constexpr int TAPS = ((G::kh + G::s - 1) / G::s) * ((G::kw + G::s - 1) / G::s);
    long long M = (long long)s.N * (s.H / G::s) * (s.W / G::s);
    const int kk = dgrad_tap_major(s.K, G::kh, G::kw, G::s) ? round_bk(s.K) : s.K;
    if (dgrad2_ok<G>(s)) {
        const TileId t2 = pick_tile2(M, s.C, 4, s.K * 4);
        if (is_tile2(t2)) return SplitPlan{t2, 1};
        // 64-255 tiles of 256x128 (small batches, deep layers): cut the reduction so that >= 256 workgroups exist,
        // each with >= 32 chunks (as the forward convolution does)
        const bool off = knobs().no_igemm2;
        const bool t64 = !knobs().no_tile64 && (s.C & 63) == 0;
        const long long tiles = ((M + 255) / 256) * (t64 ? (s.C + 63) / 64 : (s.C + 127) / 128) * 4;
        const int chunks = s.K / 4;
        const int min_tiles = knobs().dg2_min_tiles * (t64 ? 2 : 1);
        if (!off && s.C >= 128 && tiles >= min_tiles && tiles < cus() && chunks >= 64) {
            int splits = (int)((cus() + tiles - 1) / tiles);
            while (splits > 1 && chunks / splits < 32) --splits;
            if (splits > 1 && tiles * splits >= cus()) return SplitPlan{t64 ? T256x64 : T256x128, splits};
        }
    }
    {
        const SplitPlan pt = dgradtap2_plan<G>(s);
        if (pt.tile == T256x128 || pt.tile == T256x64) return pt;
    }
    return plan_split(M, s.C, kk * TAPS, G::s * G::s, pick_tile(M, s.C, G::s * G::s, kk * TAPS));
}

template <class G>
inline size_t dgrad_ws_bytes(const ConvShape& s) {
    constexpr int TAPS = ((G::kh + G::s - 1) / G::s) * ((G::kw + G::s - 1) / G::s);
    if (s.H % G::s || s.W % G::s || dgrad_direct<G>(s)) return 0;
    const int kk = dgrad_tap_major(s.K, G::kh, G::kw, G::s) ? round_bk(s.K) : s.K;
    const size_t b = split_bytes(dgrad_plan<G>(s), (long long)s.N * (s.H / G::s) * (s.W / G::s), s.C, kk * TAPS, G::s * G::s);
    // (ConvDg5A2 needs aligned tensors, known only at the launch: the workspace serves either path)
    const size_t b5 = dgrad5_ws_bytes<G>(s);
    return b > b5 ? b : b5;
}

// ---------------------------------------------------------------------------
// Wg
// ---------------------------------------------------------------------------
inline int wg_target() {
    const int t = knobs().wg_target;     // 1024: 4 workgroups of the 128x128 shape per CU (round 2; was 1536 at 2 per CU)
    return t < 1 ? 1 : t;
}

// Split-K so that ~4 workgroups per CU are in flight: the wgrad loaders are gather-heavy and only
// reach the MFMA rate when several workgroups per SIMD overlap their load and MFMA phases.
inline int wgrad_splits(long long tiles, int chunks, bool big_tile = true) {
    long long target = (big_tile ? wg_target() : 512) * cus() / 256;   // narrow tiles (3-channel layers) are slab-traffic bound
    if (tiles * 4 >= target * 3) return 1;
    long long want = (target + tiles - 1) / tiles;
    if (big_tile) {
        // ... but a 128x128 workgroup that reduces fewer than 32 chunks spends its time on the prologue and its 64 KB
        // slab: keep >= 32 chunks per split as long as >= 512 workgroups remain (bs 128, D.block1 / block2: 128 x 16
        // chunks -> 64 x 32, 0.111 -> 0.105 and 0.116 -> 0.110 ms; every bs 512 layer keeps its plan)
        const long long by_len = chunks / 32 > 0 ? chunks / 32 : 1, want_min = (2 * cus() + tiles - 1) / tiles;
        const long long floor_ = by_len > want_min ? by_len : want_min;
        if (floor_ < want) want = floor_;
    }
    long long cap = chunks / 8 > 0 ? chunks / 8 : 1;  // keep >= 8 chunks (128 pixels) per split
    long long s = want < cap ? want : cap;
    return (int)(s < 1 ? 1 : s);
}

// can a 16-pixel K chunk be taken as whole row segments of one image? (see WgBLoaderRow)
template <class G>
inline bool wg_row_geom(const ConvShape& s, WgRowGeom* g) {
    int CW = s.OW < 16 ? s.OW : 16;
    if (CW <= 0 || 16 % CW) return false;
    int R = 16 / CW;
    if (s.OW % CW || s.OH % R) return false;
    auto mx = [](int a, int b) { return a > b ? a : b; };
    if (G::s * R < mx(G::p, G::kh - 1 - G::p) || G::s * CW < mx(G::p, G::kw - 1 - G::p)) return false;
    // a negative offset must never survive masking: the only negative cases are the flagged ones
    g->CW = CW;
    g->R = R;
    g->div_ohw = make_fastdiv(s.OH * s.OW);
    g->div_ow = make_fastdiv(s.OW);
    return true;
}

// Weight gradient on the igemm2 skeleton (run_wgrad2 / run_wgrad2w, gz_conv_wgrad.hip): tile 256 (output channels) x 128
// ((c, ky, kx) columns); K in [128, 256): the 128 x 256 tile (one row of wavefronts, all four along the columns)
inline bool wgrad2_narrow(const ConvShape& s) { return s.K < 256; }

template <class G>
constexpr bool wgrad2w_geom() {
    return (G::kh == 4 && G::kw == 4 && G::s == 2 && G::p == 1) || (G::kh == 5 && G::kw == 5 && G::s == 2 && G::p == 2) ||
           (G::kh == 3 && G::kw == 3 && G::s == 1 && G::p == 1);
}

template <class G>
inline int wgrad2_splits(const ConvShape& s) {
    const bool off = knobs().no_igemm2 || knobs().no_igemm2_wg;
    WgRowGeom rg;
    const int NTOT = s.C * G::kh * G::kw;
    if (off || s.K < 128 || s.K % 32 || NTOT < 256 - 128 * !wgrad2_narrow(s) || !wg_row_geom<G>(s, &rg)) return 0;
    const long long tiles = wgrad2_narrow(s) ? (long long)((s.K + 127) / 128) * ((NTOT + 255) / 256)
                                             : (long long)((s.K + 255) / 256) * ((NTOT + 127) / 128);
    const int chunks = (s.N * s.OH * s.OW + BK - 1) / BK;
    // at most ONE round of the chip's 512 workgroup slots (two per CU): 18 tiles x 29 splits = 522 workgroups took two
    // rounds (3x3 s1 p1 256@32: 96 TFLOP/s; 28 splits: one round)
    int splits = (int)(2 * cus() / tiles);
    if (splits < 1) splits = 1;
    // >= 64 chunks per workgroup for the register-staged kernel; the LDS-DMA kernel's chunks cost nothing but their
    // MFMAs, so 32 are enough there (bs 128: D.block1-3's weight gradients move from the 128x128 kernel onto it)
    const int min_chunks_env = knobs().wg2_min_chunks;
    const bool dma = wgrad2w_geom<G>() && s.H == G::s * s.OH && s.W == G::s * s.OW &&
                     (s.OW == 4 || s.OW == 8 || s.OW % 16 == 0) && !knobs().no_igemm2w;
    const int min_chunks = min_chunks_env > 0 ? min_chunks_env : (dma ? 32 : 64);
    while (splits > 1 && chunks / splits < min_chunks) --splits;
    return tiles * splits >= cus() ? splits : 0;
}

template <class G>
inline int wgrad2w_cw_shape(const ConvShape& s) {        // pixel-chunk width of the LDS-DMA weight gradient, 0 = not applicable
    const bool off = knobs().no_igemm2w;
    const bool off_g = knobs().no_igemm2wg;        // the generic-geometry image only
    if (off || !wgrad2w_geom<G>()) return 0;
    if (off_g && !(G::kh == 4 && G::kw == 4)) return 0;
    if (s.H != G::s * s.OH || s.W != G::s * s.OW || (s.W & 3)) return 0;
    const int cw = s.OW == 4 ? 4 : s.OW == 8 ? 8 : (s.OW % 16 == 0 ? 16 : 0);
    if (!cw || s.OH % (16 / cw)) return 0;
    return cw;
}

// ---------------------------------------------------------------------------
// The launch choice of each op.  Every condition that selects a kernel or a loader is written here and nowhere else; a
// new skeleton or loader is added in choose_* here and in the op's launch_* (gz_conv_fwd.hip, gz_conv_dgrad.hip,
// gz_conv_wgrad.hip), the one function that executes the choice.
// ---------------------------------------------------------------------------
template <class G>
constexpr bool is_k4s2p1() { return G::kh == 4 && G::kw == 4 && G::s == 2 && G::p == 1; }
template <class G>
constexpr bool is_k5s2p2() { return G::kh == 5 && G::kw == 5 && G::s == 2 && G::p == 2; }
template <class G>
constexpr bool is_k3s1p1() { return G::kh == 3 && G::kw == 3 && G::s == 1 && G::p == 1; }
template <class G>
constexpr bool is_k1() { return G::kh * G::kw == 1 && G::s == 1 && G::p == 0; }

// k4 s2 p1 has loaders of its own (ConvFwdA2 / ConvDgA2) and the planners never pair it with the gather loaders
// (fwdtap2_plan / dgradtap2_plan return "not applicable" for it): not instantiating them for that geometry takes eight
// never-launched kernels out of the library (round 5, tools/kernel_reach.sh; run_fwdtap2 / run_dgradtap2 ask).
template <class G>
constexpr bool has_own_igemm2_loaders() { return G::kh == 4 && G::kw == 4 && G::s == 2 && G::p == 1; }

// the igemm2 part of a choice: slabs, and whether launch_igemm2 runs two wave groups per workgroup (its own test,
// igemm2_use_kg2; the 1x1 plane loader has no two-group form, every other igemm2 convolution loader does)
inline void choose_igemm2(Choice& c, long long tiles, int kdim) {
    c.kind = KIgemm2;
    c.slabs = split_nz(kdim, c.splits);
    const int chunks = (kdim + BK - 1) / BK, cps = (chunks + c.splits - 1) / c.splits;
    if (c.loader != LPlane2 && (c.tile == T256x128 || c.tile == T256x64) && igemm2_use_kg2(tiles * c.slabs, cps))
        c.wave_groups = 2;
}

template <class G>
inline Choice choose_fwd(const ConvShape& s, const Facts& f) {
    const long long M = (long long)s.N * s.OH * s.OW;
    SplitPlan sp = fwd_plan<G>(s);
    // (a direct kernel keeps, as its gz_conv2d_tile label, the tile of the igemm launch it replaces)
    if (is_k3s1p1<G>() && !f.stats && conv3_smallch_ok(s.N, s.C, s.K, s.H, s.W))
        return choice_of(KDirect, conv3_fewk_ok(s.C, s.K, s.H, s.W) && f.in16 && f.out16 ? LFewk : LSmallch, sp.tile);
    Choice c = choice_of(KIgemm, LGeneric, sp.tile);
    if (sp.splits > 1 && ws_lacks(f, fwd_ws_bytes<G>(s))) {
        c.ws_short = true;
        sp = SplitPlan{pick_tile_fwd(M, s.K, s.OW, G::kh, G::kw, G::s, 0), 1};
    }
    if (is_tile2(sp.tile) && fwd2_ok<G>(s) && !f.in16)      // unaligned tensor: the element-wise loaders
        sp = SplitPlan{pick_tile_fwd(M, s.K, s.OW, G::kh, G::kw, G::s, 0), 1};
    c.tile = sp.tile;
    c.splits = sp.splits;
    if (is_tile2(c.tile)) {
        const bool rows = fwd2_ok<G>(s);
        c.loader = rows ? LRows2
                   : (is_k1<G>() && !knobs().no_plane_a && ((s.H * s.W) & 3) == 0 && f.in16) ? LPlane2 : LGather2;
        choose_igemm2(c, tile_count(c.tile, M, s.K, 1), rows ? s.C * 16 : G::kh * G::kw * round_bk(s.C));
        return c;
    }
    c.slabs = split_nz(fwd_kdim<G>(s), c.splits);
    const int bm = c.tile == T64x64 ? 64 : 128;
    if (BK % (G::kh * G::kw) != 0 && fwd_tap_major(s.C, G::kh, G::kw)) c.loader = LTap;
    // Row4 (GZ_NO_ROW4: the K4V loader) for OW >= 16 only: with shorter rows the stride-2 fragment reads of the lanes
    // of a half-wave fall on 2*OW / 2 banks (OW = 4: an 8-way conflict; measured 113 -> 108 TFLOP/s on D.block3, 122 ->
    // 117 on G.block2's backward), where K4V's im2col image stays conflict-free; at OW = 16 / 32 it is +5 % (D.block1)
    // or neutral
    else if (is_k4s2p1<G>() && !knobs().no_row4 && s.W == 2 * s.OW && s.H == 2 * s.OH && s.OW >= 16 && s.OW <= bm &&
             bm % s.OW == 0 && f.in16)
        c.loader = LRow4;
    return c;
}

template <class G>
inline Choice choose_dgrad(const ConvShape& s, const Facts& f) {
    const int ny = G::s * G::s;
    const long long M = (long long)s.N * (s.H / G::s) * (s.W / G::s), M4 = (long long)s.N * s.OH * s.OW / 4;
    if (s.H % G::s || s.W % G::s) return choice_of(KUnsupported, LGeneric, T64x64);
    SplitPlan sp = dgrad_plan<G>(s);
    if (!f.stats) {      // (a direct kernel keeps, as its gz_conv2d_tile label, the tile of the igemm launch it replaces)
        if (is_k3s1p1<G>() && conv3_smallch_ok(s.N, s.K, s.C, s.H, s.W))
            return choice_of(KDirect, conv3_fewk_ok(s.K, s.C, s.H, s.W) && f.in16 && f.out16 ? LFewk : LSmallch, sp.tile);
        if (dgrad_direct<G>(s) && f.out8) {
            Choice c = choice_of(KDirect, LSmallc, sp.tile);
            c.ks = smallc_four_pos(s) && f.in16 && f.out16 ? smallc_split(M4, s.K) : 0;
            return c;
        }
        if (is_k5s2p2<G>() && dgrad_direct5_ok(s) && f.in16 && f.out16) {
            Choice c = choice_of(KDirect, LSmallc5, sp.tile);
            c.ks = smallc_split(M4, s.K);
            return c;
        }
        if (is_k5s2p2<G>() && !f.epilogue && f.in16 && f.out16) {
            const Dg5Plan p5 = dgrad5_plan<G>(s);
            if (p5.ok && (p5.nz <= 1 || !ws_lacks(f, dgrad5_ws_bytes<G>(s)))) {
                Choice c = choice_of(KDg5, LRows2, T256x128P);
                c.splits = p5.splits;
                c.slabs = p5.nz;
                return c;
            }
        }
    }
    Choice c = choice_of(KIgemm, LGeneric, sp.tile);
    // (dgrad_ws_bytes is 0 for the shapes of the direct kernel: a launch that declined it still needs its slabs)
    if (sp.splits > 1 && ws_lacks(f, dgrad_ws_bytes<G>(s))) {
        c.ws_short = true;
        sp = SplitPlan{pick_tile(M, s.C, ny), 1};
    }
    if (is_tile2(sp.tile) && dgrad2_ok<G>(s) && !f.in16)      // unaligned tensor: the element-wise loaders
        sp = SplitPlan{pick_tile(M, s.C, ny), 1};
    c.tile = sp.tile;
    c.splits = sp.splits;
    if (is_tile2(c.tile)) {
        constexpr int TAPS = ((G::kh + G::s - 1) / G::s) * ((G::kw + G::s - 1) / G::s);
        const bool rows = dgrad2_ok<G>(s);
        c.loader = rows ? LRows2
                   : (is_k1<G>() && !knobs().no_plane_a && ((s.OH * s.OW) & 3) == 0 && f.in16) ? LPlane2 : LGather2;
        choose_igemm2(c, tile_count(c.tile, M, s.C, ny), rows ? 4 * s.K : TAPS * round_bk(s.K));
        return c;
    }
    if (dgrad_tap_major(s.K, G::kh, G::kw, G::s)) c.loader = LTap;
    // Row4 (GZ_NO_ROW4: per element): the shifted fragment reads stay inside the tile's LDS row only when every tile starts
    // a row of the per-phase grid (BM % AW == 0, as 256 % OW == 0 for ConvDgA2); 12-, 24- or 48-pixel rows take the
    // per-element loader
    else if (is_k4s2p1<G>() && !knobs().no_row4 && (s.W / 2) % 4 == 0 && (c.tile == T64x64 ? 64 : 128) % (s.W / 2) == 0 && f.in16)
        c.loader = LRow4;
    return c;
}

template <class G>
inline Choice choose_wgrad(const ConvShape& s, const Facts& f) {
    Choice c = choice_of(KIgemm, LGeneric, T64x64);
    const int KTOT = s.N * s.OH * s.OW, NTOT = s.C * G::kh * G::kw;
    const long long count = (long long)s.K * NTOT;
    // (the direct kernels keep, as their gz_conv2d_tile label, the tile of the igemm launch they replace)
    if (NTOT <= 32) c.tile = T128x32;
    else if (NTOT <= 64 || s.K <= 64) c.tile = s.K <= 64 ? T64x64 : T128x64;
    // split-K supplies the parallelism; with few pixels per split (small batches) the narrower
    // tile keeps more workgroups busy per slab byte
    else c.tile = KTOT >= 8192 ? T128x128 : T128x64;     // round 2: 128x128 now holds 4 workgroups per CU (was 65536)
    const int forced = forced_tile();
    if (forced >= 0 && forced <= 3 && !(forced == T128x128 && NTOT <= 64)) c.tile = (TileId)forced;
    if (wgrad_smallch_ok(s, G::kh, G::kw, G::s, G::p)) {
        c.kind = KDirect;
        c.loader = wgrad_fewk_ok(s) ? LFewk : LSmallch;
        c.slabs = wgrad_smallch_blocks(s);
        return c;
    }
    if (is_k4s2p1<G>() && wgrad_k4s2p1_fewc_ok(s) && f.ws_bytes >= (size_t)count * 4) {
        c.kind = KDirect;
        c.loader = LFewc;
        c.slabs = wgrad_k4s2p1_fewc_blocks(s);
        return c;
    }
    if (forced < 0 && wgrad2w_geom<G>()) {
        // igemm2: both operands by LDS-DMA (igemm2w: raw-row image, needs H = S * OH, rows of 4 / 8 / 16k pixels and
        // aligned tensors), or -- k4 s2 p1 only -- the register-staged row loaders (igemm2r)
        const int splits = wgrad2_splits<G>(s);
        c.cw = wgrad2w_cw_shape<G>(s);
        if (splits > 0 && (c.cw || is_k4s2p1<G>())) {
            c.kind = c.cw && f.in16 ? KIgemm2w : (is_k4s2p1<G>() ? KIgemm2r : KIgemm);
            c.tile = c.kind == KIgemm ? T128x128 : (wgrad2_narrow(s) ? T128x256 : T256x128);
            c.splits = splits;
        }
    }
    if (c.kind == KIgemm) {
        const int bm = c.tile == T64x64 ? 64 : 128, bn = c.tile == T128x128 ? 128 : (c.tile == T128x32 ? 32 : 64);
        const long long tiles = (long long)((s.K + bm - 1) / bm) * ((NTOT + bn - 1) / bn);
        c.splits = wgrad_splits(tiles, (KTOT + BK - 1) / BK, bm * bn >= 128 * 128);
        WgRowGeom rg;
        c.loader = !knobs().wg_generic && wg_row_geom<G>(s, &rg) ? LWgRow : LGeneric;
    }
    c.splits = wg_fit_splits(c.splits, f.ws_bytes, count);
    c.slabs = split_nz(KTOT, c.splits);
    return c;
}

// ---- convolution + BatchNorm statistics in one launch: partial rows per phase (tiles_m * WM) ---------------------
inline int stats_wm(TileId t) { return t == T128x32 ? 4 : 2; }
inline int stats_tm_rows(TileId t, long long M) {
    if (t == T256x256 || t == T256x128) return (int)((M + 255) / 256) * 2;
    if (t == T512x64) return (int)((M + 511) / 512) * 4;
    if (t == T256x64) return (int)((M + 255) / 256) * 2;
    const int bm = t == T64x64 ? 64 : 128;
    return (int)((M + bm - 1) / bm) * stats_wm(t);
}

}  // namespace gz

// (every unit that dispatches writes `using namespace gz;` first; CALL(G) is the unit's own expression over a geometry)
#define GZ_GEOM_DISPATCH_OR(CALL, ELSE)                                 \
    if (KH == 4 && KW == 4 && S == 2 && P == 1) return CALL(G4421);     \
    if (KH == 5 && KW == 5 && S == 2 && P == 2) return CALL(G5522);     \
    if (KH == 3 && KW == 3 && S == 1 && P == 1) return CALL(G3311);     \
    if (KH == 1 && KW == 1 && S == 1 && P == 0) return CALL(G1110);     \
    return ELSE;
#define GZ_GEOM_DISPATCH(CALL) GZ_GEOM_DISPATCH_OR(CALL, GZ_ERR_UNSUPPORTED)
