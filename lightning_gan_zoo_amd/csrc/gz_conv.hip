// The 2-D convolution family {F, Dg, Wg} and the plain GEMM: what of their C ABI launches no convolution kernel -- the
// workspace and statistics-row queries, gz_conv2d_tile, the text that describes a launch (gz_conv2d_plan), the CU
// budget -- and the plain GEMM with its launchers.
//
//   F  : y  = conv(x, w)                 Conv2d forward; ConvTranspose2d input-gradient
//   Dg : x  = conv_transpose(y, w)       Conv2d input-gradient; ConvTranspose2d forward
//   Wg : dw = sum_pixels y (x) patch(x)  weight gradient of either
//
// Each one's two partial derivatives are the other two with arguments permuted
// (SURVEY.md appendix C), so these three close the gradient-penalty double backward.
// Replaces, for the hot path, the aten ops behind torch.nn.Conv2d / ConvTranspose2d at
// reference core/models/standard_networks.py:20-24,36-43,60-73,80-87.
//
// The family is split by what changes together:
//   gz_conv2d_choose.h  the launch decision, host arithmetic only: which kernel a launch takes (choose_fwd /
//                       choose_dgrad / choose_wgrad return a Choice, gz_conv_choice.h) and the planners they read
//   gz_conv_fwd.hip, gz_conv_dgrad.hip, gz_conv_wgrad.hip
//                       one unit per op: the run_* launchers that instantiate the op's kernels of the fp32 MFMA
//                       implicit-GEMM skeletons (gz_igemm.h), launch_* -- the one function that executes the op's Choice
//                       -- and the entry points that launch.  The families of kernel instantiations compile side by
//                       side; F, the largest, is two units by skeleton (gz_conv_fwd_igemm.hip: igemm_kernel)
// Two more siblings hold what a choice can also land on or needs, neither built on the skeletons:
//   gz_conv_direct.hip  the direct kernels for few-channel layers (reached through gz_conv_direct.h)
//   gz_pack.hip         the weight packers and the slab sums (layout rules: gz_pack_layout.h; slab sums: gz_reduce.h)
#include <cstdio>

#include "gz_conv2d_choose.h"
#include "../../include/gz_ops.h"

namespace gz {

// ---------------------------------------------------------------------------
// plain GEMM  C[M][N] = op(A) . op(B)  (+bias[n], activation)
// ---------------------------------------------------------------------------
template <class Cfg, class AL, class BL>
static int run_gemm(const float* a, const float* b, const float* bias, float* c, int M, int N, int K, int lda,
                    int ldb, int ldc, int act, float slope, hipStream_t st, int splits, float* slab) {
    typename AL::Params pa{a, K, M, lda, 0};
    typename BL::Params pb{b, K, N, ldb, 0};
    EpiRowMajor::Params pe{c, M, N, ldc, 0, bias, act, slope};
    return launch_igemm<Cfg, AL, BL, EpiRowMajor>(pa, pb, pe, M, N, K, 1, splits, st, slab);
}

template <class Cfg>
static int gemm_ops(const float* a, const float* b, const float* bias, float* c, int M, int N, int K, int lda,
                    int ldb, int ldc, int ta, int tb, int act, float slope, hipStream_t st, int splits, float* slab) {
    // ta == 0: A is [M][K] row-major (k contiguous);  ta == 1: A is stored [K][M] (m contiguous)
    // tb == 0: B is [K][N] row-major (n contiguous);  tb == 1: B is stored [N][K] (k contiguous)
    const bool b_vec = !tb && (ldb % 4 == 0) && (N % 4 == 0) && (((uintptr_t)b & 15) == 0);
    if (!ta && !tb) {
        if (b_vec) return run_gemm<Cfg, KContigLoader<Cfg::BM>, MContigLoader4<Cfg::BN>>(a, b, bias, c, M, N, K, lda, ldb, ldc, act, slope, st, splits, slab);
        return run_gemm<Cfg, KContigLoader<Cfg::BM>, MContigLoader<Cfg::BN>>(a, b, bias, c, M, N, K, lda, ldb, ldc, act, slope, st, splits, slab);
    }
    if (ta && !tb) {
        if (b_vec) return run_gemm<Cfg, MContigLoader<Cfg::BM>, MContigLoader4<Cfg::BN>>(a, b, bias, c, M, N, K, lda, ldb, ldc, act, slope, st, splits, slab);
        return run_gemm<Cfg, MContigLoader<Cfg::BM>, MContigLoader<Cfg::BN>>(a, b, bias, c, M, N, K, lda, ldb, ldc, act, slope, st, splits, slab);
    }
    if (!ta && tb) return run_gemm<Cfg, KContigLoader<Cfg::BM>, KContigLoader<Cfg::BN>>(a, b, bias, c, M, N, K, lda, ldb, ldc, act, slope, st, splits, slab);
    return run_gemm<Cfg, MContigLoader<Cfg::BM>, KContigLoader<Cfg::BN>>(a, b, bias, c, M, N, K, lda, ldb, ldc, act, slope, st, splits, slab);
}

}  // namespace gz

using namespace gz;

extern "C" {

size_t gz_conv2d_fwd_workspace_bytes(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P) {
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P)) return 0;
#define CALL(G) fwd_ws_bytes<G>(s)
    GZ_GEOM_DISPATCH_OR(CALL, 0)
#undef CALL
}

size_t gz_conv2d_dgrad_workspace_bytes(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S,
                                       int P) {
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P)) return 0;
#define CALL(G) dgrad_ws_bytes<G>(s)
    GZ_GEOM_DISPATCH_OR(CALL, 0)
#undef CALL
}

size_t gz_conv2d_wgrad_workspace_bytes(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW) {
    long long count = (long long)K * C * KH * KW;
    ConvShape s{N, C, H, W, K, OH, OW};
    if (OH == H && OW == W && wgrad_smallch_ok(s, KH, KW, 1, 1)) return (size_t)wgrad_smallch_blocks(s) * (count + K) * 4;
    size_t fewc = 0;
    if (KH == 4 && KW == 4 && wgrad_k4s2p1_fewc_ok(s)) fewc = (size_t)wgrad_k4s2p1_fewc_blocks(s) * (count + K) * 4;
    int chunks = (N * OH * OW + BK - 1) / BK;
    // upper bound over the tile choices: smallest tile count is with 128x128 tiles
    long long tiles = (long long)((K + 127) / 128) * ((C * KH * KW + 127) / 128);
    int splits = wgrad_splits(tiles, chunks);
    {                                    // the igemm2 plans may split further
        const int s2 = (KH == 4 && KW == 4) ? wgrad2_splits<G4421>(s)
                       : (KH == 5 && KW == 5 && OH * 2 == H) ? wgrad2_splits<G5522>(s)
                       : (KH == 3 && KW == 3 && OH == H) ? wgrad2_splits<G3311>(s) : 0;
        if (s2 > splits) splits = s2;
    }
    const size_t generic = splits > 1 ? (size_t)splits * count * 4 : 0;
    return generic > fewc ? generic : fewc;
}

int gz_set_cu_budget(int cu_count) {
    if (cu_count <= 0) cu_count = 256;
    if (cu_count < 64) cu_count = 64;
    if (cu_count > 256) cu_count = 256;
    gz::cu_budget_ref().store(cu_count, std::memory_order_relaxed);
    return cu_count;
}

int gz_get_cu_budget(void) { return gz::cus(); }

// ---- convolution + BatchNorm statistics in one launch: how many partial rows the launch writes -------------------
int gz_conv2d_fwd_stats_rows(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P) {
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P)) return 0;
    const Facts f{true, true, true, kIdeal.ws_bytes, false, true, true};
#define CALL(G) choose_fwd<G>(s, f)
    const Choice sp = [&]() -> Choice { GZ_GEOM_DISPATCH_OR(CALL, (Choice{KIgemm, LGeneric, T64x64, 2})) }();
#undef CALL
    // split launches (round 4): splitk_finish_kernel runs the same epilogue per 32 x 32 output block and writes the
    // statistics there -- one partial row per 32 pixels
    if (sp.splits > 1) return (int)(((long long)N * OH * OW + 31) / 32);
    return stats_tm_rows(sp.tile, (long long)N * OH * OW);      // (the tap-major gather launches do carry them)
}

int gz_conv2d_dgrad_stats_rows(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P) {
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P) || H % S || W % S) return 0;
    const Facts f{true, true, true, kIdeal.ws_bytes, false, true, true};
    // the choice gz_conv2d_dgrad_stats_ws launches (f.stats: no direct kernel), also for the <= 4-channel shapes of the
    // direct kernel: their unsplit igemm launch writes tiles_m * WM rows per phase, not one per 32 pixels
#define CALL(G) choose_dgrad<G>(s, f)
    const Choice sp = [&]() -> Choice { GZ_GEOM_DISPATCH_OR(CALL, (Choice{KIgemm, LGeneric, T64x64, 2})) }();
#undef CALL
    if (is_tile2(sp.tile) && !(KH == 4 && KW == 4 && S == 2 && P == 1)) return 0;      // gather-loader launches: not fused
    if (sp.splits > 1) {          // the finish kernel writes them, one partial row per 32 pixels of a phase (round 4)
        if (!(KH == 4 && KW == 4 && S == 2 && P == 1)) return 0;       // phases of unequal length: own slab map, not fused
        return S * S * (int)(((long long)N * (H / S) * (W / S) + 31) / 32);
    }
    return S * S * stats_tm_rows(sp.tile, (long long)N * (H / S) * (W / S));
}

size_t gz_conv2d_fwd_any_workspace_bytes(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int SH,
                                         int SW, int PH, int PW) {
    ConvShape s{N, C, H, W, K, OH, OW};
    AnyGeom g{KH, KW, SH, SW, PH, PW};
    if (!any_shape_ok(s, g)) return 0;
    return split_bytes(fwd_any_plan(s, g), (long long)N * OH * OW, K, KH * KW * round_bk(C), 1);
}

#ifdef GZ2_STAMPS
/* diagnostic builds only: copies the per-workgroup stamps of the last igemm2 launch (n x 8 x u64), from the array of
 * the unit that launched it (gz2_last_stamps, gz_igemm2_kstep.h) */
int gz_debug_read_stamps(void* out, int nwg) {
    if (!gz::gz2_last_stamps()) return GZ_ERR_UNSUPPORTED;      // no igemm2 launch yet
    return hip_status(hipMemcpyFromSymbol(out, gz::gz2_last_stamps(), (size_t)nwg * 64, 0, hipMemcpyDeviceToHost));
}
#endif

/* which tile configuration a launch of op (0 F, 1 Dg, 2 Wg) would use, a TileId: 0 128x128, 1 128x64, 2 128x32,
 * 3 64x64, 4.. the igemm2 tiles.  A label for timers: the tile of the launch's choice for ideal facts.  The call has
 * no padding argument (the four geometries differ in their kernel size); a shape or geometry that no launch exists
 * for gets 3. */
int gz_conv2d_tile(int op, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S) {
    const int P = KH == 5 ? 2 : KH == 1 ? 0 : 1;
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P)) return T64x64;
#define CALL(G) (op == 0 ? choose_fwd<G>(s, kIdeal) : op == 1 ? choose_dgrad<G>(s, kIdeal) : choose_wgrad<G>(s, kIdeal)).tile
    GZ_GEOM_DISPATCH_OR(CALL, T64x64)
#undef CALL
}

/* ---- which kernel a launch takes, as text (round 4: the dispatch is pinned by tests/test_dispatch_plan.py) ---------
 * Runs on the CPU (no HIP call).  Describes the launch for 16-byte aligned tensors and a workspace of the advertised
 * size -- an unaligned view or a missing workspace falls back to the element-wise loaders / an unsplit plan. */
}  // extern "C" (the describe_* templates need C++ linkage)

template <class G>
static int describe_fwd(const ConvShape& s, char* b, size_t n) {
    const Choice c = choose_fwd<G>(s, kIdeal);
    if (c.kind == KDirect)
        return snprintf(b, n, "F direct %s", c.loader == LFewk ? "conv3x3_fewk<fma>" : "conv3x3_smallch<mfma16x16x4>");
    const int rows = gz_conv2d_fwd_stats_rows(s.N, s.C, s.H, s.W, s.K, s.OH, s.OW, G::kh, G::kw, G::s, G::p);
    if (c.kind == KIgemm2)      // (PlaneA2 launches are described by the gather loader they stand in for)
        return snprintf(b, n, "F igemm2<%s> %s slabs=%d bn_stats_rows=%d%s", tile_text(c.tile),
                        c.loader == LRows2 ? "ConvFwdA2(raw rows, LDS-DMA 16B)" : "ConvTapA2(gather, LDS-DMA 4B)", c.slabs,
                        rows, c.wave_groups == 2 ? " wave_groups=2" : "");
    return snprintf(b, n, "F igemm<%s> %s slabs=%d bn_stats_rows=%d", tile_text(c.tile),
                    c.loader == LTap ? "ConvFwdALoaderTap" : c.loader == LRow4 ? "ConvFwdALoaderRow4"
                    : is_k4s2p1<G>() ? "ConvFwdALoaderK4V" : "ConvFwdALoader", c.slabs, rows);
}

template <class G>
static int describe_dgrad(const ConvShape& s, char* b, size_t n) {
    const Choice c = choose_dgrad<G>(s, kIdeal);
    if (c.kind == KUnsupported) return snprintf(b, n, "Dg unsupported (H, W not multiples of the stride)");
    if (c.kind == KDirect && c.loader == LSmallc5)
        return snprintf(b, n, "Dg direct dgrad_smallc4_k5s2p2<C=%d,KS=%d>", s.C, c.ks);
    if (c.kind == KDirect && c.loader == LSmallc && c.ks > 0)
        return snprintf(b, n, "Dg direct dgrad_smallc4_k4s2p1<C=%d,KS=%d>", s.C, c.ks);
    if (c.kind == KDirect && c.loader == LSmallc) return snprintf(b, n, "Dg direct dgrad_smallc_k4s2p1<C=%d>", s.C);
    if (c.kind == KDirect) return snprintf(b, n, "Dg direct conv3x3_smallch<mfma16x16x4>");      // (either 3x3 kernel)
    if (c.kind == KDg5)
        return snprintf(b, n, "Dg igemm2<256x(4 phases x 32)> ConvDg5A2(row-shared, LDS-DMA 16B, 12 k-steps) slabs=%d "
                              "(no bias / activation, aligned tensors; else the gather loader)", c.slabs);
    const int rows = gz_conv2d_dgrad_stats_rows(s.N, s.C, s.H, s.W, s.K, s.OH, s.OW, G::kh, G::kw, G::s, G::p);
    if (c.kind == KIgemm2)
        return snprintf(b, n, "Dg igemm2<%s> %s splits=%d bn_stats_rows=%d%s", tile_text(c.tile),
                        c.loader == LRows2 ? "ConvDgA2(row-shared, LDS-DMA 16B)" : "ConvDgTapA2(gather, LDS-DMA 4B)",
                        c.splits, rows, c.wave_groups == 2 ? " wave_groups=2" : "");
    return snprintf(b, n, "Dg igemm<%s> %s splits=%d bn_stats_rows=%d", tile_text(c.tile),
                    c.loader == LTap ? "ConvDgALoaderTap" : c.loader == LRow4 ? "ConvDgALoaderRow4" : "ConvDgALoader",
                    c.splits, rows);
}

template <class G>
static int describe_wgrad(const ConvShape& s, char* b, size_t n) {
    const Choice c = choose_wgrad<G>(s, kIdeal);
    if (c.kind == KDirect && c.loader == LFewc)
        return snprintf(b, n, "Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=%d,KT=%d> slabs=%d", s.C, s.K / 16, c.slabs);
    if (c.kind == KDirect)
        return snprintf(b, n, "Wg direct %s slabs=%d", c.loader == LFewk ? "wgrad_k3_fewk<fma>" : "wgrad_smallch_k3<mfma16x16x4>",
                        c.slabs);
    if (c.kind == KIgemm2w)
        return snprintf(b, n, "Wg igemm2w<%s> %s<CW=%d>(both operands LDS-DMA) slabs=%d", tile_text(c.tile),
                        is_k4s2p1<G>() ? "WgImgB2" : "WgImgBG", c.cw, c.slabs);
    if (c.kind == KIgemm2r)
        return snprintf(b, n, "Wg igemm2r<%s> WgALoaderRow+WgBLoaderRow(register-staged) slabs=%d", tile_text(c.tile), c.slabs);
    return snprintf(b, n, "Wg igemm<%s> %s slabs=%d", tile_text(c.tile),
                    c.loader == LWgRow ? "WgALoaderRow+WgBLoaderRow" : "WgALoader+WgBLoader", c.slabs);
}

extern "C" {

int gz_conv2d_plan(int op, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, char* buf,
                   int buflen) {
    if (!buf || buflen <= 0) return GZ_ERR_BAD_SHAPE;
    buf[0] = 0;
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P) || op < 0 || op > 2) return GZ_ERR_BAD_SHAPE;
    const size_t n = (size_t)buflen;
#define CALL(G) (op == 0 ? describe_fwd<G>(s, buf, n) : op == 1 ? describe_dgrad<G>(s, buf, n) : describe_wgrad<G>(s, buf, n))
    GZ_GEOM_DISPATCH(CALL)
#undef CALL
}

size_t gz_gemm_workspace_bytes(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return split_bytes(plan_split(M, N, K, 1, pick_tile(M, N, 1)), M, N, K, 1);
}

int gz_gemm(const float* a, const float* b, const float* bias, float* c, float* workspace, size_t ws_bytes, int M,
            int N, int K, int lda, int ldb, int ldc, int trans_a, int trans_b, int act, float slope,
            hipStream_t stream) {
    gz::clear_stale_error();
    if (M <= 0 || N <= 0 || K <= 0) return GZ_ERR_BAD_SHAPE;
    if (too_large((long long)M * K) || too_large((long long)K * N) || too_large((long long)M * N)) return GZ_ERR_TOO_LARGE;
    SplitPlan sp = plan_split(M, N, K, 1, pick_tile(M, N, 1));
    if (sp.splits > 1 && (!workspace || ws_bytes < split_bytes(sp, M, N, K, 1))) sp = SplitPlan{pick_tile(M, N, 1), 1};
    float* slab = sp.splits > 1 ? workspace : nullptr;
    switch (sp.tile) {
        case T128x128: return gemm_ops<Cfg128x128>(a, b, bias, c, M, N, K, lda, ldb, ldc, trans_a, trans_b, act, slope, stream, sp.splits, slab);
        case T128x64: return gemm_ops<Cfg128x64>(a, b, bias, c, M, N, K, lda, ldb, ldc, trans_a, trans_b, act, slope, stream, sp.splits, slab);
        case T128x32: return gemm_ops<Cfg128x32>(a, b, bias, c, M, N, K, lda, ldb, ldc, trans_a, trans_b, act, slope, stream, sp.splits, slab);
        default: return gemm_ops<Cfg64x64>(a, b, bias, c, M, N, K, lda, ldb, ldc, trans_a, trans_b, act, slope, stream, sp.splits, slab);
    }
}

}  // extern "C"
