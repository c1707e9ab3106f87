// Dg : x = conv_transpose(y, w) -- Conv2d input-gradient; ConvTranspose2d forward.  The run_* launchers that
// instantiate the transposed-convolution kernels of both implicit-GEMM skeletons (gz_igemm.h), launch_dgrad, which
// executes the Choice that choose_dgrad (gz_conv2d_choose.h) returned, and the C-ABI entry points that launch.  Nothing
// here decides: a condition that selects a kernel or a loader belongs in gz_conv2d_choose.h.  (Siblings:
// gz_conv_fwd.hip, gz_conv_wgrad.hip; the queries, the plan text and what the three ops are to each other: gz_conv.hip.)
#include <type_traits>

#include "gz_conv2d_choose.h"
#include "../../include/gz_ops.h"

namespace gz {

template <class G, class Cfg>
static int run_dgrad(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act,
                     float slope, hipStream_t st, Loader ld, int splits, float* slab, float* stats) {
    using AL = ConvDgALoader<Cfg::BM, G::kh, G::kw, G::s, G::p>;
    using BL = MContigLoader4<Cfg::BN>;
    using Epi = EpiPhaseB<G::s>;
    const int AH = s.H / G::s, AW = s.W / G::s;
    typename AL::Params pa{y, s, AH, AW, make_fastdiv(AH * AW), make_fastdiv(AW)};
    int Kg = s.K * AL::TAPS;
    int ldc = round4(s.C);
    typename BL::Params pb{wp, Kg, ldc, ldc, (long long)Kg * ldc};
    int M = s.N * AH * AW;
    typename Epi::Params pe{x, M, s.C, s.H, s.W, AH, AW, make_fastdiv(AH * AW), make_fastdiv(AW), bias, act, slope,
                            reinterpret_cast<f32x2*>(stats),
                            (splits > 1 && slab) ? (M + 31) / 32 : ((M + Cfg::BM - 1) / Cfg::BM) * Cfg::WM};
    if constexpr (!AL::FIXED) {
        if (ld == LTap) {
            using ALT = ConvDgALoaderTap<Cfg::BM, G::kh, G::kw, G::s, G::p>;
            typename ALT::Params pat{y, s, AH, AW, make_fastdiv(AH * AW), make_fastdiv(AW)};
            const int kpad = round_bk(s.K);
            int Kt = AL::TAPS * kpad;
            typename BL::Params pbt{wp, Kt, ldc, ldc, (long long)Kt * ldc};
            int pc[8];
            for (int ph = 0; ph < G::s * G::s; ++ph)
                pc[ph] = dg_taps(G::kh, G::s, G::p, ph / G::s) * dg_taps(G::kw, G::s, G::p, ph % G::s) * (kpad / BK);
            return launch_igemm<Cfg, ALT, BL, Epi>(pat, pbt, pe, M, s.C, Kt, G::s * G::s, splits, st, slab, pc);
        }
    }
    if constexpr (!AL::UNIFORM) {
        // phases differ in their tap count, hence in the length of their reduction
        int pc[8];
        for (int ph = 0; ph < G::s * G::s; ++ph)
            pc[ph] = (s.K * dg_taps(G::kh, G::s, G::p, ph / G::s) * dg_taps(G::kw, G::s, G::p, ph % G::s) + BK - 1) / BK;
        return launch_igemm<Cfg, AL, BL, Epi>(pa, pb, pe, M, s.C, Kg, G::s * G::s, splits, st, slab, pc);
    }
    if constexpr (G::kh == 4 && G::kw == 4 && G::s == 2 && G::p == 1) {
        if (ld == LRow4) {
            using AR = ConvDgALoaderRow4<Cfg::BM, 4, 4, 2, 1>;
            return launch_igemm<Cfg, AR, BL, Epi>(pa, pb, pe, M, s.C, Kg, G::s * G::s, splits, st, slab);
        }
    }
    return launch_igemm<Cfg, AL, BL, Epi>(pa, pb, pe, M, s.C, Kg, G::s * G::s, splits, st, slab);
}

// k4 s2 p1 transposed convolution on the igemm2 skeleton (row-shared A rows by LDS-DMA, packed per-phase weights)
// (PS: the pad-skip form of the loader, 4x4 feature maps)
template <class Cfg, bool PS = false>
static int run_dgrad2(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act,
                      float slope, hipStream_t st, int splits, float* slab, float* stats) {
    using AL = ConvDgA2<Cfg::BM, PS>;
    using BL = MContigB2<Cfg::BN>;
    using Epi = EpiPhaseB<2>;
    const int AH = s.H / 2, AW = s.W / 2;
    if constexpr (!PS && Cfg::BM == 256 && Cfg::TN <= 2) {
        if (AH == 4 && AW == 4 && !knobs().no_padskip)
            return run_dgrad2<Cfg, true>(y, wp, bias, x, s, act, slope, st, splits, slab, stats);
    }
    typename AL::Params pa{y, s, AH, AW, make_fastdiv(AH * AW), make_fastdiv(AW)};
    const int Kg = s.K * 4;
    const int ldc = round4(s.C);
    typename BL::Params pb{wp, Kg, ldc, ldc, (long long)Kg * ldc};
    const int M = s.N * AH * AW;
    // rows of partial statistics per phase: one per wavefront row of a tile, or -- split launch: the finish kernel
    // runs the epilogue per 32 x 32 block -- one per 32 pixels
    typename Epi::Params pe{x, M, s.C, s.H, s.W, AH, AW, make_fastdiv(AH * AW), make_fastdiv(AW), bias, act, slope,
                            reinterpret_cast<f32x2*>(stats),
                            (splits > 1 && slab) ? (M + 31) / 32 : ((M + Cfg::BM - 1) / Cfg::BM) * Cfg::WM};
    return launch_igemm2<Cfg, AL, BL, Epi>(pa, pb, pe, M, s.C, Kg, 4, splits, st, slab);
}

// transposed convolutions whose reduction is tap-major and whose phases differ in length (5x5 s2 p2: 9 / 6 / 6 / 4
// taps): gather loader with 4-byte LDS-DMA; the reduction is cut into pieces of ~48 chunks so that the phases'
// workgroups balance (unsplit, the 9-tap phase's workgroups would run 2.25x longer than the 4-tap phase's)
template <class G, class Cfg>
static int run_dgradtap2_impl(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act,
                              float slope, hipStream_t st, Loader ld, int splits, float* slab) {
    using AL = ConvDgTapA2<Cfg::BM, G::kh, G::kw, G::s, G::p>;
    using BL = MContigB2<Cfg::BN>;
    using Epi = EpiPhaseB<G::s>;
    const int AH = s.H / G::s, AW = s.W / G::s;
    typename AL::Params pa{y, s, AH, AW, make_fastdiv(AH * AW), make_fastdiv(AW)};
    const int kpad = round_bk(s.K);
    const int Kt = AL::Geo::TY * AL::Geo::TX * kpad;
    const int ldc = round4(s.C);
    // (1x1: the plain [K][C] image, without padding rows)
    const int Kb = G::kh * G::kw == 1 ? s.K : Kt;
    typename BL::Params pb{wp, Kb, ldc, ldc, (long long)Kb * ldc};
    const int M = s.N * AH * AW;
    typename Epi::Params pe{x, M, s.C, s.H, s.W, AH, AW, make_fastdiv(AH * AW), make_fastdiv(AW), bias, act, slope,
                            nullptr, 0};
    int pc[8];
    for (int ph = 0; ph < G::s * G::s; ++ph)
        pc[ph] = dg_taps(G::kh, G::s, G::p, ph / G::s) * dg_taps(G::kw, G::s, G::p, ph % G::s) * (kpad / BK);
    if constexpr (G::kh * G::kw == 1 && G::s == 1 && G::p == 0) {
        if (ld == LPlane2) {
            using AP = PlaneA2<Cfg::BM>;
            typename AP::Params pp{y, s.K, s.OH * s.OW, M, make_fastdiv(s.OH * s.OW)};
            return launch_igemm2<Cfg, AP, BL, Epi>(pp, pb, pe, M, s.C, Kt, 1, splits, st, slab, pc);
        }
    }
    return launch_igemm2<Cfg, AL, BL, Epi>(pa, pb, pe, M, s.C, Kt, G::s * G::s, splits, st, slab, pc);
}

template <class G, class Cfg>
static int run_dgradtap2(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act,
                         float slope, hipStream_t st, Loader ld, int splits, float* slab) {
    if constexpr (has_own_igemm2_loaders<G>()) return GZ_ERR_UNSUPPORTED;     // (gz_conv2d_choose.h)
    else return run_dgradtap2_impl<G, Cfg>(y, wp, bias, x, s, act, slope, st, ld, splits, slab);
}

// 5x5 s2 p2 on row-shared LDS rows, all four output phases per workgroup (the plan and what it measured: dgrad5_plan)
using CfgQuad = TileCfg2<4, 1, 4, 2, 2>;       // four wavefronts of 64 pixels x (4 phases x 32 channels)
static int run_dgrad5(const float* y, const float* wp, float* x, const ConvShape& s, hipStream_t st, int splits,
                      float* slab) {
    using Cfg = CfgQuad;
    using AL = ConvDg5A2<Cfg::BM>;
    using BL = DgQuadB2;
    using Epi = EpiPhaseQuadB;
    const int AH = s.OH, AW = s.OW;
    typename AL::Params pa{y, s, AH, AW, make_fastdiv(AH * AW), make_fastdiv(AW)};
    typename BL::Params pb{wp, s.K, s.C, round4(s.C)};
    const int M = s.N * AH * AW;
    typename Epi::Params pe{x, M, s.C, s.H, s.W, AH, AW, make_fastdiv(AH * AW), make_fastdiv(AW), nullptr, ACT_NONE, 0.f,
                            nullptr, 0};
    return launch_igemm2<Cfg, AL, BL, Epi>(pa, pb, pe, M, 4 * s.C, 6 * s.K, 1, splits, st, slab);
}

// the one function that executes an input-gradient Choice
template <class G>
static int launch_dgrad(const Choice& c, const float* y, const float* wp, const float* bias, float* x, const ConvShape& s,
                        int act, float slope, float* ws, float* stats, hipStream_t st) {
    float* slab = c.splits > 1 ? ws : nullptr;
    const Loader ld = c.loader;
    if (c.kind == KUnsupported) return GZ_ERR_UNSUPPORTED;
    if (stats && c.ws_short) return GZ_ERR_WORKSPACE;       // the stats entry points take no unsplit fallback
    if (c.kind == KDg5) return run_dgrad5(y, wp, x, s, st, c.splits, c.slabs > 1 ? ws : nullptr);
    if (c.kind == KDirect && (ld == LFewk || ld == LSmallch)) {
        if constexpr (is_k3s1p1<G>())
            return run_conv3_smallch(y, wp, bias, x, s.N, s.K, s.C, s.H, s.W, dgrad_tap_major(s.K, 3, 3, 1), 1, act, slope, st, ld);
        return GZ_ERR_UNSUPPORTED;
    }
    if (c.kind == KDirect)
        return ld == LSmallc5 ? run_dgrad_smallc5(y, wp, bias, x, s, act, slope, st, c.ks)
                              : run_dgrad_smallc(y, wp, bias, x, s, act, slope, st, c.ks);
    switch (c.tile) {
        case T256x256: return run_dgrad2<Cfg256x256>(y, wp, bias, x, s, act, slope, st, 1, nullptr, stats);
        case T256x128:
            if (ld != LRows2) return run_dgradtap2<G, Cfg256x128>(y, wp, bias, x, s, act, slope, st, ld, c.splits, slab);
            return run_dgrad2<Cfg256x128>(y, wp, bias, x, s, act, slope, st, c.splits, slab, stats);
        case T512x64: return run_dgrad2<Cfg512x64>(y, wp, bias, x, s, act, slope, st, 1, nullptr, stats);
        case T256x64:
            if (ld != LRows2) return run_dgradtap2<G, Cfg256x64>(y, wp, bias, x, s, act, slope, st, ld, c.splits, slab);
            return run_dgrad2<Cfg256x64>(y, wp, bias, x, s, act, slope, st, c.splits, slab, stats);
        case T128x128: return run_dgrad<G, Cfg128x128>(y, wp, bias, x, s, act, slope, st, ld, c.splits, slab, stats);
        case T128x64: return run_dgrad<G, Cfg128x64>(y, wp, bias, x, s, act, slope, st, ld, c.splits, slab, stats);
        case T128x32: return run_dgrad<G, Cfg128x32>(y, wp, bias, x, s, act, slope, st, ld, c.splits, slab, stats);
        default: return run_dgrad<G, Cfg64x64>(y, wp, bias, x, s, act, slope, st, ld, c.splits, slab, stats);
    }
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_conv2d_dgrad(const float* y, const float* wpack, const float* bias, float* x, float* workspace,
                    size_t ws_bytes, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P,
                    int act, float slope, hipStream_t stream) {
    gz::clear_stale_error();
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P)) return GZ_ERR_BAD_SHAPE;
    if (too_large((long long)N * C * H * W) || too_large((long long)N * K * OH * OW)) return GZ_ERR_TOO_LARGE;
    if ((uintptr_t)wpack & 15) return GZ_ERR_BAD_SHAPE;
    const Facts f = facts_of(y, x, workspace, ws_bytes, bias || act != ACT_NONE, false);
#define CALL(G) launch_dgrad<G>(choose_dgrad<G>(s, f), y, wpack, bias, x, s, act, slope, workspace, nullptr, stream)
    GZ_GEOM_DISPATCH(CALL)
#undef CALL
}

static bool dgrad_act_direct(const ConvShape& s, int KH, int KW, int S, int P, int act) {
    return KH == 4 && KW == 4 && S == 2 && P == 1 && (act == ACT_RELU || act == ACT_LRELU) && !knobs().no_act_fuse &&
           dgrad_direct<G4421>(s) && smallc_four_pos(s);
}

int gz_conv2d_dgrad_act_fuses(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, int act) {
    ConvShape s{N, C, H, W, K, OH, OW};
    return shape_ok(s, KH, KW, S, P) && dgrad_act_direct(s, KH, KW, S, P, act) ? 1 : 0;
}

int gz_conv2d_dgrad_act(const float* gy, const float* fwd_out, int act, float slope, const float* wpack, float* x, int N,
                        int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, hipStream_t stream) {
    gz::clear_stale_error();
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!gy || !fwd_out || !wpack || !x || !shape_ok(s, KH, KW, S, P)) return GZ_ERR_BAD_SHAPE;
    if (too_large((long long)N * C * H * W) || too_large((long long)N * K * OH * OW)) return GZ_ERR_TOO_LARGE;
    if (!dgrad_act_direct(s, KH, KW, S, P, act) || (((uintptr_t)gy | (uintptr_t)x | (uintptr_t)fwd_out | (uintptr_t)wpack) & 15))
        return GZ_ERR_UNSUPPORTED;
    const float neg = act == ACT_RELU ? 0.f : slope;
    const int ks = smallc_split((long long)N * OH * OW / 4, K);
    return run_dgrad_smallc(gy, wpack, nullptr, x, s, ACT_NONE, 0.f, stream, ks, fwd_out, neg);
}

// ---- convolution + BatchNorm statistics in one launch --------------------------------------------------------
int gz_conv2d_dgrad_stats_ws(const float* y, const float* wpack, float* x, float* stats, float* workspace,
                             size_t ws_bytes, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S,
                             int P, hipStream_t stream) {
    gz::clear_stale_error();
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P) || !stats) return GZ_ERR_BAD_SHAPE;
    if (gz_conv2d_dgrad_stats_rows(N, C, H, W, K, OH, OW, KH, KW, S, P) <= 0) return GZ_ERR_UNSUPPORTED;
    if ((((uintptr_t)x | (uintptr_t)y) & 15) != 0) return GZ_ERR_BAD_SHAPE;      // 16-byte LDS-DMA pieces / row stores
    if (too_large((long long)N * C * H * W) || too_large((long long)N * K * OH * OW)) return GZ_ERR_TOO_LARGE;
    const Facts f = facts_of(y, x, workspace, ws_bytes, false, true);
#define CALL(G) launch_dgrad<G>(choose_dgrad<G>(s, f), y, wpack, nullptr, x, s, 0, 0.f, workspace, stats, stream)
    GZ_GEOM_DISPATCH(CALL)
#undef CALL
}

int gz_conv2d_dgrad_stats(const float* y, const float* wpack, float* x, float* stats, int N, int C, int H, int W, int K,
                          int OH, int OW, int KH, int KW, int S, int P, hipStream_t stream) {
    return gz_conv2d_dgrad_stats_ws(y, wpack, x, stats, nullptr, 0, N, C, H, W, K, OH, OW, KH, KW, S, P, stream);
}

}  // extern "C"
