// F : y = conv(x, w) -- Conv2d forward; ConvTranspose2d input-gradient.  The run_* launchers that instantiate the
// forward kernels of the igemm2 skeleton (gz_igemm2_kernel.h), launch_fwd, which executes the Choice that choose_fwd
// (gz_conv2d_choose.h) returned, and the C-ABI entry points that launch.  The launchers of the igemm_kernel skeleton
// are a unit of their own, gz_conv_fwd_igemm.hip (reached through gz_conv_fwd.h): the forward family is the largest,
// and in one unit it alone would be most of a build's wall time.  Nothing here decides: a condition that selects a
// kernel or a loader belongs in gz_conv2d_choose.h.  (Siblings: gz_conv_dgrad.hip, gz_conv_wgrad.hip; the queries, the
// plan text and what the three ops are to each other: gz_conv.hip.)
#include "gz_conv_fwd.h"
#include "../../include/gz_ops.h"

namespace gz {

// k4 s2 p1 forward convolution on the igemm2 skeleton (raw input rows by LDS-DMA, taps on the fragment read)
// (PS: the pad-skip form of the loader, 4x4 output maps -- run_fwd2_ow)
template <class Cfg, int OWC, bool PS = false>
static int run_fwd2(const float* x, const float* wp, const float* bias, float* y, const ConvShape& s, int act,
                    float slope, hipStream_t st, int splits, float* slab, float* stats) {
    using AL = ConvFwdA2<Cfg::BM, OWC, PS>;
    using BL = MContigB2<Cfg::BN>;
    typename AL::Params pa{x, s, make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW)};
    const int M = s.N * s.OH * s.OW;
    EpiNCHWB::Params pe{y, M, s.K, s.OH * s.OW, make_fastdiv(s.OH * s.OW), bias, act, slope,
                        reinterpret_cast<f32x2*>(stats)};
    const int Kg = s.C * 16;
    typename BL::Params pb{wp, Kg, round4(s.K), round4(s.K), 0};
    return launch_igemm2<Cfg, AL, BL, EpiNCHWB>(pa, pb, pe, M, s.K, Kg, 1, splits, st, slab);
}

// any other geometry whose reduction is tap-major (5x5 s2 p2, 3x3 s1 p1, 1x1 ...): gather loader, 4-byte LDS-DMA
template <class G, class Cfg>
static int run_fwdtap2_impl(const float* x, const float* wp, const float* bias, float* y, const ConvShape& s, int act,
                            float slope, hipStream_t st, Loader ld, int splits, float* slab, float* stats) {
    using AL = ConvTapA2<Cfg::BM, G::kh, G::kw, G::s, G::p>;
    using BL = MContigB2<Cfg::BN>;
    typename AL::Params pa{x, s, make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW)};
    const int M = s.N * s.OH * s.OW;
    EpiNCHWB::Params pe{y, M, s.K, s.OH * s.OW, make_fastdiv(s.OH * s.OW), bias, act, slope,
                        reinterpret_cast<f32x2*>(stats)};
    const int Kt = G::kh * G::kw * round_bk(s.C);
    // (1x1: the plain [C][K] weight image IS the tap-major one; it has no padding rows, the descriptor ends at row C)
    typename BL::Params pb{wp, G::kh * G::kw == 1 ? s.C : Kt, round4(s.K), round4(s.K), 0};
    if constexpr (G::kh * G::kw == 1 && G::s == 1 && G::p == 0) {
        if (ld == LPlane2) {      // plain GEMM: 16-byte pieces
            using AP = PlaneA2<Cfg::BM>;
            typename AP::Params pp{x, s.C, s.H * s.W, M, make_fastdiv(s.H * s.W)};
            return launch_igemm2<Cfg, AP, BL, EpiNCHWB>(pp, pb, pe, M, s.K, Kt, 1, splits, st, slab);
        }
    }
    return launch_igemm2<Cfg, AL, BL, EpiNCHWB>(pa, pb, pe, M, s.K, Kt, 1, splits, st, slab);
}

// (k4 s2 p1 has loaders of its own: has_own_igemm2_loaders, gz_conv2d_choose.h)
template <class G, class Cfg>
static int run_fwdtap2(const float* x, const float* wp, const float* bias, float* y, const ConvShape& s, int act,
                       float slope, hipStream_t st, Loader ld, int splits, float* slab, float* stats) {
    if constexpr (has_own_igemm2_loaders<G>()) return GZ_ERR_UNSUPPORTED;
    else return run_fwdtap2_impl<G, Cfg>(x, wp, bias, y, s, act, slope, st, ld, splits, slab, stats);
}

template <class Cfg>
static int run_fwd2_ow(const float* x, const float* wp, const float* bias, float* y, const ConvShape& s, int act,
                       float slope, hipStream_t st, int splits, float* slab, float* stats) {
    switch (s.OW) {
        case 4:
            // 4x4 maps on 128-pixel wave tiles of at most 64 columns: the MFMAs on rows that are padding only are left out
            if constexpr (Cfg::TN <= 2) {
                if (s.OH == 4 && !knobs().no_padskip)
                    return run_fwd2<Cfg, 4, true>(x, wp, bias, y, s, act, slope, st, splits, slab, stats);
            }
            return run_fwd2<Cfg, 4>(x, wp, bias, y, s, act, slope, st, splits, slab, stats);
        case 8: return run_fwd2<Cfg, 8>(x, wp, bias, y, s, act, slope, st, splits, slab, stats);
        case 16: return run_fwd2<Cfg, 16>(x, wp, bias, y, s, act, slope, st, splits, slab, stats);
        case 32: return run_fwd2<Cfg, 32>(x, wp, bias, y, s, act, slope, st, splits, slab, stats);
        case 64: return run_fwd2<Cfg, 64>(x, wp, bias, y, s, act, slope, st, splits, slab, stats);
        default: return GZ_ERR_UNSUPPORTED;
    }
}

// ---------------------------------------------------------------------------
// F with run-time geometry (evaluation path: InceptionV3).  Always tap-major, channels padded to a chunk.
// ---------------------------------------------------------------------------
// (igemm_kernel: run_fwd_any, gz_conv_fwd_igemm.hip)
// round 6: the run-time geometries on the igemm2 skeleton (ConvTapAnyA2: 4-byte LDS-DMA gather, 16 channels at one tap
// per chunk; EpiNCHWBiasAct: lean stores with bias + ReLU) for launches that fill the chip unsplit -- most of InceptionV3
// at the evaluation batch.  64-column tiles when the output channels are a multiple of 64 but not of 128 (192, 320, 448).
// (which launches: fwd_any2_cols)
template <class Cfg>
static int run_fwd_any2(const float* x, const float* wp, const float* bias, float* y, const ConvShape& s, const AnyGeom& g,
                        int act, float slope, hipStream_t st, int y_image_channels) {
    using AL = ConvTapAnyA2<Cfg::BM>;
    using BL = MContigB2<Cfg::BN>;
    typename AL::Params pa{x, s, make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW), g.KH, g.KW, g.SH, g.SW, g.PH, g.PW};
    const int M = s.N * s.OH * s.OW;
    EpiNCHWBiasAct::Params pe{y, M, s.K, s.OH * s.OW, make_fastdiv(s.OH * s.OW), bias, act, slope, y_image_channels};
    const int Kt = g.KH * g.KW * round_bk(s.C);
    typename BL::Params pb{wp, Kt, round4(s.K), round4(s.K), 0};
    return launch_igemm2<Cfg, AL, BL, EpiNCHWBiasAct>(pa, pb, pe, M, s.K, Kt, 1, 1, st);
}

// the one function that executes a forward Choice
template <class G>
static int launch_fwd(const Choice& c, const float* x, const float* wp, const float* bias, float* y, const ConvShape& s,
                      int act, float slope, float* ws, float* stats, hipStream_t st) {
    float* slab = c.splits > 1 ? ws : nullptr;
    const Loader ld = c.loader;
    if (stats && c.ws_short) return GZ_ERR_WORKSPACE;       // the stats entry points take no unsplit fallback
    if (c.kind == KDirect) {
        if constexpr (is_k3s1p1<G>())
            return run_conv3_smallch(x, wp, bias, y, s.N, s.C, s.K, s.H, s.W, fwd_tap_major(s.C, 3, 3), 0, act, slope, st, ld);
        return GZ_ERR_UNSUPPORTED;
    }
    switch (c.tile) {
        case T256x256: return run_fwd2_ow<Cfg256x256>(x, wp, bias, y, s, act, slope, st, c.splits, slab, stats);
        case T256x64:
            if (ld != LRows2) return run_fwdtap2<G, Cfg256x64>(x, wp, bias, y, s, act, slope, st, ld, c.splits, slab, stats);
            return run_fwd2_ow<Cfg256x64>(x, wp, bias, y, s, act, slope, st, c.splits, slab, stats);
        case T256x128:
            if (ld != LRows2) return run_fwdtap2<G, Cfg256x128>(x, wp, bias, y, s, act, slope, st, ld, c.splits, slab, stats);
            return run_fwd2_ow<Cfg256x128>(x, wp, bias, y, s, act, slope, st, c.splits, slab, stats);
        default: return launch_fwd_igemm<G>(c, x, wp, bias, y, s, act, slope, slab, stats, st);      // (the igemm_kernel tiles)
    }
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_conv2d_fwd(const float* x, const float* wpack, const float* bias, float* y, float* workspace, size_t ws_bytes,
                  int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, int act,
                  float slope, hipStream_t stream) {
    gz::clear_stale_error();
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P)) return GZ_ERR_BAD_SHAPE;
    if (too_large((long long)N * C * H * W) || too_large((long long)N * K * OH * OW)) return GZ_ERR_TOO_LARGE;
    if (((uintptr_t)wpack & 15) || ((uintptr_t)y & 15)) return GZ_ERR_BAD_SHAPE;
    const Facts f = facts_of(x, y, workspace, ws_bytes, bias || act != ACT_NONE, false);
#define CALL(G) launch_fwd<G>(choose_fwd<G>(s, f), x, wpack, bias, y, s, act, slope, workspace, nullptr, stream)
    GZ_GEOM_DISPATCH(CALL)
#undef CALL
}

// ---- convolution + BatchNorm statistics in one launch --------------------------------------------------------
int gz_conv2d_fwd_stats_ws(const float* x, const float* wpack, float* y, float* stats, float* workspace, size_t ws_bytes,
                           int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P,
                           hipStream_t stream) {
    gz::clear_stale_error();
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P) || !stats) return GZ_ERR_BAD_SHAPE;
    if (gz_conv2d_fwd_stats_rows(N, C, H, W, K, OH, OW, KH, KW, S, P) <= 0) return GZ_ERR_UNSUPPORTED;
    if ((((uintptr_t)x | (uintptr_t)y) & 15) != 0) return GZ_ERR_BAD_SHAPE;      // 16-byte LDS-DMA pieces / row stores
    if (too_large((long long)N * C * H * W) || too_large((long long)N * K * OH * OW)) return GZ_ERR_TOO_LARGE;
    const Facts f = facts_of(x, y, workspace, ws_bytes, false, true);
#define CALL(G) launch_fwd<G>(choose_fwd<G>(s, f), x, wpack, nullptr, y, s, 0, 0.f, workspace, stats, stream)
    GZ_GEOM_DISPATCH(CALL)
#undef CALL
}

int gz_conv2d_fwd_stats(const float* x, const float* wpack, float* y, float* stats, int N, int C, int H, int W, int K,
                        int OH, int OW, int KH, int KW, int S, int P, hipStream_t stream) {
    return gz_conv2d_fwd_stats_ws(x, wpack, y, stats, nullptr, 0, N, C, H, W, K, OH, OW, KH, KW, S, P, stream);
}

int gz_conv2d_fwd_any(const float* x, const float* wpack, const float* bias, float* y, float* workspace,
                      size_t ws_bytes, int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int SH, int SW,
                      int PH, int PW, int act, float slope, hipStream_t stream) {
    gz::clear_stale_error();
    ConvShape s{N, C, H, W, K, OH, OW};
    AnyGeom g{KH, KW, SH, SW, PH, PW};
    if (!any_shape_ok(s, g)) return GZ_ERR_BAD_SHAPE;
    if ((long long)N * C * H * W * 4 >= (1ll << 31) || (long long)N * K * OH * OW * 4 >= (1ll << 31)) return GZ_ERR_TOO_LARGE;
    long long M = (long long)N * OH * OW;
    if (fwd_any2_cols(s, g, bias, act) == 64) return run_fwd_any2<Cfg256x64>(x, wpack, bias, y, s, g, act, slope, stream, K);
    SplitPlan sp = fwd_any_plan(s, g);
    if (sp.splits > 1 && (!workspace || ws_bytes < split_bytes(sp, M, K, KH * KW * round_bk(C), 1)))
        sp = SplitPlan{pick_tile(M, K, 1), 1};
    float* slab = sp.splits > 1 ? workspace : nullptr;
    return launch_fwd_any_igemm(sp, x, wpack, bias, y, s, g, act, slope, slab, stream);
}

int gz_conv2d_fwd_any_into(const float* x, const float* wpack, const float* bias, float* y, int y_image_channels, int N,
                           int C, int H, int W, int K, int OH, int OW, int KH, int KW, int SH, int SW, int PH, int PW,
                           int act, float slope, hipStream_t stream) {
    gz::clear_stale_error();
    ConvShape s{N, C, H, W, K, OH, OW};
    AnyGeom g{KH, KW, SH, SW, PH, PW};
    if (!any_shape_ok(s, g) || y_image_channels < K) return GZ_ERR_BAD_SHAPE;
    if ((long long)N * C * H * W * 4 >= (1ll << 31) || (long long)N * y_image_channels * OH * OW * 4 >= (1ll << 31))
        return GZ_ERR_TOO_LARGE;
    if (fwd_any2_cols(s, g, bias, act) != 64) return GZ_ERR_UNSUPPORTED;
    return run_fwd_any2<Cfg256x64>(x, wpack, bias, y, s, g, act, slope, stream, y_image_channels);
}

}  // extern "C"
