// F on the igemm_kernel skeleton (gz_igemm_core.h): run_fwd and run_fwd_any, the launchers that instantiate its forward
// kernels, and the two functions gz_conv_fwd.hip reaches them through (gz_conv_fwd.h).  A unit of its own only so that
// the forward family's two skeletons compile side by side.  Nothing here decides: see gz_conv2d_choose.h.
#include <type_traits>

#include "gz_conv_fwd.h"
#include "../../include/gz_ops.h"

namespace gz {

template <class G, class Cfg>
static int run_fwd(const float* x, const float* wp, const float* bias, float* y, const ConvShape& s, int act,
                   float slope, hipStream_t st, Loader ld, int splits, float* slab, float* stats) {
#ifndef GZ_NO_K4V
    using AL = std::conditional_t<G::kh == 4 && G::kw == 4, ConvFwdALoaderK4V<Cfg::BM, G::s, G::p>,
                                  ConvFwdALoader<Cfg::BM, G::kh, G::kw, G::s, G::p>>;
#else
    using AL = ConvFwdALoader<Cfg::BM, G::kh, G::kw, G::s, G::p>;
#endif
    using BL = MContigLoader4<Cfg::BN>;
    typename AL::Params pa{x, s, make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW)};
    int M = s.N * s.OH * s.OW;
    EpiNCHWB::Params pe{y, M, s.K, s.OH * s.OW, make_fastdiv(s.OH * s.OW), bias, act, slope,
                       reinterpret_cast<f32x2*>(stats)};
    if constexpr (BK % (G::kh * G::kw) != 0) {
        if (ld == LTap) {
            using ALT = ConvFwdALoaderTap<Cfg::BM, G::kh, G::kw, G::s, G::p>;
            int Kt = G::kh * G::kw * round_bk(s.C);
            typename BL::Params pbt{wp, Kt, round4(s.K), round4(s.K), 0};
            return launch_igemm<Cfg, ALT, BL, EpiNCHWB>(pa, pbt, pe, M, s.K, Kt, 1, splits, st, slab);
        }
    }
    int Kg = s.C * G::kh * G::kw;
    typename BL::Params pb{wp, Kg, round4(s.K), round4(s.K), 0};
    if constexpr (G::kh == 4 && G::kw == 4 && G::s == 2 && G::p == 1) {
        if (ld == LRow4) {
            using AR = ConvFwdALoaderRow4<Cfg::BM>;
            return launch_igemm<Cfg, AR, BL, EpiNCHWB>(pa, pb, pe, M, s.K, Kg, 1, splits, st, slab);
        }
    }
    return launch_igemm<Cfg, AL, BL, EpiNCHWB>(pa, pb, pe, M, s.K, Kg, 1, splits, st, slab);
}

template <class G>
int launch_fwd_igemm(const Choice& c, const float* x, const float* wp, const float* bias, float* y, const ConvShape& s,
                     int act, float slope, float* slab, float* stats, hipStream_t st) {
    const Loader ld = c.loader;
    switch (c.tile) {
        case T128x128: return run_fwd<G, Cfg128x128>(x, wp, bias, y, s, act, slope, st, ld, c.splits, slab, stats);
        case T128x64: return run_fwd<G, Cfg128x64>(x, wp, bias, y, s, act, slope, st, ld, c.splits, slab, stats);
        case T128x32: return run_fwd<G, Cfg128x32>(x, wp, bias, y, s, act, slope, st, ld, c.splits, slab, stats);
        default: return run_fwd<G, Cfg64x64>(x, wp, bias, y, s, act, slope, st, ld, c.splits, slab, stats);
    }
}
#define GZ_INSTANTIATE(G)                                                                                                \
    template int launch_fwd_igemm<G>(const Choice&, const float*, const float*, const float*, float*, const ConvShape&, \
                                     int, float, float*, float*, hipStream_t);
GZ_INSTANTIATE(G4421)
GZ_INSTANTIATE(G5522)
GZ_INSTANTIATE(G3311)
GZ_INSTANTIATE(G1110)
#undef GZ_INSTANTIATE

// ---------------------------------------------------------------------------
// F with run-time geometry (evaluation path: InceptionV3).  Always tap-major, channels padded to a chunk.
// ---------------------------------------------------------------------------
template <class Cfg>
static int run_fwd_any(const float* x, const float* wp, const float* bias, float* y, const ConvShape& s,
                       const AnyGeom& g, int act, float slope, hipStream_t st, int splits, float* slab) {
    using AL = ConvFwdALoaderTapAny<Cfg::BM>;
    using BL = MContigLoader4<Cfg::BN>;
    typename AL::Params pa{x, s, make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW), g.KH, g.KW, g.SH, g.SW, g.PH, g.PW};
    int M = s.N * s.OH * s.OW;
    EpiNCHW::Params pe{y, M, s.K, s.OH * s.OW, make_fastdiv(s.OH * s.OW), bias, act, slope};
    int Kt = g.KH * g.KW * round_bk(s.C);
    typename BL::Params pb{wp, Kt, round4(s.K), round4(s.K), 0};
    return launch_igemm<Cfg, AL, BL, EpiNCHW>(pa, pb, pe, M, s.K, Kt, 1, splits, st, slab);
}

int launch_fwd_any_igemm(const SplitPlan& sp, const float* x, const float* wp, const float* bias, float* y,
                         const ConvShape& s, const AnyGeom& g, int act, float slope, float* slab, hipStream_t st) {
    switch (sp.tile) {
        case T128x128: return run_fwd_any<Cfg128x128>(x, wp, bias, y, s, g, act, slope, st, sp.splits, slab);
        case T128x64: return run_fwd_any<Cfg128x64>(x, wp, bias, y, s, g, act, slope, st, sp.splits, slab);
        case T128x32: return run_fwd_any<Cfg128x32>(x, wp, bias, y, s, g, act, slope, st, sp.splits, slab);
        default: return run_fwd_any<Cfg64x64>(x, wp, bias, y, s, g, act, slope, st, sp.splits, slab);
    }
}

}  // namespace gz
