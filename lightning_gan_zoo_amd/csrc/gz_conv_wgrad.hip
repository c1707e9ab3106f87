// Wg : dw = sum_pixels y (x) patch(x) -- the weight gradient of Conv2d and ConvTranspose2d.  The run_* launchers that
// instantiate the weight-gradient kernels of both implicit-GEMM skeletons (gz_igemm.h), launch_wgrad, which executes the
// Choice that choose_wgrad (gz_conv2d_choose.h) returned, and the C-ABI entry points that launch.  Nothing here decides:
// a condition that selects a kernel or a loader belongs in gz_conv2d_choose.h.  (Siblings: gz_conv_fwd.hip,
// gz_conv_dgrad.hip; the queries, the plan text and what the three ops are to each other: gz_conv.hip.)
#include <type_traits>

#include "gz_conv2d_choose.h"
#include "gz_reduce.h"
#include "../../include/gz_ops.h"

namespace gz {

// after a weight-gradient launch that wrote nz slabs: sum them into dw (gz_conv2d_wgrad_partial: report them instead)
static int wg_reduce(int rc, float* ws, float* dw, int nz, long long count, hipStream_t st) {
    if (rc != GZ_OK || nz <= 1 || defer_reduce(nz, count)) return rc;
    if (nz <= 8) launch_reduce_few_slabs(ws, dw, nz, count, st);
    else launch_reduce_slabs(ws, dw, nz, count, count, nullptr, 0ll, st);
    return launch_status();
}

template <class G, class Cfg, class AL, class BL>
static int launch_wgrad_igemm(const typename AL::Params& pa, const typename BL::Params& pb, float* dw, float* ws,
                        const ConvShape& s, int KTOT, int NTOT, const Choice& c, hipStream_t st) {
    const long long count = (long long)s.K * NTOT;
    EpiRowMajorB::Params pe{c.slabs > 1 ? ws : dw, s.K, NTOT, NTOT, count, nullptr, ACT_NONE, 0.f};
    const int rc = launch_igemm<Cfg, AL, BL, EpiRowMajorB>(pa, pb, pe, s.K, NTOT, KTOT, 1, c.splits, st);
    return wg_reduce(rc, ws, dw, c.slabs, count, st);
}

// Weight gradient on the igemm2 skeleton (register-staged transposing loaders, two LDS stages).  Tile 256 (output
// channels) x 128 ((c, ky, kx) columns); the reduction over the pixels is split so that >= 512 workgroups exist.
// (K in [128, 256): Cfg128x256 -- wgrad2_narrow)
using Cfg2Wg = TileCfg2<2, 2, 2, 2>;

template <class G, class Cfg>
static int run_wgrad2(const float* x, const float* y, float* dw, float* ws, const ConvShape& s, const Choice& c,
                      hipStream_t st) {
    using AL = WgALoaderRow<Cfg::BM>;
    using BL = WgBLoaderRow<Cfg::BN, G::kh, G::kw, G::s, G::p>;
    const int KTOT = s.N * s.OH * s.OW;
    const int NTOT = s.C * G::kh * G::kw;
    WgRowGeom rg;
    wg_row_geom<G>(s, &rg);
    typename AL::Params pa{y, s, rg, KTOT};
    typename BL::Params pb{x, s, rg, KTOT, NTOT};
    const long long count = (long long)s.K * NTOT;
    EpiRowMajorB::Params pe{c.slabs > 1 ? ws : dw, s.K, NTOT, NTOT, count, nullptr, ACT_NONE, 0.f};
    const int rc = launch_igemm2r<Cfg, AL, BL, EpiRowMajorB>(pa, pb, pe, s.K, NTOT, KTOT, c.splits, st);
    return wg_reduce(rc, ws, dw, c.slabs, count, st);
}

// ... and with both operands by LDS-DMA (igemm2w_kernel: k4 s2 p1 only, pixel rows of 4, 8 or a multiple of 16:
// wgrad2w_cw_shape)
template <class G, int BN, int CW>
struct wg2w_image {
    using type = std::conditional_t<G::kh == 4 && G::kw == 4, WgImgB2<BN, CW>, WgImgBG<BN, CW, G::kh, G::kw, G::s, G::p>>;
};

template <class G, class Cfg, int CW>
static int run_wgrad2w(const float* x, const float* y, float* dw, float* ws, const ConvShape& s, const Choice& c,
                       hipStream_t st) {
    using BL = typename wg2w_image<G, Cfg::BN, CW>::type;
    const int KTOT = s.N * s.OH * s.OW;
    const int NTOT = s.C * G::kh * G::kw;
    Wg2Params p{x, y, s, make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW)};
    const long long count = (long long)s.K * NTOT;
    EpiRowMajorB::Params pe{c.slabs > 1 ? ws : dw, s.K, NTOT, NTOT, count, nullptr, ACT_NONE, 0.f};
    const int rc = launch_igemm2w<Cfg, BL, EpiRowMajorB>(p, pe, s.K, NTOT, KTOT, c.splits, st);
    return wg_reduce(rc, ws, dw, c.slabs, count, st);
}

template <class G, class Cfg>
static int run_wgrad2w_cw(const float* x, const float* y, float* dw, float* ws, const ConvShape& s, const Choice& c,
                          hipStream_t st) {
    if constexpr (wgrad2w_geom<G>()) {
        switch (c.cw) {
            case 4: return run_wgrad2w<G, Cfg, 4>(x, y, dw, ws, s, c, st);
            case 8: return run_wgrad2w<G, Cfg, 8>(x, y, dw, ws, s, c, st);
            default: return run_wgrad2w<G, Cfg, 16>(x, y, dw, ws, s, c, st);
        }
    }
    return GZ_ERR_UNSUPPORTED;
}

template <class G, class Cfg>
static int run_wgrad(const float* x, const float* y, float* dw, float* ws, const ConvShape& s, const Choice& c,
                     hipStream_t st) {
    const int KTOT = s.N * s.OH * s.OW;
    const int NTOT = s.C * G::kh * G::kw;
    if (c.loader == LWgRow) {
        WgRowGeom rg;
        wg_row_geom<G>(s, &rg);
        using AL = WgALoaderRow<Cfg::BM>;
        using BL = WgBLoaderRow<Cfg::BN, G::kh, G::kw, G::s, G::p>;
        typename AL::Params pa{y, s, rg, KTOT};
        typename BL::Params pb{x, s, rg, KTOT, NTOT};
        return launch_wgrad_igemm<G, Cfg, AL, BL>(pa, pb, dw, ws, s, KTOT, NTOT, c, st);
    }
    using AL = WgALoader<Cfg::BM>;
    using BL = WgBLoader<Cfg::BN, G::kh, G::kw, G::s, G::p>;
    typename AL::Params pa{y, s, make_fastdiv(s.OH * s.OW), KTOT};
    typename BL::Params pb{x, s, make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW), KTOT, NTOT};
    return launch_wgrad_igemm<G, Cfg, AL, BL>(pa, pb, dw, ws, s, KTOT, NTOT, c, st);
}

// the one function that executes a weight-gradient Choice
template <class G>
static int launch_wgrad(const Choice& c, const float* x, const float* y, float* dw, float* dbias, float* ws,
                        size_t ws_bytes, const ConvShape& s, hipStream_t st) {
    if (c.kind == KDirect && c.loader != LFewc) return run_wgrad_smallch(x, y, dw, dbias, ws, ws_bytes, s, c.loader, st);
    if (dbias) return GZ_ERR_UNSUPPORTED;       // ask gz_conv2d_wgrad_fuses_bias first
    if (c.kind == KDirect) return run_wgrad_k4s2p1_fewc(x, y, nullptr, ACT_NONE, 0.f, dw, ws, ws_bytes, s, st);
    if (c.kind == KIgemm2w)
        return wgrad2_narrow(s) ? run_wgrad2w_cw<G, Cfg128x256>(x, y, dw, ws, s, c, st)
                                : run_wgrad2w_cw<G, Cfg2Wg>(x, y, dw, ws, s, c, st);
    if constexpr (G::kh == 4 && G::kw == 4)       // unaligned tensors: the register-staged loaders
        if (c.kind == KIgemm2r)
            return wgrad2_narrow(s) ? run_wgrad2<G, Cfg128x256>(x, y, dw, ws, s, c, st)
                                    : run_wgrad2<G, Cfg2Wg>(x, y, dw, ws, s, c, st);
    switch (c.tile) {
        case T128x128: return run_wgrad<G, Cfg128x128>(x, y, dw, ws, s, c, st);
        case T128x64: return run_wgrad<G, Cfg128x64>(x, y, dw, ws, s, c, st);
        case T128x32: return run_wgrad<G, Cfg128x32>(x, y, dw, ws, s, c, st);
        default: return run_wgrad<G, Cfg64x64>(x, y, dw, ws, s, c, st);
    }
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_conv2d_wgrad_fuses_bias(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P) {
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P)) return 0;
#define CALL(G) choose_wgrad<G>(s, kIdeal)
    const Choice c = [&]() -> Choice { GZ_GEOM_DISPATCH_OR(CALL, choice_of(KUnsupported, LGeneric, T64x64)) }();
#undef CALL
    return c.kind == KDirect && c.loader != LFewc;
}

int gz_conv2d_wgrad(const float* x, const float* y, float* dw, float* dbias, float* workspace, size_t ws_bytes, int N,
                    int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, hipStream_t stream) {
    gz::clear_stale_error();
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P)) return GZ_ERR_BAD_SHAPE;
    if (too_large((long long)N * C * H * W) || too_large((long long)N * K * OH * OW)) return GZ_ERR_TOO_LARGE;
    const Facts f = facts_of((const void*)((uintptr_t)x | (uintptr_t)y), dw, workspace, ws_bytes, false, false);
#define CALL(G) launch_wgrad<G>(choose_wgrad<G>(s, f), x, y, dw, dbias, workspace, ws_bytes, s, stream)
    GZ_GEOM_DISPATCH(CALL)
#undef CALL
}

int gz_conv2d_wgrad_partial(const float* x, const float* y, float* dw, float* workspace, size_t ws_bytes, int N, int C,
                            int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, int* nz_out,
                            long long* stride_out, hipStream_t stream) {
    gz::clear_stale_error();
    if (!nz_out || !stride_out) return GZ_ERR_BAD_SHAPE;
    ConvShape s{N, C, H, W, K, OH, OW};
    if (!shape_ok(s, KH, KW, S, P)) return GZ_ERR_BAD_SHAPE;
    if (too_large((long long)N * C * H * W) || too_large((long long)N * K * OH * OW)) return GZ_ERR_TOO_LARGE;
    *nz_out = 1;
    *stride_out = (long long)K * C * KH * KW;
    const Facts f = facts_of((const void*)((uintptr_t)x | (uintptr_t)y), dw, workspace, ws_bytes, false, false);
    WgDefer d{1, *stride_out};       // (the 3x3 direct kernels reduce their own slabs and leave it alone)
    tl_wg_defer = &d;
#define CALL(G) launch_wgrad<G>(choose_wgrad<G>(s, f), x, y, dw, nullptr, workspace, ws_bytes, s, stream)
    const int rc = [&]() -> int { GZ_GEOM_DISPATCH(CALL) }();
#undef CALL
    tl_wg_defer = nullptr;
    *nz_out = d.nz;
    *stride_out = d.stride;
    return rc;
}

}  // extern "C"
