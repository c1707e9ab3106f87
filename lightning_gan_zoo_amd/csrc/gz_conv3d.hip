// C-ABI entry points for the cubic-kernel 3-D convolution family on the fp32 MFMA implicit-GEMM core:
// HoloGAN's ConvTranspose3d(k3, s2, p1, output_padding 1) forward (= Dg), its input gradient (= F)
// and weight gradient (= Wg).  Reference call sites: core/models/hologan_generator.py:29-30,55-58.
//
// As for conv2d (gz_conv2d_choose.h), one function per op -- choose_fwd3 / choose_dgrad3 / choose_wgrad3 -- decides skeleton, loader,
// tile and splits once (gz_conv_choice.h): launch_*3 switch on the answer, gz_conv3d_*_workspace_bytes size its slabs,
// gz_conv3d_plan prints it.
#include <cstdio>
#include <type_traits>

#include "gz_conv_choice.h"
#include "gz_igemm.h"
#include "../../include/gz_ops.h"

namespace gz {

static inline int r4(int v) { return (v + 3) & ~3; }

// ---- weight images -------------------------------------------------------------------------------------------------
// wp[col][ld] = w[r][col] (r < R rows of length COLS), zero padded to ld
__global__ __launch_bounds__(256) void transpose_pad3_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                             int R, int COLS, int ld) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int r = r0 + ty + 8 * i, c = c0 + tx;
        tile[ty + 8 * i][tx] = (r < R && c < COLS) ? src[(long long)r * COLS + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = c0 + ty + 8 * i, r = r0 + tx;
        if (c < COLS && r < ld) dst[(long long)c * ld + r] = tile[tx][ty + 8 * i];
    }
}

// forward weights in tap-major order (Conv3DFwdALoaderTap): wp[(tap, c)][ld] = w[ko][c][tap], c padded to BK
static bool fwd3_tap_major(int C) {
    const bool off = knobs().no_tapmajor;
    return !off && C >= BK;
}

__global__ __launch_bounds__(256) void pack_fwd3_tap_kernel(const float* __restrict__ w, float* __restrict__ wp, int K,
                                                            int C, int taps, int cpad, int ld) {
    const long long total = (long long)taps * cpad * ld;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        int ko = (int)(i % ld);
        long long row = i / ld;
        int c = (int)(row % cpad), tap = (int)(row / cpad);
        wp[i] = (ko < K && c < C) ? w[((long long)ko * C + c) * taps + tap] : 0.f;
    }
}

// wp[phase][(ko, td, ty, tx)][ldc] = w[ko][c][kd][ky][kx], k* = ((p* + P) % S) + S * t*.  Only the taps with
// k* < KS exist (k3 s2 p1: 1 tap on an even output coordinate, 2 on an odd one -> 1..8 per phase, 27 over the 8
// phases instead of 8 x 8); a phase's rows are packed tightly, the rest of its fixed-size region is zero.
__global__ __launch_bounds__(256) void pack_dgrad3_kernel(const float* __restrict__ w, float* __restrict__ wp, int K,
                                                          int C, int KS, int S, int P, int T, int ldc) {
    const int ko = blockIdx.x, phase = blockIdx.y;
    const int pd = phase / (S * S), py = (phase / S) % S, px = phase % S;
    const int rd = (pd + P) % S, ry = (py + P) % S, rx = (px + P) % S;
    const int nd = dg_taps(KS, S, P, pd), ny = dg_taps(KS, S, P, py), nx = dg_taps(KS, S, P, px);
    const int taps = nd * ny * nx, pad = T * T * T - taps;
    float* dst = wp + (long long)phase * K * T * T * T * ldc;
    for (int i = threadIdx.x; i < taps * ldc; i += blockDim.x) {
        int tap = i / ldc, c = i - tap * ldc;
        int kd = rd + S * (tap / (ny * nx)), ky = ry + S * ((tap / nx) % ny), kx = rx + S * (tap % nx);
        dst[((long long)ko * taps + tap) * ldc + c] =
            c < C ? w[((((long long)ko * C + c) * KS + kd) * KS + ky) * KS + kx] : 0.f;
    }
    for (int i = threadIdx.x; i < pad * ldc; i += blockDim.x)
        dst[((long long)K * taps + (long long)ko * pad) * ldc + i] = 0.f;
}

// Whether the transposed form runs on the igemm2 skeleton with its weight rows tap-major per phase.  THE predicate: the
// pack size (gz_conv3d_pack_dgrad_elems), the pack kernel (gz_conv3d_pack_dgrad) and the launch (choose_dgrad3) all ask
// it and nothing else, so the image that was packed is the image that is read.
// Multiples of 128 columns only: with 64 (HoloGAN's block2, 8-64 chunks per workgroup) the 256x64 tile measured 164 us
// against 147 us on the round-1 kernel, and a 512x64 tile needs more gather pieces per k-step than the stream holds.
static bool dg3_tap2(int K, int C) {
    return !knobs().no_igemm2 && !knobs().no_igemm2_tap && K >= BK && (C & 127) == 0;
}

// wp[phase][(tap, ko)][ldc] = w[ko][c][kd][ky][kx] over the phase's own nd x ny x nx taps (tap = (td * ny + ty) * nx +
// tx, k* = ((p* + P) % S) + S * t*), ko padded to a multiple of BK with zero rows; the unused tail of a phase's
// fixed-size T^3 * kpad-row region is never read
__global__ __launch_bounds__(256) void pack_dgrad3_tap_kernel(const float* __restrict__ w, float* __restrict__ wp, int K,
                                                              int C, int KS, int S, int P, int T, int kpad, int ldc) {
    const int phase = blockIdx.y;
    const int pd = phase / (S * S), py = (phase / S) % S, px = phase % S;
    const int rd = (pd + P) % S, ry = (py + P) % S, rx = (px + P) % S;
    const int nd = dg_taps(KS, S, P, pd), ny = dg_taps(KS, S, P, py), nx = dg_taps(KS, S, P, px);
    float* dst = wp + (long long)phase * T * T * T * kpad * ldc;
    const long long total = (long long)nd * ny * nx * kpad * ldc;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % ldc);
        const long long row = i / ldc;
        const int ko = (int)(row % kpad), tap = (int)(row / kpad);
        const int kd = rd + S * (tap / (ny * nx)), ky = ry + S * ((tap / nx) % ny), kx = rx + S * (tap % nx);
        dst[i] = (ko < K && c < C) ? w[((((long long)ko * C + c) * KS + kd) * KS + ky) * KS + kx] : 0.f;
    }
}

__global__ __launch_bounds__(256) void reduce_slabs3_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                            int S, long long count) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += slab[(long long)s * count + i];
    out[i] = acc;
}

__global__ __launch_bounds__(256) void act_inplace3_kernel(float* __restrict__ x, long long total4, int act, float slope) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += stride) {
        f32x4 v = reinterpret_cast<f32x4*>(x)[i];
        v[0] = act_fwd(v[0], act, slope); v[1] = act_fwd(v[1], act, slope);
        v[2] = act_fwd(v[2], act, slope); v[3] = act_fwd(v[3], act, slope);
        reinterpret_cast<f32x4*>(x)[i] = v;
    }
}

static bool shape3_ok(const Conv3DShape& s, int KS, int S, int P) {
    if (s.N <= 0 || s.C <= 0 || s.K <= 0 || s.D <= 0 || s.H <= 0 || s.W <= 0) return false;
    auto o = [&](int v) { return (v + 2 * P - KS) / S + 1; };
    return s.OD == o(s.D) && s.OH == o(s.H) && s.OW == o(s.W);
}

static bool big3(long long e) { return e * 4 >= (1ll << 31); }

// ---- the launches --------------------------------------------------------------------------------------------------
// Reduction chunks per phase of the transposed form (1, 2, 2, 2, 4, 4, 4, 8 taps for k3 s2 p1), counted here and nowhere
// else: choose_dgrad3 sizes splits and slabs from them, run_dgrad3 / run_dgradtap3 hand them to the launcher.
struct Phases3 {
    int n, pc[8], maxpc;
    long long total;
    // slabs when the longest phase is cut into `splits` pieces: a phase gets as many as its own reduction needs
    // (GridMap::phase_nz), not the longest phase's count
    int slabs(int splits) const {
        const int per = (maxpc + splits - 1) / splits;
        int sum = 0;
        for (int ph = 0; ph < n; ++ph) sum += (pc[ph] + per - 1) / per;
        return sum;
    }
};

static Phases3 dg3_phases(int K, int KS, int S, int P, bool tap2) {      // tap2: whole BK-blocks of K per tap (dg3_tap2)
    Phases3 p{S * S * S, {}, 0, 0};
    for (int ph = 0; ph < p.n; ++ph) {
        const int taps = dg_taps(KS, S, P, ph / (S * S)) * dg_taps(KS, S, P, (ph / S) % S) * dg_taps(KS, S, P, ph % S);
        p.pc[ph] = tap2 ? taps * (round_bk(K) / BK) : (K * taps + BK - 1) / BK;
        p.total += p.pc[ph];
        p.maxpc = p.pc[ph] > p.maxpc ? p.pc[ph] : p.maxpc;
    }
    return p;
}

template <class Cfg, int KS, int S, int P>
static int run_fwd3(const float* x, const float* wp, const float* bias, float* y, const Conv3DShape& s, int act,
                    float slope, hipStream_t st, Loader ld, int splits, float* slab) {
    using AL = Conv3DFwdALoader<Cfg::BM, KS, S, P>;
    using BL = MContigLoader4<Cfg::BN>;
    const int osp = s.OD * s.OH * s.OW;
    typename AL::Params pa{x, s, make_fastdiv(osp), make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW)};
    int M = s.N * osp;
    EpiNCHW::Params pe{y, M, s.K, osp, make_fastdiv(osp), bias, act, slope};
    if (ld == LTap) {
        using ALT = Conv3DFwdALoaderTap<Cfg::BM, KS, S, P>;
        int Kt = KS * KS * KS * round_bk(s.C);
        typename BL::Params pbt{wp, Kt, r4(s.K), r4(s.K), 0};
        return launch_igemm<Cfg, ALT, BL, EpiNCHW>(pa, pbt, pe, M, s.K, Kt, 1, splits, st, slab);
    }
    int Kg = s.C * KS * KS * KS;
    typename BL::Params pb{wp, Kg, r4(s.K), r4(s.K), 0};
    return launch_igemm<Cfg, AL, BL, EpiNCHW>(pa, pb, pe, M, s.K, Kg, 1, splits, st, slab);
}

template <class Cfg, int KS, int S, int P>
static int run_dgrad3(const float* y, const float* wp, const float* bias, float* x, const Conv3DShape& s, int act,
                      float slope, hipStream_t st, int splits, float* slab) {
    using AL = Conv3DDgALoader<Cfg::BM, KS, S, P>;
    using BL = MContigLoader4<Cfg::BN>;
    using Epi = EpiPhase3D<S>;
    const int AD = s.D / S, AH = s.H / S, AW = s.W / S;
    typename AL::Params pa{y, s, AD, AH, AW, make_fastdiv(AD * AH * AW), make_fastdiv(AH * AW), make_fastdiv(AW)};
    int Kg = s.K * AL::TAPS;
    int ldc = r4(s.C);
    typename BL::Params pb{wp, Kg, ldc, ldc, (long long)Kg * ldc};
    int M = s.N * AD * AH * AW;
    typename Epi::Params pe{x, M, s.C, s.D, s.H, s.W, AD, AH, AW, make_fastdiv(AD * AH * AW), make_fastdiv(AH * AW),
                            make_fastdiv(AW), bias, act, slope};
    const Phases3 ph = dg3_phases(s.K, KS, S, P, false);
    return launch_igemm<Cfg, AL, BL, Epi>(pa, pb, pe, M, s.C, Kg, S * S * S, splits, st, slab, ph.pc);
}

// Weight gradient on either skeleton (KD = KIgemm: igemm_kernel; KIgemm2r: igemm2r_kernel with the same register-staged
// loaders): a split launch writes c.slabs slabs of K x C*KS^3 floats to the workspace, reduce_slabs3_kernel sums them
// in slab order.
template <class Cfg, Kind KD, int KS, int S, int P>
static int run_wgrad3(const float* x, const float* y, float* dw, float* ws, const Conv3DShape& s, const Choice& c,
                      hipStream_t st) {
    using AL = WgALoader<Cfg::BM>;
    using BL = Wg3DBLoader<Cfg::BN, KS, S, P>;
    using Epi = std::conditional_t<KD == KIgemm2r, EpiRowMajorB, EpiRowMajor>;
    const int osp = s.OD * s.OH * s.OW;
    const int KTOT = s.N * osp;
    const int NTOT = s.C * KS * KS * KS;
    ConvShape flat{s.N, s.C, 1, 1, s.K, osp, 1};      // WgALoader only needs N, K and OH*OW
    typename AL::Params pa{y, flat, make_fastdiv(osp), KTOT};
    typename BL::Params pb{x, s, make_fastdiv(osp), make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW), KTOT, NTOT};
    const long long count = (long long)s.K * NTOT;
    typename Epi::Params pe{c.slabs > 1 ? ws : dw, s.K, NTOT, NTOT, count, nullptr, ACT_NONE, 0.f};
    int rc;
    if constexpr (KD == KIgemm2r) rc = launch_igemm2r<Cfg, AL, BL, Epi>(pa, pb, pe, s.K, NTOT, KTOT, c.splits, st);
    else rc = launch_igemm<Cfg, AL, BL, Epi>(pa, pb, pe, s.K, NTOT, KTOT, 1, c.splits, st);
    if (rc != GZ_OK || c.slabs <= 1) return rc;
    hipLaunchKernelGGL(reduce_slabs3_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, ws, dw, c.slabs,
                       count);
    return launch_status();
}

// ---- the igemm2 skeleton for the two gather-fed directions (round 4) -----------------------------------------
// The round-1 kernels above run HoloGAN's two ConvTranspose3d layers at 89-100 TFLOP/s forward and 95-104 on the input
// gradient; the one-wavefront-per-SIMD skeleton with 4-byte LDS-DMA gathers (Conv3DDgTapA2 / Conv3DTapA2) takes them
// when the GEMM's column count is a multiple of 64 (256x128 or 256x64 tiles).
template <class Cfg, int KS, int S, int P>
static int run_dgradtap3(const float* y, const float* wp, const float* bias, float* x, const Conv3DShape& s, int act,
                         float slope, hipStream_t st, int splits, float* slab) {
    using AL = Conv3DDgTapA2<Cfg::BM, KS, S, P>;
    using BL = MContigB2<Cfg::BN>;
    using Epi = EpiPhase3DB<S>;
    const int AD = s.D / S, AH = s.H / S, AW = s.W / S;
    typename AL::Params pa{y, s, AD, AH, AW, make_fastdiv(AD * AH * AW), make_fastdiv(AH * AW), make_fastdiv(AW)};
    const int kpad = round_bk(s.K), Kt = AL::Geo::T * AL::Geo::T * AL::Geo::T * kpad, ldc = r4(s.C);
    typename BL::Params pb{wp, Kt, ldc, ldc, (long long)Kt * ldc};
    const int M = s.N * AD * AH * AW;
    typename Epi::Params pe{x, M, s.C, s.D, s.H, s.W, AD, AH, AW, make_fastdiv(AD * AH * AW), make_fastdiv(AH * AW),
                            make_fastdiv(AW), bias, act, slope};
    const Phases3 ph = dg3_phases(s.K, KS, S, P, true);
    const int rc = launch_igemm2<Cfg, AL, BL, Epi>(pa, pb, pe, M, s.C, Kt, S * S * S, splits, st, slab, ph.pc);
    if (rc != GZ_OK || act == ACT_NONE) return rc;
    // (EpiPhase3DB adds the bias only; no shipped model puts an activation on a ConvTranspose3d)
    const long long total4 = (long long)s.N * s.C * s.D * s.H * s.W / 4;       // D, H, W even: a multiple of 8 elements
    hipLaunchKernelGGL(act_inplace3_kernel, dim3((unsigned)((total4 + 255) / 256 > 4096 ? 4096 : (total4 + 255) / 256)),
                       dim3(256), 0, st, x, total4, act, slope);
    return launch_status();
}

template <class Cfg, int KS, int S, int P>
static int run_fwdtap3(const float* x, const float* wp, const float* bias, float* y, const Conv3DShape& s, int act,
                       float slope, hipStream_t st, int splits, float* slab) {
    using AL = Conv3DTapA2<Cfg::BM, KS, S, P>;
    using BL = MContigB2<Cfg::BN>;
    const int osp = s.OD * s.OH * s.OW;
    typename AL::Params pa{x, s, make_fastdiv(osp), make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW)};
    const int M = s.N * osp, Kt = KS * KS * KS * round_bk(s.C);
    EpiNCHWB::Params pe{y, M, s.K, osp, make_fastdiv(osp), bias, act, slope};
    typename BL::Params pb{wp, Kt, r4(s.K), r4(s.K), 0};
    return launch_igemm2<Cfg, AL, BL, EpiNCHWB>(pa, pb, pe, M, s.K, Kt, 1, splits, st, slab);
}

// ---- the launch choice of each op, and the one function that executes it -------------------------------------------
// The choosers read C and the feature side of the shape only (N, K, OD, OH, OW): all that a workspace query knows.
static long long tiles3(TileId t, long long M, long long N, int ny) {
    const int bm = t == T64x64 ? 64 : 128, bn = t == T128x128 ? 128 : (t == T128x32 ? 32 : 64);
    return ((M + bm - 1) / bm) * ((N + bn - 1) / bn) * ny;
}

static TileId pick3(long long M, long long N, int ny) {
    if (N <= 32) return T128x32;
    if (N <= 64) return tiles3(T128x64, M, N, ny) >= cus() ? T128x64 : T64x64;
    if (tiles3(T128x128, M, N, ny) >= cus()) return T128x128;
    if (tiles3(T128x64, M, N, ny) >= cus()) return T128x64;
    return T64x64;
}

// split-K of under-filled F / Dg launches: same policy as conv2d (plan_split, gz_conv2d_choose.h)
static int plan3(TileId tile, long long M, long long N, int Kdim, int ny) {
    const long long tiles = tiles3(tile, M, N, ny);
    const int chunks = (Kdim + BK - 1) / BK;
    if (knobs().no_splitk || chunks < 16 || tiles >= 2 * cus()) return 1;
    long long want = (4 * cus() + tiles - 1) / tiles, cap = chunks / 8;
    long long sp = want < cap ? want : cap;
    return sp < 2 ? 1 : (int)sp;
}

static size_t slab_bytes(const Choice& c, long long M, long long N) {
    return c.splits > 1 ? (size_t)c.slabs * M * N * 4 : 0;
}

// F on igemm2: the tap-major forward image is the one already packed.  KUnsupported: the launch stays on igemm_kernel.
static Choice fwd3_igemm2(long long M, int K, int C, int KS) {
    const Choice none = choice_of(KUnsupported, LGeneric, T64x64);
    if (knobs().no_igemm2 || knobs().no_igemm2_tap || !fwd3_tap_major(C) || (K & 63)) return none;
    const int chunks = KS * KS * KS * round_bk(C) / BK;
    const long long tm = (M + 255) / 256, t64 = tm * (K / 64), t128 = (K & 127) ? 0 : tm * (K / 128);
    const int cu = cus();
    Choice c = choice_of(KIgemm2, LGather2, t128 >= cu * 7 / 8 ? T256x128 : T256x64);
    if (t128 >= cu * 7 / 8 || t64 >= cu * 7 / 8) return c;
    if (knobs().no_splitk) return none;
    for (int tile = t128 ? 1 : 2; tile <= 2; ++tile) {
        const long long tiles = tile == 1 ? t128 : t64;
        c.tile = tile == 1 ? T256x128 : T256x64;
        c.splits = (int)((cu + tiles - 1) / tiles);
        while (c.splits > 1 && chunks / c.splits < 48) --c.splits;
        if (c.splits > 1 && tiles * c.splits >= cu * 3 / 4) return c;
    }
    return none;
}

// Short workspace: an igemm2 launch is refused (GZ_ERR_WORKSPACE, launch_fwd3), an igemm launch runs unsplit.
static Choice choose_fwd3(const Conv3DShape& s, int KS, const Facts& f) {
    const long long M = (long long)s.N * s.OD * s.OH * s.OW;
    const bool tap = fwd3_tap_major(s.C);
    const int kdim = (tap ? round_bk(s.C) : s.C) * KS * KS * KS;
    Choice c = fwd3_igemm2(M, s.K, s.C, KS);
    if (c.kind != KIgemm2 || !f.in4) {
        c = choice_of(KIgemm, tap ? LTap : LGeneric, pick3(M, s.K, 1));
        c.splits = plan3(c.tile, M, s.K, kdim, 1);
    }
    c.slabs = split_nz(kdim, c.splits);
    c.ws_short = c.splits > 1 && ws_lacks(f, slab_bytes(c, M, s.K));
    if (c.ws_short && c.kind == KIgemm) c.splits = c.slabs = 1;
    return c;
}

template <int KS, int S, int P>
static int launch_fwd3(const Choice& c, const float* x, const float* wp, const float* bias, float* y,
                       const Conv3DShape& s, int act, float slope, float* ws, hipStream_t st) {
    if (c.kind == KIgemm2 && c.ws_short) return GZ_ERR_WORKSPACE;
    float* slab = c.splits > 1 ? ws : nullptr;
    switch (c.tile) {
        case T256x128: return run_fwdtap3<Cfg256x128, KS, S, P>(x, wp, bias, y, s, act, slope, st, c.splits, slab);
        case T256x64: return run_fwdtap3<Cfg256x64, KS, S, P>(x, wp, bias, y, s, act, slope, st, c.splits, slab);
        case T128x128: return run_fwd3<Cfg128x128, KS, S, P>(x, wp, bias, y, s, act, slope, st, c.loader, c.splits, slab);
        case T128x64: return run_fwd3<Cfg128x64, KS, S, P>(x, wp, bias, y, s, act, slope, st, c.loader, c.splits, slab);
        case T128x32: return run_fwd3<Cfg128x32, KS, S, P>(x, wp, bias, y, s, act, slope, st, c.loader, c.splits, slab);
        default: return run_fwd3<Cfg64x64, KS, S, P>(x, wp, bias, y, s, act, slope, st, c.loader, c.splits, slab);
    }
}

// Split-K of the transposed convolution's 8 phases: the chunk count per workgroup is chosen from the TOTAL work so that
// workgroups of equal length come out (~1024 on igemm; ~2 per CU of >= 32 chunks on igemm2); c.splits cuts the longest
// phase, c.slabs sums Phases3::slabs.  Short workspace: as for F (the packed image is tap-major or not -- dg3_tap2 --
// so an igemm2 launch has no other kernel to fall back to).
static Choice choose_dgrad3(const Conv3DShape& s, int KS, int S, int P, const Facts& f) {
    const long long Mp = (long long)s.N * s.OD * s.OH * s.OW;      // rows per phase: D = S * OD
    const int ny = S * S * S;
    const bool tap2 = dg3_tap2(s.K, s.C);
    const Phases3 ph = dg3_phases(s.K, KS, S, P, tap2);
    Choice c = choice_of(tap2 ? KIgemm2 : KIgemm, tap2 ? LGather2 : LGeneric, T64x64);
    if (tap2) {
        // 256x128 also when its tiles alone do not fill the chip (HoloGAN block1 at bs 64, 128 tiles, 27 slabs: 184 us
        // against 193 us on 256x64 tiles with 21 slabs; the round-1 kernel: 223 us)
        c.tile = knobs().dg3_tile == 2 ? T256x64 : T256x128;
        const long long tp = ((Mp + 255) / 256) * (c.tile == T256x128 ? s.C / 128 : s.C / 64);
        // phases of 1..8 taps: with >= 4 workgroups per CU the longest-first launch order balances them; below that the
        // reduction is cut into pieces of equal length (>= 32 chunks), ~2 workgroups per CU
        if (!knobs().no_splitk && tp * ny < 4LL * cus()) {
            const int wgs = knobs().dg3_wgs * cus();
            long long cps = (ph.total * tp + wgs - 1) / wgs;
            if (cps < knobs().dg3_min_chunks) cps = knobs().dg3_min_chunks;
            c.splits = (int)((ph.maxpc + cps - 1) / cps);
        }
    } else {
        c.tile = pick3(Mp, s.C, ny);
        const long long tp = tiles3(c.tile, Mp, s.C, 1);
        if (!knobs().no_splitk && ph.maxpc >= 16 && tp * ny < 2 * cus()) {
            long long cps = (ph.total * tp + 4 * cus() - 1) / (4 * cus());
            if (cps < 8) cps = 8;
            // (GZ_DG3_EVEN_SPLIT: the round-1 plan, sized as if every phase had 8 taps)
            c.splits = knobs().dg3_even_split ? plan3(c.tile, Mp, s.C, s.K * 8, 8) : (int)((ph.maxpc + cps - 1) / cps);
        }
    }
    if (c.splits < 2) c.splits = 1;
    else c.slabs = ph.slabs(c.splits);
    c.ws_short = c.splits > 1 && ws_lacks(f, slab_bytes(c, Mp, s.C));
    if (c.ws_short && c.kind == KIgemm) c.splits = c.slabs = 1;
    return c;
}

template <int KS, int S, int P>
static int launch_dgrad3(const Choice& c, const float* y, const float* wp, const float* bias, float* x,
                         const Conv3DShape& s, int act, float slope, float* ws, hipStream_t st) {
    if (c.kind == KIgemm2 && c.ws_short) return GZ_ERR_WORKSPACE;
    float* slab = c.splits > 1 ? ws : nullptr;
    switch (c.tile) {
        case T256x128: return run_dgradtap3<Cfg256x128, KS, S, P>(y, wp, bias, x, s, act, slope, st, c.splits, slab);
        case T256x64: return run_dgradtap3<Cfg256x64, KS, S, P>(y, wp, bias, x, s, act, slope, st, c.splits, slab);
        case T128x128: return run_dgrad3<Cfg128x128, KS, S, P>(y, wp, bias, x, s, act, slope, st, c.splits, slab);
        case T128x64: return run_dgrad3<Cfg128x64, KS, S, P>(y, wp, bias, x, s, act, slope, st, c.splits, slab);
        case T128x32: return run_dgrad3<Cfg128x32, KS, S, P>(y, wp, bias, x, s, act, slope, st, c.splits, slab);
        default: return run_dgrad3<Cfg64x64, KS, S, P>(y, wp, bias, x, s, act, slope, st, c.splits, slab);
    }
}

// Weight gradient.  K >= 128: the igemm2 skeleton (256 x 128 tiles, or 128 x 256 with fewer than 256 output channels),
// split so that two workgroups per CU come out, >= 24 chunks each: HoloGAN block1 (54 tiles x 9 splits) 238 -> 178 us,
// block2 (7 tiles x 73) 210 -> 205 us; pieces of 48-64 chunks leave a partial second round of workgroups and measured
// 240-310 us.  Short workspace: the splits are clamped to the slabs it holds (wg_fit_splits), unsplit below 2.
static Choice choose_wgrad3(const Conv3DShape& s, int KS, const Facts& f) {
    const long long NTOT = (long long)s.C * KS * KS * KS;
    const int KTOT = s.N * s.OD * s.OH * s.OW, chunks = (KTOT + BK - 1) / BK;
    Choice c = choice_of(KIgemm, LGeneric, T64x64);
    if (!knobs().no_igemm2 && !knobs().no_wg3r && s.K >= 128) {
        c.kind = KIgemm2r;
        c.tile = s.K >= 256 ? T256x128 : T128x256;
        const long long tiles = s.K >= 256 ? (long long)((s.K + 255) / 256) * ((NTOT + 127) / 128)
                                           : (long long)((s.K + 127) / 128) * ((NTOT + 255) / 256);
        c.splits = (int)(knobs().wg3r_wgs * cus() / tiles);
        if (c.splits < 1) c.splits = 1;
        while (c.splits > 1 && chunks / c.splits < knobs().wg3r_min_chunks) --c.splits;
    } else {
        c.tile = NTOT <= 32 ? T128x32 : ((NTOT <= 64 || s.K <= 64) ? (s.K <= 64 ? T64x64 : T128x64) : T128x128);
        const int force = knobs().wg3_tile;      // experiment
        if (force >= 0 && c.tile == T128x128) c.tile = force <= T64x64 ? (TileId)force : T64x64;
        const long long tiles = tiles3(c.tile, s.K, NTOT, 1);
        const long long want = (knobs().wg3_target * cus() / 256 + tiles - 1) / tiles, cap = chunks / 8;
        c.splits = tiles >= cus() ? 1 : (int)(want < cap ? want : cap);
        if (c.splits < 1) c.splits = 1;
    }
    const int wish = c.splits;
    c.splits = wg_fit_splits(wish, f.ws_bytes, s.K * NTOT);
    c.ws_short = c.splits < wish;
    c.slabs = split_nz(KTOT, c.splits);
    return c;
}

template <int KS, int S, int P>
static int launch_wgrad3(const Choice& c, const float* x, const float* y, float* dw, float* ws, const Conv3DShape& s,
                         hipStream_t st) {
    switch (c.tile) {
        case T256x128: return run_wgrad3<Cfg256x128, KIgemm2r, KS, S, P>(x, y, dw, ws, s, c, st);
        case T128x256: return run_wgrad3<Cfg128x256, KIgemm2r, KS, S, P>(x, y, dw, ws, s, c, st);
        case T128x128: return run_wgrad3<Cfg128x128, KIgemm, KS, S, P>(x, y, dw, ws, s, c, st);
        case T128x64: return run_wgrad3<Cfg128x64, KIgemm, KS, S, P>(x, y, dw, ws, s, c, st);
        case T128x32: return run_wgrad3<Cfg128x32, KIgemm, KS, S, P>(x, y, dw, ws, s, c, st);
        default: return run_wgrad3<Cfg64x64, KIgemm, KS, S, P>(x, y, dw, ws, s, c, st);
    }
}

// The workspace sizes are asked by the feature side alone; the one geometry that exists (k3 s2 p1 between even image
// sides) has D = 2 * OD, and no chooser reads the image side.
constexpr int kS3 = 2, kP3 = 1;
static Conv3DShape shape3_of_features(int N, int C, int K, int OD, int OH, int OW) {
    return Conv3DShape{N, C, kS3 * OD, kS3 * OH, kS3 * OW, K, OD, OH, OW};
}

// the A-operand loader a choice of op (0 F, 1 Dg, 2 Wg) runs with, as gz_conv3d_plan names it
static const char* loader_text3(int op, const Choice& c) {
    if (op == 2) return c.kind == KIgemm2r ? "WgALoader+Wg3DBLoader(register-staged)" : "WgALoader+Wg3DBLoader";
    switch (c.loader) {
        case LGather2: return op == 0 ? "Conv3DTapA2(gather, LDS-DMA 4B)" : "Conv3DDgTapA2(gather, LDS-DMA 4B)";
        case LTap: return "Conv3DFwdALoaderTap";
        default: return op == 0 ? "Conv3DFwdALoader" : "Conv3DDgALoader";
    }
}

}  // namespace gz

using namespace gz;

extern "C" {

long long gz_conv3d_pack_fwd_elems(int K, int C, int KS) {
    return (long long)(fwd3_tap_major(C) ? round_bk(C) : C) * KS * KS * KS * r4(K);
}

long long gz_conv3d_pack_dgrad_elems(int K, int C, int KS, int S) {
    int T = (KS + S - 1) / S;
    return (long long)S * S * S * (dg3_tap2(K, C) ? round_bk(K) : K) * T * T * T * r4(C);
}

int gz_conv3d_pack_fwd(const float* w, float* wp, int K, int C, int KS, hipStream_t stream) {
    gz::clear_stale_error();
    if (K <= 0 || C <= 0 || KS <= 0) return GZ_ERR_BAD_SHAPE;
    int Kg = C * KS * KS * KS, ld = r4(K);
    if (fwd3_tap_major(C)) {
        long long total = (long long)KS * KS * KS * round_bk(C) * ld;
        hipLaunchKernelGGL(pack_fwd3_tap_kernel, dim3((unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256)),
                           dim3(256), 0, stream, w, wp, K, C, KS * KS * KS, round_bk(C), ld);
        return launch_status();
    }
    hipLaunchKernelGGL(transpose_pad3_kernel, dim3((Kg + 31) / 32, (ld + 31) / 32), dim3(256), 0, stream, w, wp, K, Kg,
                       ld);
    return launch_status();
}

int gz_conv3d_pack_dgrad(const float* w, float* wp, int K, int C, int KS, int S, int P, hipStream_t stream) {
    gz::clear_stale_error();
    if (K <= 0 || C <= 0 || KS <= 0 || S <= 0) return GZ_ERR_BAD_SHAPE;
    int T = (KS + S - 1) / S;
    if (dg3_tap2(K, C)) {
        const long long total = (long long)T * T * T * round_bk(K) * r4(C);
        const unsigned bx = (unsigned)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
        hipLaunchKernelGGL(pack_dgrad3_tap_kernel, dim3(bx, S * S * S), dim3(256), 0, stream, w, wp, K, C, KS, S, P, T,
                           round_bk(K), r4(C));
        return launch_status();
    }
    hipLaunchKernelGGL(pack_dgrad3_kernel, dim3(K, S * S * S), dim3(256), 0, stream, w, wp, K, C, KS, S, P, T, r4(C));
    return launch_status();
}

size_t gz_conv3d_fwd_workspace_bytes(int N, int C, int K, int OD, int OH, int OW, int KS) {
    return slab_bytes(choose_fwd3(shape3_of_features(N, C, K, OD, OH, OW), KS, kIdeal), (long long)N * OD * OH * OW, K);
}

size_t gz_conv3d_dgrad_workspace_bytes(int N, int C, int K, int OD, int OH, int OW, int KS) {
    return slab_bytes(choose_dgrad3(shape3_of_features(N, C, K, OD, OH, OW), KS, kS3, kP3, kIdeal),
                      (long long)N * OD * OH * OW, C);
}

// (in asked splits, not slabs: wg_fit_splits clamps in that unit)
size_t gz_conv3d_wgrad_workspace_bytes(int N, int C, int K, int OD, int OH, int OW, int KS) {
    const Choice c = choose_wgrad3(shape3_of_features(N, C, K, OD, OH, OW), KS, kIdeal);
    return c.splits > 1 ? (size_t)c.splits * K * C * KS * KS * KS * 4 : 0;
}

int gz_conv3d_fwd(const float* x, const float* wpack, const float* bias, float* y, float* workspace, size_t ws_bytes,
                  int N, int C, int D, int H, int W, int K, int OD, int OH, int OW, int KS, int S, int P, int act,
                  float slope, hipStream_t stream) {
    gz::clear_stale_error();
    Conv3DShape s{N, C, D, H, W, K, OD, OH, OW};
    if (KS != 3 || S != 2 || P != 1) return GZ_ERR_UNSUPPORTED;
    if (!shape3_ok(s, KS, S, P)) return GZ_ERR_BAD_SHAPE;
    if (big3((long long)N * C * D * H * W) || big3((long long)N * K * OD * OH * OW)) return GZ_ERR_TOO_LARGE;
    if (((uintptr_t)wpack & 15) || ((uintptr_t)y & 15)) return GZ_ERR_BAD_SHAPE;
    const Facts f = facts_of(x, y, workspace, ws_bytes, bias || act != ACT_NONE, false);
    return launch_fwd3<3, 2, 1>(choose_fwd3(s, KS, f), x, wpack, bias, y, s, act, slope, workspace, stream);
}

int gz_conv3d_dgrad(const float* y, const float* wpack, const float* bias, float* x, float* workspace,
                    size_t ws_bytes, int N, int C, int D, int H, int W, int K, int OD, int OH, int OW, int KS, int S,
                    int P, int act, float slope, hipStream_t stream) {
    gz::clear_stale_error();
    Conv3DShape s{N, C, D, H, W, K, OD, OH, OW};
    if (KS != 3 || S != 2 || P != 1) return GZ_ERR_UNSUPPORTED;
    if (!shape3_ok(s, KS, S, P) || D % S || H % S || W % S) return GZ_ERR_BAD_SHAPE;
    if (big3((long long)N * C * D * H * W) || big3((long long)N * K * OD * OH * OW)) return GZ_ERR_TOO_LARGE;
    if ((uintptr_t)wpack & 15) return GZ_ERR_BAD_SHAPE;
    const Facts f = facts_of(y, x, workspace, ws_bytes, bias || act != ACT_NONE, false);
    return launch_dgrad3<3, 2, 1>(choose_dgrad3(s, KS, S, P, f), y, wpack, bias, x, s, act, slope, workspace, stream);
}

int gz_conv3d_wgrad(const float* x, const float* y, float* dw, float* workspace, size_t ws_bytes, int N, int C, int D,
                    int H, int W, int K, int OD, int OH, int OW, int KS, int S, int P, hipStream_t stream) {
    gz::clear_stale_error();
    Conv3DShape s{N, C, D, H, W, K, OD, OH, OW};
    if (KS != 3 || S != 2 || P != 1) return GZ_ERR_UNSUPPORTED;
    if (!shape3_ok(s, KS, S, P)) return GZ_ERR_BAD_SHAPE;
    if (big3((long long)N * C * D * H * W) || big3((long long)N * K * OD * OH * OW)) return GZ_ERR_TOO_LARGE;
    const Facts f = facts_of((const void*)((uintptr_t)x | (uintptr_t)y), dw, workspace, ws_bytes, false, false);
    return launch_wgrad3<3, 2, 1>(choose_wgrad3(s, KS, f), x, y, dw, workspace, s, stream);
}

/* Which kernel a launch of op (0 F, 1 Dg, 2 Wg) takes, as text: the choice for 16-byte aligned tensors and a workspace
 * of the advertised size.  Runs on the CPU (no HIP call); pinned by tests/test_dispatch_plan.py. */
int gz_conv3d_plan(int op, int N, int C, int D, int H, int W, int K, int OD, int OH, int OW, int KS, int S, int P,
                   char* buf, int buflen) {
    if (!buf || buflen <= 0) return GZ_ERR_BAD_SHAPE;
    buf[0] = 0;
    Conv3DShape s{N, C, D, H, W, K, OD, OH, OW};
    if (KS != 3 || S != 2 || P != 1) return GZ_ERR_UNSUPPORTED;
    if (!shape3_ok(s, KS, S, P) || op < 0 || op > 2 || (op == 1 && (D % S || H % S || W % S))) return GZ_ERR_BAD_SHAPE;
    const Choice c = op == 0 ? choose_fwd3(s, KS, kIdeal) : op == 1 ? choose_dgrad3(s, KS, S, P, kIdeal)
                                                                     : choose_wgrad3(s, KS, kIdeal);
    return snprintf(buf, (size_t)buflen, "%s %s<%s> %s splits=%d slabs=%d", op == 0 ? "F" : op == 1 ? "Dg" : "Wg",
                    c.kind == KIgemm ? "igemm" : c.kind == KIgemm2 ? "igemm2" : "igemm2r", tile_text(c.tile),
                    loader_text3(op, c), c.splits, c.slabs);
}

}  // extern "C"
