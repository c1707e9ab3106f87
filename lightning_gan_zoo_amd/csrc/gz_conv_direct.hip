// The direct (non-implicit-GEMM) convolution kernels: six families for layers an MFMA tile of the igemm skeletons would
// mostly pad -- <= 4 image channels, or <= 32 channels on both sides of a 3x3 -- each with the predicate that admits a
// shape, its block-count helper and its launcher.  choose_* (gz_conv2d_choose.h) decide when one is taken, launch_* (gz_conv_{fwd,dgrad,wgrad}.hip) reach
// this file through gz_conv_direct.h only; the weight images they read are gz_pack.hip's.
//
//   Dg  dgrad_smallc_k4s2p1 / dgrad_smallc4_k4s2p1 (k4 s2 p1 and 5x5 s2 p2 onto <= 4 channels)
//   F / Dg  conv3x3_smallch, conv3x3_fewk (3x3 s1 p1)
//   Wg  wgrad_smallch_k3, wgrad_k3_fewk (3x3 s1 p1), wgrad_k4s2p1_fewc (+ its fused activation-backward form)
#include "gz_conv_direct.h"
#include "gz_knobs.h"
#include "gz_pack_layout.h"
#include "gz_reduce.h"
#include "../../include/gz_ops.h"

namespace gz {

// ---------------------------------------------------------------------------
// Dg with <= 4 image channels (the generator's output layer, 128 -> 3 @ 32 -> 64, and the
// discriminator's input gradient in the gradient penalty): an MFMA tile would waste 29 of 32
// columns, and the layer is HBM-bound anyway (reads 268 MB, 6.4 GFLOP at bs 512).  Direct VALU
// kernel: one lane per input position (n, a, b) produces the 2x2 output pixels of all channels
// from the 3x3 neighbourhood of y; lanes run along b so loads and the 8-byte stores coalesce; the
// per-(phase, ko, tap) weights are wave-uniform 16-byte rows of the packed dgrad image (scalar
// loads).  k4 s2 p1 only.
// ---------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void dgrad_smallc_k4s2p1_kernel(const float* __restrict__ y,
                                                                  const float* __restrict__ wp,
                                                                  const float* __restrict__ bias,
                                                                  float* __restrict__ x, ConvShape s,
                                                                  FastDiv div_ohw, FastDiv div_ow, int act,
                                                                  float slope) {
    const int OHW = s.OH * s.OW;
    const uint32_t M = (uint32_t)s.N * OHW;
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    const bool m_ok = m < M;
    const uint32_t n = fdiv(m, div_ohw);
    const uint32_t pix = m - n * (uint32_t)OHW;
    const int a = (int)fdiv(pix, div_ow);
    const int b = (int)(pix - (uint32_t)a * (uint32_t)s.OW);
    __amdgpu_buffer_rsrc_t rsrc = make_rsrc(y, (uint32_t)s.N * s.K * OHW * 4u);
    uint32_t voff[3][3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            int oy = a + dy - 1, ox = b + dx - 1;
            bool ok = m_ok && (unsigned)oy < (unsigned)s.OH && (unsigned)ox < (unsigned)s.OW;
            voff[dy][dx] = ok ? (n * (uint32_t)(s.K * OHW) + (uint32_t)(oy * s.OW + ox)) * 4u : OOB;
        }
    float acc[2][2][C];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[i][j][c] = 0.f;
    const long long phase_stride = (long long)s.K * 16;    // floats: K * 4 taps * ldc(4)
    for (int ko = 0; ko < s.K; ++ko) {
        float v[3][3];
        const uint32_t soff = (uint32_t)ko * (uint32_t)OHW * 4u;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) v[dy][dx] = bload(rsrc, voff[dy][dx], soff);
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                const float* wrow = wp + (py * 2 + px) * phase_stride + (long long)ko * 16;
#pragma unroll
                for (int ty = 0; ty < 2; ++ty)
#pragma unroll
                    for (int tx = 0; tx < 2; ++tx) {
                        // oy = a + (py+1)/2 - ty  -> neighbourhood row index (oy - a + 1)
                        const float yv = v[(py + 1) / 2 - ty + 1][(px + 1) / 2 - tx + 1];
                        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wrow + (ty * 2 + tx) * 4);
#pragma unroll
                        for (int c = 0; c < C; ++c) acc[py][px][c] = fmaf(yv, w4[c], acc[py][px][c]);
                    }
            }
    }
    if (!m_ok) return;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float bv = bias ? bias[c] : 0.f;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            f32x2 o;
            o.x = act_fwd(acc[py][0][c] + bv, act, slope);
            o.y = act_fwd(acc[py][1][c] + bv, act, slope);
            float* dst = x + (((long long)n * C + c) * s.H + (2 * a + py)) * s.W + 2 * b;
            *reinterpret_cast<f32x2*>(dst) = o;
        }
    }
}

// Same operation, 4 input positions per lane (round 2).  The one-position kernel issues 9 dword loads per lane
// and feature channel -- every y value is requested 9 times, and at 256 B per wave-instruction the vector cache,
// not HBM, sets the pace (186 us for the 268 MB of G's last layer = 1.6 TB/s).  Here a lane owns (n, a, b..b+3):
// per channel it loads the three rows a-1, a, a+1 as ONE aligned 16-byte vector each and takes the two halo
// columns from its neighbour lanes (wave shuffles; at the image edge they are zero), i.e. 0.75 load instructions
// per position instead of 9, then runs the same 48 FMAs per position.  The eight outputs of an output row are two
// 16-byte stores.  Needs OW % 4 == 0 and 16-byte aligned rows.
// The four wavefronts of a workgroup own the SAME 64 lane positions and every fourth feature channel each (the
// channel loop is the only long dimension: at bs 128 one wavefront per 64 positions would leave the chip with 512
// wavefronts); their partial sums meet in LDS and wavefront 0 applies bias / activation and stores.
// KH = 5 (round 3): the 5x5 s2 p2 transposed convolution has the same 3 x 3 neighbourhood (rows a-1 .. a+1) and
// 9 / 6 / 6 / 4 taps per phase; its weights come in the tap-major pack (pack_dgrad_tap: [phase][tap][ko padded][4]).
// Round 5: the wavefront index is read into a scalar register (readfirstlane).  As a per-lane value it made the
// channel index "divergent" for the compiler: the 16 weight rows of a channel were fetched with sixteen 64-lane
// vector loads of ONE address each (1 KB through the vector cache per instruction, 16 KB per channel and wavefront --
// the vector cache, not the 96 packed FMAs, set the pace: 41 us at bs 128) and every y load sat in a waterfall loop.
// With a uniform index they are scalar loads into SGPRs again, as in the unsplit form.  KS = 8 (512 threads): eight
// wavefronts per 64 lane positions -- 4 per SIMD at bs 128 instead of 2; partial sums meet in a binary tree in LDS.
template <int C, int KS, int KH = 4>      // KS = 4 / 8: channel loop split over the workgroup's wavefronts; KS = 1: 256 lane positions
__global__ __launch_bounds__(KS > 4 ? 64 * KS : 256) void dgrad_smallc4_k4s2p1_kernel(const float* __restrict__ y,
                                                                   const float* __restrict__ wp,
                                                                   const float* __restrict__ bias,
                                                                   float* __restrict__ x, ConvShape s,
                                                                   FastDiv div_ohw4, FastDiv div_ow4, int act,
                                                                   float slope, const float* __restrict__ mask = nullptr,
                                                                   float mask_neg = 0.f) {
    // mask != nullptr (round 5, the input gradient of `LeakyReLU(conv(.))`): y is the gradient with respect to the
    // activation's OUTPUT and `mask` the saved forward output, same shape -- y * (mask > 0 ? 1 : mask_neg) is formed on
    // load (three more 16-byte loads per channel instead of an act_bwd launch: read 2, write 1, read 1 of the tensor)
    constexpr int P = KH == 4 ? 1 : 2, TMAX = (KH + 1) / 2;
    __shared__ float part[KS > 1 ? KS / 2 : 1][KS > 1 ? 16 * C : 1][64];
    const int OW4 = s.OW >> 2, OHW = s.OH * s.OW;
    const uint32_t M4 = (uint32_t)s.N * s.OH * OW4;
    const int lane = threadIdx.x & 63, wave = KS > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    const uint32_t m = KS > 1 ? blockIdx.x * 64u + lane : blockIdx.x * 256u + threadIdx.x;
    const bool m_ok = m < M4;
    const uint32_t n = fdiv(m, div_ohw4);
    const uint32_t pix = m - n * (uint32_t)(s.OH * OW4);
    const int a = (int)fdiv(pix, div_ow4);
    const int b = (int)(pix - (uint32_t)a * (uint32_t)OW4) * 4;
    __amdgpu_buffer_rsrc_t rsrc = make_rsrc(y, (uint32_t)s.N * s.K * OHW * 4u);
    uint32_t voff[3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        int oy = a + dy - 1;
        bool ok = m_ok && (unsigned)oy < (unsigned)s.OH;
        voff[dy] = ok ? (n * (uint32_t)(s.K * OHW) + (uint32_t)(oy * s.OW + b)) * 4u : OOB;
    }
    // halo columns come from the neighbour lanes; a lane at the left / right image edge has none (the lane next to
    // it then belongs to another row, or to another wave: both cases are exactly the edge cases)
    const bool has_l = b > 0, has_r = b + 4 < s.OW;
    float acc[4][2][2][C];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int c = 0; c < C; ++c) acc[q][i][j][c] = 0.f;
    const int kpad = round_bk(s.K);
    const long long phase_stride = KH == 4 ? (long long)s.K * 16             // floats: K * 4 taps * ldc(4)
                                           : (long long)TMAX * TMAX * kpad * 4;
    // the next channel's three rows are requested before this channel's 192 FMAs (round 4: with two wavefronts per SIMD
    // nothing else covers the load latency; G's last layer at bs 128: 56 us with the loads issued in place)
    // (the 256-position form, KS = 1, runs 4-7 wavefronts per SIMD and keeps its loads in place: with the prefetch's 26
    // extra registers it measured 80 -> 110 us at bs 256 and 113 -> 133 us at bs 512)
    const __amdgpu_buffer_rsrc_t rmask = make_rsrc(mask ? mask : y, (uint32_t)s.N * s.K * OHW * 4u);
    f32x4 nxt[3], mnx[3];
    if constexpr (KS > 1) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            nxt[dy] = bload4(rsrc, wave < s.K ? voff[dy] : OOB, (uint32_t)wave * (uint32_t)OHW * 4u);
            if (mask) mnx[dy] = bload4(rmask, wave < s.K ? voff[dy] : OOB, (uint32_t)wave * (uint32_t)OHW * 4u);
        }
    }
    for (int ko = wave; ko < s.K; ko += KS) {
        float v[3][6];
        f32x4 cur[3], mcur[3];
        if constexpr (KS > 1) {
            const bool more = ko + KS < s.K;
            const uint32_t soff = (uint32_t)(more ? ko + KS : ko) * (uint32_t)OHW * 4u;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                cur[dy] = nxt[dy];
                nxt[dy] = bload4(rsrc, more ? voff[dy] : OOB, soff);
                if (mask) {
                    mcur[dy] = mnx[dy];
                    mnx[dy] = bload4(rmask, more ? voff[dy] : OOB, soff);
                }
            }
        } else {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                cur[dy] = bload4(rsrc, voff[dy], (uint32_t)ko * (uint32_t)OHW * 4u);
                if (mask) mcur[dy] = bload4(rmask, voff[dy], (uint32_t)ko * (uint32_t)OHW * 4u);
            }
        }
        if (mask) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int e = 0; e < 4; ++e) cur[dy][e] = mcur[dy][e] > 0.f ? cur[dy][e] : cur[dy][e] * mask_neg;
        }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const f32x4 r = cur[dy];
            const float l = __shfl_up(r.w, 1), rr = __shfl_down(r.x, 1);
            v[dy][0] = has_l ? l : 0.f;
            v[dy][1] = r.x; v[dy][2] = r.y; v[dy][3] = r.z; v[dy][4] = r.w;
            v[dy][5] = has_r ? rr : 0.f;
        }
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                const int ny = dg_taps(KH, 2, P, py), nx = dg_taps(KH, 2, P, px);
                const float* wrow = KH == 4 ? wp + (py * 2 + px) * phase_stride + (long long)ko * 16
                                            : wp + (py * 2 + px) * phase_stride + (long long)ko * 4;
#pragma unroll
                for (int ty = 0; ty < TMAX; ++ty)
#pragma unroll
                    for (int tx = 0; tx < TMAX; ++tx) {
                        if (ty < ny && tx < nx) {      // (folded after unrolling)
                            const f32x4 w4 = *reinterpret_cast<const f32x4*>(
                                KH == 4 ? wrow + (ty * 2 + tx) * 4 : wrow + (long long)(ty * nx + tx) * kpad * 4);
                            const int ry = (py + P) / 2 - ty + 1, rx = (px + P) / 2 - tx + 1;
#pragma unroll
                            for (int q = 0; q < 4; ++q)
#pragma unroll
                                for (int c = 0; c < C; ++c)
                                    acc[q][py][px][c] = fmaf(v[ry][q + rx], w4[c], acc[q][py][px][c]);
                        }
                    }
            }
    }
    if constexpr (KS > 1) {
        // binary tree, fixed order: wavefronts [h, 2h) hand their sums to wavefronts [0, h), h = KS/2 .. 1
#pragma unroll
        for (int h = KS / 2; h >= 1; h >>= 1) {
            if (wave >= h && wave < 2 * h) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
#pragma unroll
                            for (int c = 0; c < C; ++c)
                                part[wave - h][((q * 2 + i) * 2 + j) * C + c][lane] = acc[q][i][j][c];
            }
            __syncthreads();
            if (wave < h) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
#pragma unroll
                            for (int c = 0; c < C; ++c)
                                acc[q][i][j][c] += part[wave][((q * 2 + i) * 2 + j) * C + c][lane];
            }
            __syncthreads();
        }
        // the totals go back through LDS once more so that bias, activation (tanh in G's last layer: ~60 instructions
        // per value) and the 16-byte stores are shared by all KS wavefronts instead of wavefront 0 doing all 16 * C
        if (wave == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int c = 0; c < C; ++c) part[0][((q * 2 + i) * 2 + j) * C + c][lane] = acc[q][i][j][c];
        }
        __syncthreads();
        if (!m_ok) return;
        for (int g = wave; g < 4 * C; g += KS) {           // g = (c, py, h): one 16-byte store each
            const int c = g >> 2, py = (g >> 1) & 1, h = g & 1;
            const float bv = bias ? bias[c] : 0.f;
            float* dst = x + (((long long)n * C + c) * s.H + (2 * a + py)) * s.W + 2 * b;
            f32x4 o;
            o.x = act_fwd(part[0][(((2 * h) * 2 + py) * 2 + 0) * C + c][lane] + bv, act, slope);
            o.y = act_fwd(part[0][(((2 * h) * 2 + py) * 2 + 1) * C + c][lane] + bv, act, slope);
            o.z = act_fwd(part[0][(((2 * h + 1) * 2 + py) * 2 + 0) * C + c][lane] + bv, act, slope);
            o.w = act_fwd(part[0][(((2 * h + 1) * 2 + py) * 2 + 1) * C + c][lane] + bv, act, slope);
            *reinterpret_cast<f32x4*>(dst + 4 * h) = o;
        }
        return;
    }
    if (!m_ok) return;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float bv = bias ? bias[c] : 0.f;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            float* dst = x + (((long long)n * C + c) * s.H + (2 * a + py)) * s.W + 2 * b;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 o;
                o.x = act_fwd(acc[2 * h][py][0][c] + bv, act, slope);
                o.y = act_fwd(acc[2 * h][py][1][c] + bv, act, slope);
                o.z = act_fwd(acc[2 * h + 1][py][0][c] + bv, act, slope);
                o.w = act_fwd(acc[2 * h + 1][py][1][c] + bv, act, slope);
                *reinterpret_cast<f32x4*>(dst + 4 * h) = o;
            }
        }
    }
}

// How many wavefronts share the channel loop of 64 lane positions (the KS of dgrad_smallc4_k4s2p1_kernel): enough that
// every SIMD has about four wavefronts to switch between -- a launch has M4 / 64 * KS of them on 1024 SIMDs.
int smallc_split(long long M4, int K) {
    const int forced = knobs().smallc_ks;
    if (forced == 1 || forced == 4 || forced == 8) return K >= 2 * forced || forced == 1 ? forced : 1;
    if (K < 16) return 1;
    if (M4 < knobs().smallc_split8_below && K >= 32) return 8;
    return M4 < knobs().smallc_split_below ? 4 : 1;
}

// 5x5 s2 p2 onto <= 4 channels (HoloGAN's critic: the gradient of its first convolution with respect to the image):
// the four-positions kernel only (rows of OW/4 lanes inside a wavefront, 16-byte aligned tensors, tap-major pack)
bool dgrad_direct5_ok(const ConvShape& s) {
    const bool off = knobs().no_smallc || knobs().no_smallc5;
    return !off && s.C <= 4 && s.H == 2 * s.OH && s.W == 2 * s.OW && s.OW % 4 == 0 && 64 % (s.OW / 4) == 0 &&
           dgrad_tap_major(s.K, 5, 5, 2);
}

template <int C>
static int run_dgrad_smallc5_c(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act,
                             float slope, hipStream_t st, int ks) {
    const long long M4 = (long long)s.N * s.OH * s.OW / 4;
    if (ks == 8)
        hipLaunchKernelGGL((dgrad_smallc4_k4s2p1_kernel<C, 8, 5>), dim3((unsigned)((M4 + 63) / 64)), dim3(512), 0, st, y, wp,
                           bias, x, s, make_fastdiv(s.OH * (s.OW / 4)), make_fastdiv(s.OW / 4), act, slope,
                           (const float*)nullptr, 0.f);
    else if (ks == 4)
        hipLaunchKernelGGL((dgrad_smallc4_k4s2p1_kernel<C, 4, 5>), dim3((unsigned)((M4 + 63) / 64)), dim3(256), 0, st, y, wp,
                           bias, x, s, make_fastdiv(s.OH * (s.OW / 4)), make_fastdiv(s.OW / 4), act, slope,
                           (const float*)nullptr, 0.f);
    else
        hipLaunchKernelGGL((dgrad_smallc4_k4s2p1_kernel<C, 1, 5>), dim3((unsigned)((M4 + 255) / 256)), dim3(256), 0, st, y,
                           wp, bias, x, s, make_fastdiv(s.OH * (s.OW / 4)), make_fastdiv(s.OW / 4), act, slope,
                           (const float*)nullptr, 0.f);
    return launch_status();
}

// the four-positions kernel: a row of OW/4 lanes must not straddle two wavefronts (the halo columns come from the
// neighbour LANES); it also needs 16-byte aligned tensors.  GZ_SMALLC_ONE_POS: the round-1 kernel (experiment)
bool smallc_four_pos(const ConvShape& s) {
    return !knobs().smallc_one_pos && s.OW % 4 == 0 && 64 % (s.OW / 4) == 0;
}

// ks = smallc_split(...): the four-positions kernel; ks = 0: the one-position kernel
template <int C>
static int run_dgrad_smallc_c(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act,
                            float slope, hipStream_t st, int ks, const float* mask = nullptr, float mask_neg = 0.f) {
    long long M = (long long)s.N * s.OH * s.OW;
    if (ks > 0) {
        const long long M4 = M / 4;
        // few lane positions (bs 128 at 32x32: 512 wavefronts): split the channel loop over the workgroup instead
        // (0.080 -> 0.056 ms there; at bs 512 the unsplit form is 2x faster)
        // (round 3: measured crossover between bs 128 and bs 160 at 32x32 feature maps -- 32768 / 40960 lane positions;
        // bs 256: 114 -> 91 us for G's last layer without the split)
        if (ks == 8)
            hipLaunchKernelGGL((dgrad_smallc4_k4s2p1_kernel<C, 8>), dim3((unsigned)((M4 + 63) / 64)), dim3(512), 0, st, y,
                               wp, bias, x, s, make_fastdiv(s.OH * (s.OW / 4)), make_fastdiv(s.OW / 4), act, slope, mask,
                               mask_neg);
        else if (ks == 4)
            hipLaunchKernelGGL((dgrad_smallc4_k4s2p1_kernel<C, 4>), dim3((unsigned)((M4 + 63) / 64)), dim3(256), 0, st, y,
                               wp, bias, x, s, make_fastdiv(s.OH * (s.OW / 4)), make_fastdiv(s.OW / 4), act, slope, mask,
                               mask_neg);
        else
            hipLaunchKernelGGL((dgrad_smallc4_k4s2p1_kernel<C, 1>), dim3((unsigned)((M4 + 255) / 256)), dim3(256), 0, st,
                               y, wp, bias, x, s, make_fastdiv(s.OH * (s.OW / 4)), make_fastdiv(s.OW / 4), act, slope, mask,
                               mask_neg);
        return launch_status();
    }
    if (mask) return GZ_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dgrad_smallc_k4s2p1_kernel<C>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, y, wp, bias,
                       x, s, make_fastdiv(s.OH * s.OW), make_fastdiv(s.OW), act, slope);
    return launch_status();
}

// The channel count is a template parameter of the kernels and a run-time value to the dispatcher.
int run_dgrad_smallc(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act, float slope,
                     hipStream_t st, int ks, const float* mask, float mask_neg) {
    switch (s.C) {
        case 1: return run_dgrad_smallc_c<1>(y, wp, bias, x, s, act, slope, st, ks, mask, mask_neg);
        case 2: return run_dgrad_smallc_c<2>(y, wp, bias, x, s, act, slope, st, ks, mask, mask_neg);
        case 3: return run_dgrad_smallc_c<3>(y, wp, bias, x, s, act, slope, st, ks, mask, mask_neg);
        default: return run_dgrad_smallc_c<4>(y, wp, bias, x, s, act, slope, st, ks, mask, mask_neg);
    }
}

int run_dgrad_smallc5(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act, float slope,
                      hipStream_t st, int ks) {
    switch (s.C) {
        case 1: return run_dgrad_smallc5_c<1>(y, wp, bias, x, s, act, slope, st, ks);
        case 2: return run_dgrad_smallc5_c<2>(y, wp, bias, x, s, act, slope, st, ks);
        case 3: return run_dgrad_smallc5_c<3>(y, wp, bias, x, s, act, slope, st, ks);
        default: return run_dgrad_smallc5_c<4>(y, wp, bias, x, s, act, slope, st, ks);
    }
}

// ---------------------------------------------------------------------------
// F / Dg of 3x3 s1 p1 layers with <= 32 channels on both sides (same layers as wgrad_smallch below).  In the
// 128x32 implicit-GEMM tile half of the MFMA columns are padding when K = 16 and the three kx taps of a row are
// fetched three times.  Here a wavefront owns 16 consecutive pixels of one output row: B = x[4 channels][16
// pixels] comes from ONE dword load per lane and row, the kx = -1 / +1 operands are the same registers shifted
// by one lane (plus one predicated edge load), A = w[16 output channels][4 input channels] of the tap is read
// from an LDS copy of the packed weights staged once per workgroup, and v_mfma_f32_16x16x4_f32 accumulates
// D[output channel][pixel] -- stores are 64-byte runs per channel.  Dg is the same kernel on gy with the taps
// mirrored (tap' = 8 - tap) and the roles of K and C exchanged; both read the weight images the implicit-GEMM
// path uses (tap-major when the input side has >= 16 channels, (c, tap)-major otherwise).
// ---------------------------------------------------------------------------
template <int OT, int IT>     // 16-channel blocks on the output / input side
__global__ __launch_bounds__(256) void conv3x3_smallch_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                              const float* __restrict__ bias, float* __restrict__ out,
                                                              int N, int CI, int CO, int H, int W, int groups,
                                                              FastDiv div_seg, FastDiv div_h, int tap_major, int inpad,
                                                              int ld, int flip, int act, float slope) {
    constexpr int CB = IT * 4;                       // input-channel quads
    __shared__ float Ws[9 * CB * OT * 64];           // [tap][cb][ot][q][i]
    for (int e = threadIdx.x; e < 9 * CB * OT * 64; e += 256) {
        const int i = e & 15, q = (e >> 4) & 3;
        int rest = e >> 6;
        const int ot = rest % OT;
        rest /= OT;
        const int cb = rest % CB, tap = rest / CB;
        const int co = ot * 16 + i, ci = cb * 4 + q;
        const int t = flip ? 8 - tap : tap;
        float v = 0.f;
        if (co < CO && ci < CI) v = wp[(long long)(tap_major ? t * inpad + ci : ci * 9 + t) * ld + co];
        Ws[e] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int HW = H * W;
    // descriptor moved back by one image row: the per-lane voffset addresses row h - 1 + 1 = h of channel q, the
    // (row, channel-quad) step is a wave-uniform scalar offset, so the inner loop has no per-lane address math
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(reinterpret_cast<const char*>(in) - (size_t)W * 4,
                                                 (uint32_t)N * CI * HW * 4u + (uint32_t)W * 4u);
    const int segs = W >> 4;
    const int nwaves = gridDim.x * 4;
    for (int g = blockIdx.x * 4 + wave; g < groups; g += nwaves) {
        const uint32_t rowid = fdiv((uint32_t)g, div_seg);               // n * H + h
        const int w0 = (g - (int)rowid * segs) << 4;
        const uint32_t n = fdiv(rowid, div_h);
        const int h = (int)(rowid - n * (uint32_t)H);
        const uint32_t vmain = ((n * (uint32_t)CI + q) * (uint32_t)HW + (uint32_t)(h * W + w0 + i)) * 4u;
        uint32_t vedge = OOB;
        if (i == 0 && w0 > 0) vedge = vmain - 4u;
        if (i == 15 && w0 + 16 < W) vedge = vmain + 4u;
        f32x4 acc[OT];
#pragma unroll
        for (int a = 0; a < OT; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int hh = h + dy - 1;
            if ((unsigned)hh >= (unsigned)H) continue;                   // wave-uniform
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const bool cok = cb * 4 + q < CI;
                const uint32_t soff = (uint32_t)(cb * 4 * HW + dy * W) * 4u;
                const float v0 = bload(rin, cok ? vmain : OOB, soff);
                // lanes 0 / 15 of each 16-lane row fetch the pixel left / right of the segment (zero in the padding)
                const float ev = bload(rin, cok ? vedge : OOB, soff);
                float left = __shfl_up(v0, 1, 16), right = __shfl_down(v0, 1, 16);
                if (i == 0) left = ev;
                if (i == 15) right = ev;
                const float* wrow = Ws + ((dy * 3) * CB + cb) * OT * 64 + lane;
#pragma unroll
                for (int a = 0; a < OT; ++a) {
                    acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[(0 * CB) * OT * 64 + a * 64], left, acc[a], 0, 0, 0);
                    acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[(1 * CB) * OT * 64 + a * 64], v0, acc[a], 0, 0, 0);
                    acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[(2 * CB) * OT * 64 + a * 64], right, acc[a], 0, 0, 0);
                }
            }
        }
        // D[row = output channel 4q + r][column = pixel i]
#pragma unroll
        for (int a = 0; a < OT; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = a * 16 + 4 * q + r;
                if (co < CO) {
                    const float bv = bias ? bias[co] : 0.f;
                    out[((long long)(n * (uint32_t)CO + co) * H + h) * W + w0 + i] = act_fwd(acc[a][r] + bv, act, slope);
                }
            }
    }
}

// ... with at most 4 output channels on 64-pixel-wide maps (HoloGAN's last layer, 64 -> 3 + tanh): the MFMA tile above
// multiplies 13 padding rows of 16 (81 us for one read of a 67 MB activation).  Plain FMAs: a workgroup owns an
// 8-row x 64-pixel block of one sample, lane = (row, 8-pixel segment) as in wgrad_k3_fewk_kernel; its four wavefronts
// take a quarter of the input channels each and meet in LDS in a fixed order.  Same weight images, `flip` as above.
template <int KK>
__global__ __launch_bounds__(256) void conv3x3_fewk_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                           const float* __restrict__ bias, float* __restrict__ out, int N,
                                                           int CI, int CO, int H, int tap_major, int inpad, int ld,
                                                           int flip, int act, float slope) {
    __shared__ float Ws[64 * 9 * KK];                // [ci][tap][k]
    __shared__ float red[3][KK * 8][64];
    for (int e = threadIdx.x; e < CI * 9 * KK; e += 256) {
        const int k = e % KK, tap = (e / KK) % 9, ci = e / (9 * KK);
        const int t = flip ? 8 - tap : tap;
        Ws[e] = k < CO ? wp[(long long)(tap_major ? t * inpad + ci : ci * 9 + t) * ld + k] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rbs = H >> 3, HW = H * 64;
    const int n = blockIdx.x / rbs, rb = blockIdx.x - n * rbs;
    const int r = lane >> 3, sg = lane & 7, h = rb * 8 + r, w0 = sg * 8;
    const int cq = (CI + 3) >> 2, c0 = wave * cq, c1 = min(CI, c0 + cq);
    float acc[KK][8];
#pragma unroll
    for (int k = 0; k < KK; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    const float* xn = in + (long long)n * CI * HW + w0;
    // the next channel's rows are requested before this channel's FMAs (two wavefronts per SIMD: nothing else covers
    // the load latency)
    auto load_rows = [&](int ci, f32x4 (&rws)[6]) {
        const float* xc = xn + (long long)ci * HW;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int hh = h + d - 1;
            const bool ok = (unsigned)hh < (unsigned)H;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            rws[2 * d] = ok ? *reinterpret_cast<const f32x4*>(xc + hh * 64) : z;
            rws[2 * d + 1] = ok ? *reinterpret_cast<const f32x4*>(xc + hh * 64 + 4) : z;
        }
    };
    f32x4 nxt[6];
    if (c0 < c1) load_rows(c0, nxt);
    for (int ci = c0; ci < c1; ++ci) {
        f32x4 cur[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) cur[e] = nxt[e];
        if (ci + 1 < c1) load_rows(ci + 1, nxt);
        float xr[3][10];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const f32x4 v0 = cur[2 * d], v1 = cur[2 * d + 1];
            const float left = __shfl_up(v1[3], 1, 64), right = __shfl_down(v0[0], 1, 64);
            xr[d][0] = sg == 0 ? 0.f : left;
            xr[d][1] = v0[0]; xr[d][2] = v0[1]; xr[d][3] = v0[2]; xr[d][4] = v0[3];
            xr[d][5] = v1[0]; xr[d][6] = v1[1]; xr[d][7] = v1[2]; xr[d][8] = v1[3];
            xr[d][9] = sg == 7 ? 0.f : right;
        }
        const float* wc = Ws + ci * 9 * KK;
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                for (int k = 0; k < KK; ++k) {
                    const float wv = wc[(d * 3 + tx) * KK + k];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(wv, xr[d][j + tx], acc[k][j]);
                }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < KK; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) red[wave - 1][k * 8 + j][lane] = acc[k][j];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            if (k >= CO) continue;
            const float bv = bias ? bias[k] : 0.f;
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = ((acc[k][j] + red[0][k * 8 + j][lane]) + red[1][k * 8 + j][lane]) + red[2][k * 8 + j][lane];
                o[j] = act_fwd(v + bv, act, slope);
            }
            float* dst = out + ((long long)(n * CO + k) * H + h) * 64 + w0;
            *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
            *reinterpret_cast<f32x4*>(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
        }
    }
}

bool conv3_fewk_ok(int CI, int CO, int H, int W) {          // (and 16-byte aligned tensors: choose_fwd / choose_dgrad)
    return !knobs().no_fewk_conv && CO <= 4 && CI <= 64 && W == 64 && (H & 7) == 0;
}

bool conv3_smallch_ok(int N, int CI, int CO, int H, int W) {
    const bool off = knobs().no_smallch_conv;
    // measured against the implicit-GEMM path (tools/resnet_bench.py): wins when the output side fits one 16-row
    // MFMA tile and the input side fills at least half a 16-channel block (16->16 @ 128x128: 123 -> 72 us);
    // loses for 3 input channels (K dimension mostly padding) and for 32 output channels
    return !off && CO <= 16 && CI > 8 && CI <= 64 && (W & 15) == 0 && (long long)N * H * W >= 65536;
}

int run_conv3_smallch(const float* in, const float* wp, const float* bias, float* out, int N, int CI, int CO,
                             int H, int W, int tap_major, int flip, int act, float slope, hipStream_t st, Loader ld) {
    if (ld == LFewk) {
        const dim3 grid((unsigned)(N * (H >> 3)));
#define GZ_FEWK(KK_)                                                                                                  \
    hipLaunchKernelGGL((conv3x3_fewk_kernel<KK_>), grid, dim3(256), 0, st, in, wp, bias, out, N, CI, CO, H, tap_major, \
                       round_bk(CI), round4(CO), flip, act, slope)
        if (CO == 1) GZ_FEWK(1);
        else if (CO == 2) GZ_FEWK(2);
        else if (CO == 3) GZ_FEWK(3);
        else GZ_FEWK(4);
#undef GZ_FEWK
        return launch_status();
    }
    const int groups = N * H * (W >> 4);
    const int gpw = knobs().c3_gpw;
    long long blocks = (groups + 4 * gpw - 1) / (4 * gpw);   // >= gpw pixel groups per wavefront: the weights are staged per workgroup
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    const FastDiv dseg = make_fastdiv(W >> 4), dh = make_fastdiv(H);
    const int ot = (CO + 15) / 16, it = (CI + 15) / 16;
#define GZ_C3(OT_, IT_)                                                                                              \
    hipLaunchKernelGGL((conv3x3_smallch_kernel<OT_, IT_>), dim3((unsigned)blocks), dim3(256), 0, st, in, wp, bias, out, \
                       N, CI, CO, H, W, groups, dseg, dh, tap_major, round_bk(CI), round4(CO), flip, act, slope)
    (void)ot;                                        // conv3_smallch_ok admits one output block only
    if (it == 1) GZ_C3(1, 1);
    else if (it == 2) GZ_C3(1, 2);
    else GZ_C3(1, 4);
#undef GZ_C3
    return launch_status();
}

// ---------------------------------------------------------------------------
// Wg of 3x3 s1 p1 layers with few channels (ceil(K/16) * ceil(C/16) <= 4: the 128x128 / 64x64 stages of the R1
// ResNets, the image-side convolutions 64 -> 3 / 3 -> 16).  As an implicit GEMM this is M = K <= 32 rows of a 64-row tile: three quarters of
// the MFMA work multiplies padding.  Here one wavefront owns 16 consecutive pixels of one image row and issues
// v_mfma_f32_16x16x4_f32 with A = y[ko][4 pixels], B = x[c][the same 4 pixels shifted by the tap]: 9 * KT * CT
// exact 16x16 tiles, nothing padded.  Lane (i = l & 15, q = l >> 4) loads ONE aligned float4 per operand row i
// (pixels 4q..4q+3); the dx = -1 / +1 taps are assembled from the neighbouring lanes' vectors (lane +-16) plus
// one edge dword, rows in the vertical padding are skipped wave-uniformly.  Each workgroup sums its four
// wavefronts through LDS in a fixed order and writes one slab; reduce_slabs_kernel adds the slabs.
// ---------------------------------------------------------------------------
template <int KT, int CT>
__global__ __launch_bounds__(256) void wgrad_smallch_k3_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               float* __restrict__ slab, ConvShape s, int groups,
                                                               FastDiv div_seg, FastDiv div_h) {
    constexpr int NACC = KT * CT * 9;
    __shared__ float red[KT * CT * 9 * 256];
    __shared__ float bsum[4][KT * 16];
    float ysum[KT];                 // the bias gradient sum_pixels y[ko] comes for free: y is read here anyway
#pragma unroll
    for (int a = 0; a < KT; ++a) ysum[a] = 0.f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int H = s.H, W = s.W, HW = s.H * s.W;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x, (uint32_t)s.N * s.C * HW * 4u);
    const __amdgpu_buffer_rsrc_t ry = make_rsrc(y, (uint32_t)s.N * s.K * HW * 4u);
    f32x4 acc[KT][CT][9];
#pragma unroll
    for (int a = 0; a < KT; ++a)
#pragma unroll
        for (int b = 0; b < CT; ++b)
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[a][b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int segs = W >> 4;
    const int nwaves = gridDim.x * 4;
    for (int g = blockIdx.x * 4 + wave; g < groups; g += nwaves) {
        const uint32_t rowid = fdiv((uint32_t)g, div_seg);               // n * H + h
        const int w0 = (g - (int)rowid * segs) << 4;
        const uint32_t n = fdiv(rowid, div_h);
        const int h = (int)(rowid - n * (uint32_t)H);
        const int wq = w0 + 4 * q;
        f32x4 yv[KT];
#pragma unroll
        for (int a = 0; a < KT; ++a) {
            const int ko = a * 16 + i;
            yv[a] = bload4(ry, ko < s.K ? ((n * (uint32_t)s.K + ko) * (uint32_t)HW + (uint32_t)(h * W + wq)) * 4u : OOB, 0);
            ysum[a] += (yv[a][0] + yv[a][1]) + (yv[a][2] + yv[a][3]);
        }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int hh = h + dy - 1;
            if ((unsigned)hh >= (unsigned)H) continue;                   // wave-uniform: a padding row contributes nothing
#pragma unroll
            for (int b = 0; b < CT; ++b) {
                const int c = b * 16 + i;
                const uint32_t base = ((n * (uint32_t)s.C + c) * (uint32_t)HW + (uint32_t)(hh * W + wq)) * 4u;
                const bool cok = c < s.C;
                const f32x4 cv = bload4(rx, cok ? base : OOB, 0);
                // the pixel left of this lane's vector: lane - 16 holds it, except for q == 0 (previous segment / padding)
                float left = __shfl_up(cv[3], 16, 64);
                float right = __shfl_down(cv[0], 16, 64);
                const float el = bload(rx, (cok && q == 0 && wq > 0) ? base - 4u : OOB, 0);
                const float er = bload(rx, (cok && q == 3 && wq + 4 < W) ? base + 16u : OOB, 0);
                if (q == 0) left = el;
                if (q == 3) right = er;
                const f32x4 lv = {left, cv[0], cv[1], cv[2]};
                const f32x4 rv = {cv[1], cv[2], cv[3], right};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int a = 0; a < KT; ++a) {
                        acc[a][b][dy * 3 + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a][j], lv[j], acc[a][b][dy * 3 + 0], 0, 0, 0);
                        acc[a][b][dy * 3 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a][j], cv[j], acc[a][b][dy * 3 + 1], 0, 0, 0);
                        acc[a][b][dy * 3 + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a][j], rv[j], acc[a][b][dy * 3 + 2], 0, 0, 0);
                    }
                }
            }
        }
    }
    // workgroup sum in a fixed order: wave 0 stores, waves 1..3 add in turn
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int a = 0; a < KT; ++a)
#pragma unroll
                for (int b = 0; b < CT; ++b)
#pragma unroll
                    for (int t = 0; t < 9; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float* dst = &red[(((a * CT + b) * 9 + t) * 4 + r) * 64 + lane];
                            *dst = (w == 0 ? 0.f : *dst) + acc[a][b][t][r];
                        }
        }
        __syncthreads();
    }
    // bias gradient: lanes i, i+16, i+32, i+48 hold the same channel; then the four wavefronts in order
#pragma unroll
    for (int a = 0; a < KT; ++a) {
        float v = ysum[a];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 16) bsum[wave][a * 16 + lane] = v;
    }
    __syncthreads();
    // slab row of this workgroup: K*C*9 weight-gradient entries followed by K bias-gradient entries
    float* out = slab + (long long)blockIdx.x * ((long long)s.K * s.C * 9 + s.K);
    if (threadIdx.x < KT * 16 && (int)threadIdx.x < s.K)
        out[(long long)s.K * s.C * 9 + threadIdx.x] =
            ((bsum[0][threadIdx.x] + bsum[1][threadIdx.x]) + bsum[2][threadIdx.x]) + bsum[3][threadIdx.x];
    // D layout of the 16x16 tile: register r of lane l is (row 4 * (l >> 4) + r, column l & 15) = (ko, c)
    for (int e = threadIdx.x; e < NACC * 256; e += 256) {
        const int l = e & 63, r = (e >> 6) & 3, rest = e >> 8;
        const int t = rest % 9, ab = rest / 9;
        const int ko = (ab / CT) * 16 + 4 * (l >> 4) + r, c = (ab % CT) * 16 + (l & 15);
        if (ko < s.K && c < s.C) out[((long long)ko * s.C + c) * 9 + t] = red[e];
    }
}

// ---------------------------------------------------------------------------
// ... and with at most 4 OUTPUT channels on 64-pixel-wide maps (HoloGAN's last layer, Conv2d(64, 3, k3, p1) at 64x64,
// core/models/hologan_generator.py:65): the 16x16x4 MFMA above multiplies 13 padding rows out of 16 and ran at
// 6 TFLOP/s (150 us for 0.9 GFLOP; the layer is one read of a 67 MB activation).  Plain FMAs instead: a wavefront owns
// one input channel and an 8-row x 64-pixel block -- lane = (row, 8-pixel segment) -- keeps the 9 * K sums of its
// channel in registers while it walks the samples of its slice, and adds the 64 lanes once at the end.  The image rows
// come as aligned float4 loads, the two halo pixels of a segment from the neighbouring lanes.  One slab row per
// (row block, sample slice); reduce_slabs_kernel adds them (and the bias gradient in the row's tail).
// ---------------------------------------------------------------------------
template <int KK>
__global__ __launch_bounds__(256) void wgrad_k3_fewk_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            float* __restrict__ slab, ConvShape s, int nslices,
                                                            int n_per_slice) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = s.H, HW = s.H * 64, rbs = s.H >> 3;
    int b = blockIdx.x;
    const int ns = b % nslices;
    b /= nslices;
    const int rb = b % rbs, c = (b / rbs) * 4 + wave;
    if (c >= s.C) return;                                     // (wave-uniform)
    const int r = lane >> 3, sg = lane & 7, h = rb * 8 + r, w0 = sg * 8;
    float acc[KK][9], ysum[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        ysum[k] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[k][t] = 0.f;
    }
    const int n0 = ns * n_per_slice, n1 = min(s.N, n0 + n_per_slice);
    // the next sample's rows are requested before this sample's FMAs (see conv3x3_fewk_kernel)
    auto load_rows = [&](int n, f32x4 (&rws)[6], f32x4 (&yws)[2 * KK]) {
        const float* xc = x + ((long long)n * s.C + c) * HW + w0;
        const float* yn = y + (long long)n * s.K * HW + h * 64 + w0;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int hh = h + d - 1;
            const bool ok = (unsigned)hh < (unsigned)H;
            rws[2 * d] = ok ? *reinterpret_cast<const f32x4*>(xc + hh * 64) : z;
            rws[2 * d + 1] = ok ? *reinterpret_cast<const f32x4*>(xc + hh * 64 + 4) : z;
        }
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            yws[2 * k] = k < s.K ? *reinterpret_cast<const f32x4*>(yn + (long long)k * HW) : z;
            yws[2 * k + 1] = k < s.K ? *reinterpret_cast<const f32x4*>(yn + (long long)k * HW + 4) : z;
        }
    };
    f32x4 nxt[6], ynx[2 * KK];
    if (n0 < n1) load_rows(n0, nxt, ynx);
    for (int n = n0; n < n1; ++n) {
        f32x4 cur[6], ycur[2 * KK];
#pragma unroll
        for (int e = 0; e < 6; ++e) cur[e] = nxt[e];
#pragma unroll
        for (int e = 0; e < 2 * KK; ++e) ycur[e] = ynx[e];
        if (n + 1 < n1) load_rows(n + 1, nxt, ynx);
        float xr[3][10];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const f32x4 v0 = cur[2 * d], v1 = cur[2 * d + 1];
            const float left = __shfl_up(v1[3], 1, 64), right = __shfl_down(v0[0], 1, 64);
            xr[d][0] = sg == 0 ? 0.f : left;
            xr[d][1] = v0[0]; xr[d][2] = v0[1]; xr[d][3] = v0[2]; xr[d][4] = v0[3];
            xr[d][5] = v1[0]; xr[d][6] = v1[1]; xr[d][7] = v1[2]; xr[d][8] = v1[3];
            xr[d][9] = sg == 7 ? 0.f : right;
        }
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            float yv[8];
            {
                const f32x4 a = ycur[2 * k], bq = ycur[2 * k + 1];
                yv[0] = a[0]; yv[1] = a[1]; yv[2] = a[2]; yv[3] = a[3];
                yv[4] = bq[0]; yv[5] = bq[1]; yv[6] = bq[2]; yv[7] = bq[3];
            }
            if (c == 0) ysum[k] += ((yv[0] + yv[1]) + (yv[2] + yv[3])) + ((yv[4] + yv[5]) + (yv[6] + yv[7]));
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int tx = 0; tx < 3; ++tx) {
                    float a = acc[k][d * 3 + tx];
#pragma unroll
                    for (int j = 0; j < 8; ++j) a = fmaf(yv[j], xr[d][j + tx], a);
                    acc[k][d * 3 + tx] = a;
                }
        }
    }
    const long long count = (long long)s.K * s.C * 9;
    float* out = slab + (long long)(rb * nslices + ns) * (count + s.K);
#pragma unroll
    for (int k = 0; k < KK; ++k) {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float v = wave_sum(acc[k][t]);
            if (lane == 0 && k < s.K) out[((long long)k * s.C + c) * 9 + t] = v;
        }
        if (c == 0) {
            const float v = wave_sum(ysum[k]);
            if (lane == 0 && k < s.K) out[count + k] = v;
        }
    }
}

bool wgrad_fewk_ok(const ConvShape& s) {
    return !knobs().no_fewk_wg && s.K <= 4 && s.W == 64 && (s.H & 7) == 0 && s.OH == s.H && s.OW == s.W;
}

static int wgrad_fewk_slices(const ConvShape& s) {       // sample slices: ~4 workgroups per CU in all
    const long long base = (long long)((s.C + 3) / 4) * (s.H >> 3);
    long long want = (4LL * cus() + base - 1) / base;
    if (want > s.N) want = s.N;
    if (want < 1) want = 1;
    const int per = (int)((s.N + want - 1) / want);
    return (s.N + per - 1) / per;
}

bool wgrad_smallch_ok(const ConvShape& s, int KH, int KW, int S, int P) {
    const bool off = knobs().no_smallch_wg;
    const int kt = (s.K + 15) / 16, ct = (s.C + 15) / 16;      // 16x16 tiles per tap: at most 4 (36 accumulators)
    return !off && KH == 3 && KW == 3 && S == 1 && P == 1 && kt * ct <= 4 && (s.W & 15) == 0 &&
           (long long)s.N * s.H * s.W >= 65536;
}

int wgrad_smallch_blocks(const ConvShape& s) {
    if (wgrad_fewk_ok(s)) return (s.H >> 3) * wgrad_fewk_slices(s);       // slab rows
    long long groups = (long long)s.N * s.H * (s.W >> 4);
    long long blocks = (groups + 15) / 16;          // >= 4 pixel groups per wavefront
    return (int)(blocks > 1024 ? 1024 : (blocks < 1 ? 1 : blocks));
}

int run_wgrad_smallch(const float* x, const float* y, float* dw, float* dbias, float* ws, size_t ws_bytes,
                             const ConvShape& s, Loader ld, hipStream_t st) {
    const int blocks = wgrad_smallch_blocks(s);
    const long long count = (long long)s.K * s.C * 9;
    if (!ws || ws_bytes < (size_t)blocks * (count + s.K) * 4) return GZ_ERR_WORKSPACE;
    const long long row = count + s.K;
    const long long outs = dbias ? row : count;
    if (ld == LFewk) {
        const int nsl = wgrad_fewk_slices(s), per = (s.N + nsl - 1) / nsl;
        const dim3 grid((unsigned)(((s.C + 3) / 4) * (s.H >> 3) * nsl));
        switch (s.K) {
            case 1: hipLaunchKernelGGL((wgrad_k3_fewk_kernel<1>), grid, dim3(256), 0, st, x, y, ws, s, nsl, per); break;
            case 2: hipLaunchKernelGGL((wgrad_k3_fewk_kernel<2>), grid, dim3(256), 0, st, x, y, ws, s, nsl, per); break;
            case 3: hipLaunchKernelGGL((wgrad_k3_fewk_kernel<3>), grid, dim3(256), 0, st, x, y, ws, s, nsl, per); break;
            default: hipLaunchKernelGGL((wgrad_k3_fewk_kernel<4>), grid, dim3(256), 0, st, x, y, ws, s, nsl, per);
        }
        launch_reduce_slabs(ws, dw, blocks, outs, row, dbias, count, st);
        return launch_status();
    }
    const int groups = s.N * s.H * (s.W >> 4);
    const FastDiv dseg = make_fastdiv(s.W >> 4), dh = make_fastdiv(s.H);
    const int kt = (s.K + 15) / 16, ct = (s.C + 15) / 16;
#define GZ_SMALLCH(KT_, CT_) \
    hipLaunchKernelGGL((wgrad_smallch_k3_kernel<KT_, CT_>), dim3(blocks), dim3(256), 0, st, x, y, ws, s, groups, dseg, dh)
    if (kt == 1 && ct == 1) GZ_SMALLCH(1, 1);
    else if (kt == 1 && ct == 2) GZ_SMALLCH(1, 2);
    else if (kt == 2 && ct == 1) GZ_SMALLCH(2, 1);
    else if (kt == 2 && ct == 2) GZ_SMALLCH(2, 2);
    else if (kt == 1 && ct <= 4) GZ_SMALLCH(1, 4);
    else GZ_SMALLCH(4, 1);
#undef GZ_SMALLCH
    // slab rows are count + K long; without a dbias pointer the K-long tails are simply not reduced
    launch_reduce_slabs(ws, dw, blocks, outs, row, dbias, count, st);
    return launch_status();
}

// ---------------------------------------------------------------------------
// Wg of k4 s2 p1 layers with <= 4 channels on the image side (the critics' first convolution and -- as the adjoint --
// G's last transposed convolution): dw[k][c][ky][kx] = sum over (n, oy, ox) of y[n][k][oy][ox] *
// x[n][c][2 oy - 1 + ky][2 ox - 1 + kx], a K x (C * 16) result from a reduction over all N * OH * OW pixels.  On the
// implicit-GEMM skeleton that is ONE 64 x 64 or 128 x 64 tile split 512 ways: prologue, epilogue and a BK-chunk per
// workgroup (36 / 28 us at bs 128 for 5 / 9 us of HBM time).  Here v_mfma_f32_16x16x4_f32 runs with k = 4 pixels:
// A[channel k][pixel] comes from ONE 16-byte load per lane, 16-channel block and 16-pixel segment (component j of the
// vector feeds MFMA j: pixel ox0 + 4 q + j -- any assignment of pixels to k slots is as good as another, as long as B
// uses the same); B[pixel][(ky, kx)] = x[c][2 oy - 1 + ky][2 (ox0 + 4 q + j) - 1 + kx] is one dword load per lane, c
// and j (padding columns are out-of-range voffsets, padding rows wave-uniform).  A wavefront walks its share of the
// (n, oy, segment) items with the next item's loads in flight; the four wavefronts of a workgroup meet in an LDS tree
// and wavefront 0 writes the workgroup's slab (the same slabs gz_reduce_multi / the optimizer read).  In the step at
// bs 128 (inputs cold): D.conv_in 36 -> 27 us.  (Issuing the loads of four items at once measured 35 us.)
// ---------------------------------------------------------------------------
// FUSE (round 5, the first-order backward of `LeakyReLU(conv(x) + bias)`): the operand is the gradient with respect to
// the ACTIVATION's output, masked on load with the saved forward output (g * (out > 0 ? 1 : slope) -- the act_bwd
// launch and its write + re-read of the 34 MB gradient disappear), and a (C+1)-th column block multiplies it with a
// column of ones: D[k][0] = sum over the pixels = the bias gradient, which lands behind the K * C * 16 weight-gradient
// values of the workgroup's slab (a channel_sum launch and its second read of the gradient disappear).
template <int C, int KT, bool FUSE>      // image channels; 16-channel blocks on the feature side
__global__ __launch_bounds__(256) void wgrad_k4s2p1_fewc_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ fwd_out, float* __restrict__ slab,
                                                                int N, int K, int H, int W, int OH, int OW, int items,
                                                                FastDiv div_seg, FastDiv div_oh, int act, float slope,
                                                                long long slab_stride) {
    constexpr int CB = FUSE ? C + 1 : C;
    __shared__ float part[2][KT * CB * 4][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, q = lane >> 4;
    const int ky = i >> 2, kx = i & 3;
    const int HW = H * W, OHW = OH * OW;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x, (uint32_t)N * C * HW * 4u);
    const __amdgpu_buffer_rsrc_t ry = make_rsrc(y, (uint32_t)N * K * OHW * 4u);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(FUSE ? fwd_out : y, (uint32_t)N * K * OHW * 4u);
    const float neg = act == ACT_RELU ? 0.f : slope;
    const float ones = i == 0 ? 1.f : 0.f;
    const int segs = OW >> 4;
    const int nwaves = gridDim.x * 4;
    auto fetch = [&](int g, f32x4 (&ya)[KT], f32x4 (&oa)[FUSE ? KT : 1], float (&xb)[C][4]) {
        const uint32_t rowid = fdiv((uint32_t)g, div_seg);               // n * OH + oy
        const int ox0 = (g - (int)rowid * segs) << 4;
        const uint32_t n = fdiv(rowid, div_oh);
        const int oy = (int)(rowid - n * (uint32_t)OH);
        const uint32_t vy = ((n * (uint32_t)K + i) * (uint32_t)OHW + (uint32_t)(oy * OW + ox0 + 4 * q)) * 4u;
#pragma unroll
        for (int a = 0; a < KT; ++a) {
            ya[a] = bload4(ry, vy, (uint32_t)(a * 16 * OHW) * 4u);
            if constexpr (FUSE) oa[a] = bload4(ro, vy, (uint32_t)(a * 16 * OHW) * 4u);
        }
        const int row = 2 * oy - 1 + ky;
        const bool rok = (unsigned)row < (unsigned)H;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 2 * (ox0 + 4 * q + j) - 1 + kx;
            const uint32_t vx = (rok && (unsigned)col < (unsigned)W)
                                    ? (n * (uint32_t)(C * HW) + (uint32_t)(row * W + col)) * 4u : OOB;
#pragma unroll
            for (int c = 0; c < C; ++c) xb[c][j] = bload(rx, vx, (uint32_t)(c * HW) * 4u);
        }
    };
    f32x4 acc[KT][CB];
#pragma unroll
    for (int a = 0; a < KT; ++a)
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    int g = blockIdx.x * 4 + wave;
    if (g < items) {
        f32x4 yc[KT], yn[KT], oc[FUSE ? KT : 1], on[FUSE ? KT : 1];
        float xc[C][4], xn[C][4];
        fetch(g, yc, oc, xc);
        for (; g < items; g += nwaves) {
            const bool more = g + nwaves < items;
            if (more) fetch(g + nwaves, yn, on, xn);      // in flight during this item's 4 * KT * CB MFMAs
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int a = 0; a < KT; ++a) {
                    float av = yc[a][j];
                    if constexpr (FUSE) av = oc[a][j] > 0.f ? av : av * neg;
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc[c][j], acc[a][c], 0, 0, 0);
                    if constexpr (FUSE) acc[a][C] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ones, acc[a][C], 0, 0, 0);
                }
            if (more) {
#pragma unroll
                for (int a = 0; a < KT; ++a) {
                    yc[a] = yn[a];
                    if constexpr (FUSE) oc[a] = on[a];
                }
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j) xc[c][j] = xn[c][j];
            }
        }
    }
    // binary tree over the four wavefronts, fixed order
#pragma unroll
    for (int h = 2; h >= 1; h >>= 1) {
        if (wave >= h && wave < 2 * h) {
#pragma unroll
            for (int a = 0; a < KT; ++a)
#pragma unroll
                for (int c = 0; c < CB; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) part[wave - h][(a * CB + c) * 4 + r][lane] = acc[a][c][r];
        }
        __syncthreads();
        if (wave < h) {
#pragma unroll
            for (int a = 0; a < KT; ++a)
#pragma unroll
                for (int c = 0; c < CB; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[a][c][r] += part[wave][(a * CB + c) * 4 + r][lane];
        }
        __syncthreads();
    }
    if (wave > 0) return;
    // D[row = channel 16 a + 4 q + r][column = (ky, kx)]  ->  dw[k][c][ky][kx]; the ones column -> dbias[k]
    float* out = slab + (long long)blockIdx.x * slab_stride;
#pragma unroll
    for (int a = 0; a < KT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int c = 0; c < C; ++c) out[((a * 16 + 4 * q + r) * C + c) * 16 + i] = acc[a][c][r];
            if constexpr (FUSE) {
                if (i == 0) out[K * C * 16 + a * 16 + 4 * q + r] = acc[a][C][r];
            }
        }
}

bool wgrad_k4s2p1_fewc_ok(const ConvShape& s) {
    // (K = 128, G's last layer: 29 us against the tile path's 28 in the step at bs 128 -- not taken)
    return !knobs().no_fewc_wg && s.C <= 4 && (s.K == 16 || s.K == 32 || s.K == 64) &&
           s.H == 2 * s.OH && s.W == 2 * s.OW && s.OW % 16 == 0 && (long long)s.N * s.K * s.OH * s.OW < (1ll << 29) &&
           (long long)s.N * s.OH * (s.OW >> 4) >= 1024;
}

int wgrad_k4s2p1_fewc_blocks(const ConvShape& s) {
    const long long items = (long long)s.N * s.OH * (s.OW >> 4);
    long long blocks = items / (4 * 4);                       // >= 4 items per wavefront
    const long long cap = knobs().fewc_wg_blocks;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

// fwd_out != nullptr: the fused form (y = gradient w.r.t. the activation output, masked with fwd_out; slab rows carry
// the K bias-gradient values behind the K * C * 16 weight-gradient values).  The fused form is always left unreduced
// (gz_conv2d_wgrad_act_partial).
int run_wgrad_k4s2p1_fewc(const float* x, const float* y, const float* fwd_out, int act, float slope, float* dw,
                                 float* ws, size_t ws_bytes, const ConvShape& s, hipStream_t st) {
    const bool fuse = fwd_out != nullptr;
    const long long count = (long long)s.K * s.C * 16;
    const long long stride = count + (fuse ? s.K : 0);
    int blocks = wgrad_k4s2p1_fewc_blocks(s);
    const long long room = (long long)(ws_bytes / 4) / stride;
    if (room < 1 || !ws) return GZ_ERR_WORKSPACE;
    if (blocks > room) blocks = (int)room;
    const int items = s.N * s.OH * (s.OW >> 4);
    const FastDiv dseg = make_fastdiv(s.OW >> 4), doh = make_fastdiv(s.OH);
#define GZ_FEWC(C_, KT_, F_)                                                                                         \
    hipLaunchKernelGGL((wgrad_k4s2p1_fewc_kernel<C_, KT_, F_>), dim3((unsigned)blocks), dim3(256), 0, st, x, y, fwd_out, \
                       ws, s.N, s.K, s.H, s.W, s.OH, s.OW, items, dseg, doh, act, slope, stride)
#define GZ_FEWC_C(KT_, F_)                                                                                           \
    switch (s.C) {                                                                                                   \
        case 1: GZ_FEWC(1, KT_, F_); break;                                                                          \
        case 2: GZ_FEWC(2, KT_, F_); break;                                                                          \
        case 3: GZ_FEWC(3, KT_, F_); break;                                                                          \
        default: GZ_FEWC(4, KT_, F_);                                                                                \
    }
#define GZ_FEWC_K(F_)                                                                                                \
    switch (s.K / 16) {                                                                                              \
        case 1: GZ_FEWC_C(1, F_); break;                                                                             \
        case 2: GZ_FEWC_C(2, F_); break;                                                                             \
        default: GZ_FEWC_C(4, F_);                                                                                   \
    }
    if (fuse) { GZ_FEWC_K(true) } else { GZ_FEWC_K(false) }
#undef GZ_FEWC_K
#undef GZ_FEWC_C
#undef GZ_FEWC
    int rc = launch_status();
    if (rc != GZ_OK) return rc;
    if (defer_reduce(blocks, stride)) return rc;
    if (fuse) return GZ_ERR_UNSUPPORTED;
    if (blocks <= 8) launch_reduce_few_slabs(ws, dw, blocks, count, st);
    else launch_reduce_slabs(ws, dw, blocks, count, count, nullptr, 0ll, st);
    return launch_status();
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_conv2d_wgrad_act_fuses(int N, int C, int H, int W, int K, int OH, int OW, int KH, int KW, int S, int P, int act) {
    ConvShape s{N, C, H, W, K, OH, OW};
    return shape_ok(s, KH, KW, S, P) && KH == 4 && KW == 4 && S == 2 && P == 1 && (act == ACT_RELU || act == ACT_LRELU) &&
                   !knobs().no_act_fuse && wgrad_k4s2p1_fewc_ok(s) ? 1 : 0;
}

int gz_conv2d_wgrad_act_partial(const float* x, const float* gy, const float* fwd_out, int act, float slope,
                                float* workspace, size_t ws_bytes, int N, int C, int H, int W, int K, int OH, int OW,
                                int KH, int KW, int S, int P, int* nz_out, long long* stride_out,
                                long long* bias_offset_out, hipStream_t stream) {
    gz::clear_stale_error();
    if (!nz_out || !stride_out || !bias_offset_out || !x || !gy || !fwd_out) return GZ_ERR_BAD_SHAPE;
    if (!gz_conv2d_wgrad_act_fuses(N, C, H, W, K, OH, OW, KH, KW, S, P, act)) return GZ_ERR_UNSUPPORTED;
    ConvShape s{N, C, H, W, K, OH, OW};
    if (too_large((long long)N * C * H * W) || too_large((long long)N * K * OH * OW)) return GZ_ERR_TOO_LARGE;
    WgDefer d{1, 0};
    tl_wg_defer = &d;
    const int rc = run_wgrad_k4s2p1_fewc(x, gy, fwd_out, act, slope, nullptr, workspace, ws_bytes, s, stream);
    tl_wg_defer = nullptr;
    *nz_out = d.nz;
    *stride_out = d.stride;
    *bias_offset_out = (long long)K * C * 16;
    return rc;
}

}  // extern "C"
