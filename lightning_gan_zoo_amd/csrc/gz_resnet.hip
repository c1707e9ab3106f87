// HBM-bound pieces of the R1-regularised ResNet path: the pre-activation
// LeakyReLU, the residual combination `x_s + 0.1*dx`, AvgPool2d(3, stride 2, padding 1) and the
// nearest-neighbour 2x Upsample of reference core/submodules/gan_stability/models/resnet.py:30-33,
// 72-75,119-124,131-133.  All four are linear (or piecewise linear) maps, so each forward/backward
// pair below is also its own double-backward pair: the adjoint of the adjoint is the forward.
#include "gz_common.h"
#include "../../include/gz_ops.h"

namespace gz {

constexpr int RT = 256;

static int rn_grid(long long items) {
    long long b = (items + RT - 1) / RT;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (int)b;
}

__global__ __launch_bounds__(RT) void act_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                     long long total4, int act, float slope) {
    const long long stride = (long long)gridDim.x * RT;
    for (long long i = (long long)blockIdx.x * RT + threadIdx.x; i < total4; i += stride) {
        f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = act_fwd(v[q], act, slope);
        reinterpret_cast<f32x4*>(y)[i] = o;
    }
}

// out = alpha*a + beta*b  (b may be null: out = alpha*a); optionally act_out = act(out) in the same pass
__global__ __launch_bounds__(RT) void axpby_kernel(const float* __restrict__ a, float alpha,
                                                   const float* __restrict__ b, float beta,
                                                   float* __restrict__ out, float* __restrict__ act_out,
                                                   long long total4, int act, float slope) {
    const long long stride = (long long)gridDim.x * RT;
    for (long long i = (long long)blockIdx.x * RT + threadIdx.x; i < total4; i += stride) {
        f32x4 o = reinterpret_cast<const f32x4*>(a)[i] * alpha;
        if (b) o = o + reinterpret_cast<const f32x4*>(b)[i] * beta;
        reinterpret_cast<f32x4*>(out)[i] = o;
        if (act_out) {
            f32x4 t;
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] = act_fwd(o[q], act, slope);
            reinterpret_cast<f32x4*>(act_out)[i] = t;
        }
    }
}

// AvgPool2d(3, 2, 1), count_include_pad: y[oh][ow] = (1/9) * sum over the 3x3 window centred on (2oh, 2ow)
// with out-of-map taps contributing zero.  One thread per output element; the 3 rows it reads are shared with
// its neighbours through L1/L2.
__global__ __launch_bounds__(RT) void avgpool3s2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            long long total, int H, int W, int OH, int OW,
                                                            FastDiv div_ow, FastDiv div_oh) {
    const long long stride = (long long)gridDim.x * RT;
    for (long long i = (long long)blockIdx.x * RT + threadIdx.x; i < total; i += stride) {
        uint32_t t = fdiv((uint32_t)i, div_ow);
        int ow = (int)((uint32_t)i - t * (uint32_t)OW);
        uint32_t p = fdiv(t, div_oh);
        int oh = (int)(t - p * (uint32_t)OH);
        const float* src = x + (long long)p * H * W;
        float s = 0.f;
#pragma unroll
        for (int dh = -1; dh <= 1; ++dh) {
            int h = 2 * oh + dh;
            if (h < 0 || h >= H) continue;
#pragma unroll
            for (int dw = -1; dw <= 1; ++dw) {
                int w = 2 * ow + dw;
                if (w >= 0 && w < W) s += src[h * W + w];
            }
        }
        y[i] = s * (1.f / 9.f);
    }
}

// adjoint of the above: gx[h][w] = (1/9) * sum of gy over the (at most 2x2) windows that cover (h, w)
__global__ __launch_bounds__(RT) void avgpool3s2_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx,
                                                            long long total, int H, int W, int OH, int OW,
                                                            FastDiv div_w, FastDiv div_h) {
    const long long stride = (long long)gridDim.x * RT;
    for (long long i = (long long)blockIdx.x * RT + threadIdx.x; i < total; i += stride) {
        uint32_t t = fdiv((uint32_t)i, div_w);
        int w = (int)((uint32_t)i - t * (uint32_t)W);
        uint32_t p = fdiv(t, div_h);
        int h = (int)(t - p * (uint32_t)H);
        const float* src = gy + (long long)p * OH * OW;
        // windows centred on 2*o cover 2o-1..2o+1: an even coordinate has one covering window, an odd one two
        int oh0 = h >> 1, oh1 = (h & 1) ? oh0 + 1 : oh0;
        int ow0 = w >> 1, ow1 = (w & 1) ? ow0 + 1 : ow0;
        float s = 0.f;
        for (int oh = oh0; oh <= oh1; ++oh) {
            if (oh >= OH) continue;
            for (int ow = ow0; ow <= ow1; ++ow)
                if (ow < OW) s += src[oh * OW + ow];
        }
        gx[i] = s * (1.f / 9.f);
    }
}

// nn.Upsample(scale_factor=2), nearest: y[2h+a][2w+b] = x[h][w].  One thread per input element, two 8-byte stores.
__global__ __launch_bounds__(RT) void upsample2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           long long total, int W, FastDiv div_w) {
    const long long stride = (long long)gridDim.x * RT;
    for (long long i = (long long)blockIdx.x * RT + threadIdx.x; i < total; i += stride) {
        uint32_t row = fdiv((uint32_t)i, div_w);          // plane*H + h
        uint32_t w = (uint32_t)i - row * (uint32_t)W;
        float v = x[i];
        f32x2 vv = {v, v};
        float* dst = y + (long long)row * 4 * W + 2 * w;  // row (2*(plane*H+h)) of width 2W
        *reinterpret_cast<f32x2*>(dst) = vv;
        *reinterpret_cast<f32x2*>(dst + 2 * W) = vv;
    }
}

__global__ __launch_bounds__(RT) void upsample2_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx,
                                                           long long total, int W, FastDiv div_w) {
    const long long stride = (long long)gridDim.x * RT;
    for (long long i = (long long)blockIdx.x * RT + threadIdx.x; i < total; i += stride) {
        uint32_t row = fdiv((uint32_t)i, div_w);
        uint32_t w = (uint32_t)i - row * (uint32_t)W;
        const float* src = gy + (long long)row * 4 * W + 2 * w;
        f32x2 a = *reinterpret_cast<const f32x2*>(src);
        f32x2 b = *reinterpret_cast<const f32x2*>(src + 2 * W);
        gx[i] = (a.x + a.y) + (b.x + b.y);
    }
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_act_fwd(const float* x, float* y, long long count, int act, float slope, hipStream_t stream) {
    gz::clear_stale_error();
    if (count <= 0 || (count & 3)) return GZ_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(act_fwd_kernel, dim3(rn_grid(count / 4)), dim3(RT), 0, stream, x, y, count / 4, act, slope);
    return launch_status();
}

int gz_axpby(const float* a, float alpha, const float* b, float beta, float* out, float* act_out, long long count,
             int act, float slope, hipStream_t stream) {
    gz::clear_stale_error();
    if (count <= 0 || (count & 3)) return GZ_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(axpby_kernel, dim3(rn_grid(count / 4)), dim3(RT), 0, stream, a, alpha, b, beta, out, act_out,
                       count / 4, act, slope);
    return launch_status();
}

static int pool_shape_ok(long long planes, int H, int W, int OH, int OW) {
    if (planes <= 0 || H <= 0 || W <= 0) return 0;
    if (OH != (H - 1) / 2 + 1 || OW != (W - 1) / 2 + 1) return 0;
    return planes * H * W < (1ll << 31);
}

int gz_avgpool3s2_fwd(const float* x, float* y, long long planes, int H, int W, int OH, int OW,
                      hipStream_t stream) {
    gz::clear_stale_error();
    if (!pool_shape_ok(planes, H, W, OH, OW)) return GZ_ERR_BAD_SHAPE;
    long long total = planes * OH * OW;
    hipLaunchKernelGGL(avgpool3s2_fwd_kernel, dim3(rn_grid(total)), dim3(RT), 0, stream, x, y, total, H, W, OH, OW,
                       make_fastdiv(OW), make_fastdiv(OH));
    return launch_status();
}

int gz_avgpool3s2_bwd(const float* gy, float* gx, long long planes, int H, int W, int OH, int OW,
                      hipStream_t stream) {
    gz::clear_stale_error();
    if (!pool_shape_ok(planes, H, W, OH, OW)) return GZ_ERR_BAD_SHAPE;
    long long total = planes * H * W;
    hipLaunchKernelGGL(avgpool3s2_bwd_kernel, dim3(rn_grid(total)), dim3(RT), 0, stream, gy, gx, total, H, W, OH, OW,
                       make_fastdiv(W), make_fastdiv(H));
    return launch_status();
}

int gz_upsample2_fwd(const float* x, float* y, long long planes, int H, int W, hipStream_t stream) {
    gz::clear_stale_error();
    if (planes <= 0 || H <= 0 || W <= 0 || planes * H * W * 4 >= (1ll << 31)) return GZ_ERR_BAD_SHAPE;
    long long total = planes * H * W;
    hipLaunchKernelGGL(upsample2_fwd_kernel, dim3(rn_grid(total)), dim3(RT), 0, stream, x, y, total, W,
                       make_fastdiv(W));
    return launch_status();
}

int gz_upsample2_bwd(const float* gy, float* gx, long long planes, int H, int W, hipStream_t stream) {
    gz::clear_stale_error();
    if (planes <= 0 || H <= 0 || W <= 0 || planes * H * W * 4 >= (1ll << 31)) return GZ_ERR_BAD_SHAPE;
    long long total = planes * H * W;
    hipLaunchKernelGGL(upsample2_bwd_kernel, dim3(rn_grid(total)), dim3(RT), 0, stream, gy, gx, total, W,
                       make_fastdiv(W));
    return launch_status();
}

}  // extern "C"

// ---------------------------------------------------------------------------
// input step: decoded uint8 HWC images -> normalised float NCHW on the device, i.e.
// ToTensor() + Normalize(mean, std) of reference core/lightning_module.py:42-47 in one HBM pass (1 B read, 4 B
// written per element) instead of on the host.  One thread per output pixel, all channels.
// ---------------------------------------------------------------------------
namespace gz {
// (the one expression of the input step, u8_norm, lives in gz_common.h: gz_infer.hip's fused input kernel calls it too)
__global__ __launch_bounds__(256) void u8hwc_to_nchw_kernel(const unsigned char* __restrict__ in,
                                                            float* __restrict__ out, long long pixels, int HW, int C,
                                                            float scale, float shift, FastDiv div_hw) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += stride) {
        const uint32_t n = fdiv((uint32_t)p, div_hw);
        const uint32_t pix = (uint32_t)p - n * (uint32_t)HW;
        const unsigned char* src = in + p * C;
        float* dst = out + (long long)n * C * HW + pix;
        for (int c = 0; c < C; ++c) dst[(long long)c * HW] = u8_norm(src[c], scale, shift);
    }
}

// Resident training set: batch row i is row idx[i] of a uint8 [M, H, W, C] set that stays in HBM.  One thread takes
// PX consecutive pixels of one batch row with all their channels.  WIDE (PX = 4) needs H*W % 4 == 0 and aligned base
// pointers: then every row, and every group of 4 pixels in it, starts on a 4-byte boundary of the set and on a
// 16-byte boundary of each output plane, so a lane reads C dwords (lanes back to back: 4*C bytes each) and writes one
// float4 per plane (lanes back to back: 16 bytes each).  Otherwise (PX = 1; e.g. rows of 5*7*3 = 105 bytes) the
// accesses are byte loads and dword stores, the mapping of u8hwc_to_nchw_kernel.  The row's byte offset idx[i]*H*W*C
// is 64-bit.  An index outside [0, M) is never used as an address: its row is written as quiet NaN, its label as -1.
template <int C, bool WIDE>
__global__ __launch_bounds__(256) void u8hwc_gather_kernel(const unsigned char* __restrict__ set, long long M,
                                                           const long long* __restrict__ idx,
                                                           const long long* __restrict__ labels,
                                                           float* __restrict__ out, long long* __restrict__ labels_out,
                                                           long long items, int HW, int G, float scale, float shift,
                                                           FastDiv div_g) {
    constexpr int PX = WIDE ? 4 : 1;
    const long long stride = (long long)gridDim.x * 256;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < items; p += stride) {
        const uint32_t i = fdiv((uint32_t)p, div_g);
        const uint32_t g = (uint32_t)p - i * (uint32_t)G;
        const long long row = idx[i];
        const bool ok = row >= 0 && row < M;
        if (g == 0 && labels_out != nullptr) labels_out[i] = ok ? labels[row] : -1ll;
        float* dst = out + (long long)i * C * HW + (long long)g * PX;
        float v[C][PX];
        if (!ok) {
            for (int c = 0; c < C; ++c)
                for (int k = 0; k < PX; ++k) v[c][k] = __builtin_nanf("");
        } else {
            const unsigned char* src = set + row * ((long long)HW * C) + (long long)g * (PX * C);
            if constexpr (WIDE) {
                uint32_t w[C];
                for (int j = 0; j < C; ++j) w[j] = reinterpret_cast<const uint32_t*>(src)[j];
                for (int k = 0; k < PX; ++k)
                    for (int c = 0; c < C; ++c) {
                        const int b = k * C + c;
                        v[c][k] = u8_norm((unsigned char)((w[b >> 2] >> (8 * (b & 3))) & 0xffu), scale, shift);
                    }
            } else {
                for (int c = 0; c < C; ++c) v[c][0] = u8_norm(src[c], scale, shift);
            }
        }
        for (int c = 0; c < C; ++c) {
            if constexpr (WIDE) {
                f32x4 q = {v[c][0], v[c][1], v[c][2], v[c][3]};
                *reinterpret_cast<f32x4*>(dst + (long long)c * HW) = q;
            } else {
                dst[(long long)c * HW] = v[c][0];
            }
        }
    }
}

template <int C>
static void launch_u8hwc_gather(bool wide, int grid, hipStream_t stream, const unsigned char* set, long long M,
                                const long long* idx, const long long* labels, float* out, long long* labels_out,
                                long long items, int HW, int G, float scale, float shift) {
    if (wide)
        hipLaunchKernelGGL((u8hwc_gather_kernel<C, true>), dim3(grid), dim3(256), 0, stream, set, M, idx, labels, out,
                           labels_out, items, HW, G, scale, shift, make_fastdiv(G));
    else
        hipLaunchKernelGGL((u8hwc_gather_kernel<C, false>), dim3(grid), dim3(256), 0, stream, set, M, idx, labels, out,
                           labels_out, items, HW, G, scale, shift, make_fastdiv(G));
}
}  // namespace gz

extern "C" int gz_u8hwc_to_nchw(const unsigned char* in, float* out, int N, int H, int W, int C, float mean, float std,
                                hipStream_t stream) {
    gz::clear_stale_error();
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 4 || std == 0.f) return GZ_ERR_BAD_SHAPE;
    const long long pixels = (long long)N * H * W;
    if (pixels >= (1ll << 31)) return GZ_ERR_TOO_LARGE;
    // (x / 255 - mean) / std  =  x * (1 / (255 std)) - mean / std
    hipLaunchKernelGGL(gz::u8hwc_to_nchw_kernel, dim3(gz::rn_grid(pixels)), dim3(256), 0, stream, in, out, pixels, H * W,
                       C, 1.f / (255.f * std), -mean / std, gz::make_fastdiv(H * W));
    return gz::launch_status();
}

extern "C" int gz_u8hwc_gather_to_nchw(const unsigned char* set, long long M, const long long* idx,
                                       const long long* labels, float* out, long long* labels_out, int n, int H, int W,
                                       int C, float mean, float std, hipStream_t stream) {
    gz::clear_stale_error();
    if (M <= 0 || n <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 4 || std == 0.f) return GZ_ERR_BAD_SHAPE;
    if (set == nullptr || idx == nullptr || out == nullptr) return GZ_ERR_BAD_SHAPE;
    const long long pixels = (long long)n * H * W;
    if (pixels >= (1ll << 31)) return GZ_ERR_TOO_LARGE;
    const int HW = H * W;
    const bool wide = HW % 4 == 0 && (uintptr_t)set % 4 == 0 && (uintptr_t)out % 16 == 0;
    const int G = wide ? HW / 4 : HW;
    const long long items = (long long)n * G;
    if (labels == nullptr) labels_out = nullptr;
    const float scale = 1.f / (255.f * std), shift = -mean / std;      // as gz_u8hwc_to_nchw
    const int grid = gz::rn_grid(items);
    switch (C) {
        case 1: gz::launch_u8hwc_gather<1>(wide, grid, stream, set, M, idx, labels, out, labels_out, items, HW, G, scale, shift); break;
        case 2: gz::launch_u8hwc_gather<2>(wide, grid, stream, set, M, idx, labels, out, labels_out, items, HW, G, scale, shift); break;
        case 3: gz::launch_u8hwc_gather<3>(wide, grid, stream, set, M, idx, labels, out, labels_out, items, HW, G, scale, shift); break;
        default: gz::launch_u8hwc_gather<4>(wide, grid, stream, set, M, idx, labels, out, labels_out, items, HW, G, scale, shift); break;
    }
    return gz::launch_status();
}
