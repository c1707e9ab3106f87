// Figure frames (reference core/figures/types.py:137-167, 61-65, 109-116): F frames of n images each laid out as
// torchvision's make_grid does (ncol images per row, `padding` pixels of `pad_value` around every cell, empty cells
// left at the pad value, one image = the image itself without padding, 1 channel repeated to 3), clamped to [0, 1],
// multiplied by 255 in fp32 and truncated toward zero -- the array both the PNG and the GIF path encode -- written
// as uint8 [F][GH][GW][3] in one launch.
#include "gz_common.h"
#include "../../include/gz_ops.h"

namespace gz {

constexpr int FF_THREADS = 256;

struct FrameGeom {
    int n, C, H, W, xmaps, GH, GW, padding;
    float pad_value;
};

__device__ __forceinline__ unsigned char frame_byte(const float* __restrict__ img, const FrameGeom& g, long long e) {
    const int ch = (int)(e % 3);
    long long p = e / 3;
    const int gx = (int)(p % g.GW);
    p /= g.GW;
    const int gy = (int)(p % g.GH);
    const long long f = p / g.GH;
    float v = g.pad_value;
    int k, iy, ix;
    if (g.n == 1) {                        // make_grid returns a single image unpadded
        k = 0, iy = gy, ix = gx;
    } else {
        const int ch_ = g.H + g.padding, cw = g.W + g.padding;
        const int cy = gy / ch_, cx = gx / cw;
        iy = gy - cy * ch_ - g.padding, ix = gx - cx * cw - g.padding;
        k = cy * g.xmaps + cx;
        if (iy < 0 || ix < 0 || cx >= g.xmaps || k >= g.n) k = -1;
    }
    if (k >= 0) {
        const int c = g.C == 1 ? 0 : ch;
        v = img[(((f * g.n + k) * g.C + c) * g.H + iy) * (long long)g.W + ix];
    }
    v = fminf(fmaxf(v, 0.f), 1.f);          // torch.clamp(grid, 0, 1)
    return (unsigned char)(int)(v * 255.0f);  // (array * 255).astype(int / uint8): fp32 product, truncated
}

// one lane per 4 output bytes, one 32-bit store each (the last lane of an odd-sized output stores byte by byte)
__global__ __launch_bounds__(FF_THREADS) void figure_frames_kernel(const float* __restrict__ img,
                                                                   unsigned char* __restrict__ out, FrameGeom g,
                                                                   long long total) {
    const long long e0 = ((long long)blockIdx.x * FF_THREADS + threadIdx.x) * 4;
    if (e0 >= total) return;
    if (e0 + 4 <= total) {
        const unsigned w = (unsigned)frame_byte(img, g, e0) | ((unsigned)frame_byte(img, g, e0 + 1) << 8) |
                           ((unsigned)frame_byte(img, g, e0 + 2) << 16) | ((unsigned)frame_byte(img, g, e0 + 3) << 24);
        *reinterpret_cast<unsigned*>(out + e0) = w;
    } else {
        for (long long e = e0; e < total; ++e) out[e] = frame_byte(img, g, e);
    }
}

static bool frame_dims(int n, int H, int W, int ncol, int padding, int* gh_gw) {
    if (n <= 0 || H <= 0 || W <= 0 || ncol <= 0 || padding < 0) return false;
    if (n == 1) {
        gh_gw[0] = H, gh_gw[1] = W;
        return true;
    }
    const int xmaps = n < ncol ? n : ncol;
    const int ymaps = (n + xmaps - 1) / xmaps;
    gh_gw[0] = (H + padding) * ymaps + padding;
    gh_gw[1] = (W + padding) * xmaps + padding;
    return true;
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_figure_frames_u8(const float* img, unsigned char* out, int F, int n, int C, int H, int W, int ncol, int padding,
                        float pad_value, hipStream_t stream) {
    gz::clear_stale_error();
    int dims[2];
    if (F <= 0 || (C != 1 && C != 3) || !frame_dims(n, H, W, ncol, padding, dims)) return GZ_ERR_BAD_SHAPE;
    if ((((uintptr_t)out) & 3)) return GZ_ERR_BAD_SHAPE;
    FrameGeom g{n, C, H, W, n < ncol ? n : ncol, dims[0], dims[1], padding, pad_value};
    const long long total = (long long)F * dims[0] * dims[1] * 3;
    const long long lanes = (total + 3) / 4;
    hipLaunchKernelGGL(figure_frames_kernel, dim3((unsigned)((lanes + FF_THREADS - 1) / FF_THREADS)), dim3(FF_THREADS), 0,
                       stream, img, out, g, total);
    return launch_status();
}

}  // extern "C"
