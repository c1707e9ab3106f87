// DiffAugment (Zhao et al. 2020) of the discriminator's input: brightness, saturation, contrast, integer translation
// with zero fill and a cutout box, per sample, as ONE launch each way.
//
//     y = A x + k,   A = Mask . Shift . Con . Sat,   k from the brightness alone
//     Sat = s I + (1 - s) P_channel,  Con = c I + (1 - c) P_all   (symmetric, commuting, both keep the sample mean)
//     A^T g = Con . Sat . Shift^T . Mask g
//
// mode 0: A x + k, mode 1: A x, mode 2: A^T x.  All three are the same walk: an output element (c, h, w) reads the
// source element (c, h + dh, w + dw) with the indices taken MODULO the image, dh/dw = +shift in modes 0/1 and -shift
// in mode 2.  The modular shift is a bijection of the sample, so one pass reads every input element exactly once --
// which is what the contrast mean needs, whatever the shift -- and the lane that ends up with a wrapped-around element
// knows that its output lies outside the shifted image.  Modes 0/1 zero such an element (and the cutout box, tested
// at the OUTPUT position) after the colour maps; mode 2 zeroes it (and the box, tested at the SOURCE position: the
// mask acts on g before the shift back) before the sum and the colour maps.
//
// One workgroup per sample; the sample stays in registers between the sum and the colour maps (3x64x64: 48 floats per
// lane at 256 lanes; 3x128x128: 48 floats per lane at 1024 lanes).  A lane owns units of 4 consecutive pixels of the
// flattened H*W plane in all C channels, so the channel mean of the saturation is lane-local and the store of a unit
// is one 16-byte store per channel wherever its address is 16-byte aligned.  The 4 source pixels of a unit are
// fetched by one 16-byte load where they are contiguous and aligned (shift a multiple of 4 columns), by dword loads
// otherwise: misaligned source columns are NOT re-placed through LDS.
//
// The mean is a fixed-order reduction -- per lane 4 running sums over at most 18 values each, 2 additions to join them,
// a 6-level butterfly per wave and a 4-level tree over the at most 16 waves: no atomics, equal bits on every run,
// longest chain of dependent additions 18 + 2 + 6 + 4 = 30.
#include "gz_common.h"
#include "../../include/gz_ops.h"

namespace gz {

constexpr int DA_MAX_THREADS = 1024;
constexpr int DA_MAX_ELEMS = 65536;

struct DiffAugArgs {
    const float* x0;
    const float* x1;
    const float* params;
    float* y;
    int R0, H, W, HW, cut_h, cut_w, mode;
    float inv_c, inv_l;
    FastDiv div_w;
};

// a float holding an integer -> int in [-lim, lim]; NaN becomes 0.  The shifts and the box corner come from device
// memory: whatever they hold, no index derived from them leaves the sample.
__device__ __forceinline__ int da_int(float v, int lim) {
    v = fminf(fmaxf(v, (float)-lim), (float)lim);
    return v == v ? (int)v : 0;
}

__device__ __forceinline__ float da_block_sum(float v, float* part) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) part[wave] = v;
    __syncthreads();
    float p[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) p[i] = i < nwaves ? part[i] : 0.f;
#pragma unroll
    for (int w = 8; w > 0; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) p[i] += p[i + w];
    return p[0];
}

template <int C, int NU>
__global__ __launch_bounds__(DA_MAX_THREADS) void diffaug_kernel(const DiffAugArgs a) {
    __shared__ float part[16];
    const int n = blockIdx.x;
    const int H = a.H, W = a.W, HW = a.HW, mode = a.mode;
    const size_t L = (size_t)C * HW;
    const float* __restrict__ src = n < a.R0 ? a.x0 + (size_t)n * L : a.x1 + (size_t)(n - a.R0) * L;
    float* __restrict__ dst = a.y + (size_t)n * L;
    const float* __restrict__ pr = a.params + (size_t)n * 8;
    const float b = mode == 0 ? pr[0] : 0.f, s = pr[1], cc = pr[2];
    int th = da_int(pr[3], H), tw = da_int(pr[4], W);
    const int h0 = da_int(pr[5], 1 << 20), w0 = da_int(pr[6], 1 << 20);
    const int h1 = h0 + a.cut_h, w1 = w0 + a.cut_w;
    if (mode == 2) { th = -th; tw = -tw; }
    int dhm = th % H, dwm = tw % W;          // the shift modulo the image, in [0, H) x [0, W)
    if (dhm < 0) dhm += H;
    if (dwm < 0) dwm += W;

    float v[NU][C][4];
    unsigned dead[NU];                        // bit j: element j of the unit is zeroed by the shift or the box
    float acc[4] = {0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int p0 = 4 * (u * (int)blockDim.x + (int)threadIdx.x);
        dead[u] = 0;
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[u][c][j] = 0.f;
        if (p0 >= HW) continue;
        int hh = (int)fdiv((uint32_t)p0, a.div_w), ww = p0 - hh * W;
        int off[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            off[j] = -1;
            if (p0 + j < HW) {
                int hs = hh + dhm, ws = ww + dwm;
                if (hs >= H) hs -= H;
                if (ws >= W) ws -= W;
                const bool wrapped = (unsigned)(hh + th) >= (unsigned)H || (unsigned)(ww + tw) >= (unsigned)W;
                const int ch = mode == 2 ? hs : hh, cw = mode == 2 ? ws : ww;      // where the box is tested
                const bool cut = ch >= h0 && ch < h1 && cw >= w0 && cw < w1;
                if (wrapped || cut) dead[u] |= 1u << j;
                off[j] = hs * W + ws;
            }
            if (++ww == W) { ww = 0; ++hh; }
        }
        const bool run = p0 + 4 <= HW && off[1] == off[0] + 1 && off[2] == off[0] + 2 && off[3] == off[0] + 3;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float* plane = src + (size_t)c * HW;
            if (run && (((uintptr_t)(plane + off[0])) & 15) == 0) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(plane + off[0]);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[u][c][j] = t[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (off[j] >= 0) v[u][c][j] = plane[off[j]];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (mode == 2 && ((dead[u] >> j) & 1u)) v[u][c][j] = 0.f;
                acc[j] += v[u][c][j];
            }
        }
    }

    const float total = da_block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), part);
    const float M = total * a.inv_l + b;

#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int p0 = 4 * (u * (int)blockDim.x + (int)threadIdx.x);
        if (p0 >= HW) continue;
        float o[C][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float m = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                v[u][c][j] += b;
                m += v[u][c][j];
            }
            m = C == 1 ? m : m * a.inv_c;
            const bool zero = mode != 2 && ((dead[u] >> j) & 1u);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float x2 = m + s * (v[u][c][j] - m);
                const float x3 = M + cc * (x2 - M);
                o[c][j] = zero ? 0.f : x3;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float* q = dst + (size_t)c * HW + p0;
            if (p0 + 4 <= HW && (((uintptr_t)q) & 15) == 0) {
                f32x4 t;
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = o[c][j];
                *reinterpret_cast<f32x4*>(q) = t;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (p0 + j < HW) q[j] = o[c][j];
            }
        }
    }
}

template <int C>
static int diffaug_launch(const DiffAugArgs& a, int R, int nu, int threads, hipStream_t stream) {
#define GZ_DA_CASE(NU)                                                                                       \
    if (nu <= NU) {                                                                                          \
        hipLaunchKernelGGL((diffaug_kernel<C, NU>), dim3(R), dim3(threads), 0, stream, a);                   \
        return launch_status();                                                                              \
    }
    GZ_DA_CASE(1)
    GZ_DA_CASE(2)
    GZ_DA_CASE(4)
    if constexpr (C == 3) { GZ_DA_CASE(6) }
    if constexpr (C <= 2) { GZ_DA_CASE(8) }
    if constexpr (C == 1) { GZ_DA_CASE(16) }
#undef GZ_DA_CASE
    return GZ_ERR_UNSUPPORTED;
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_diffaug(const float* x0, const float* x1, const float* params, float* y, int R0, int R1, int C, int H, int W,
               int cut_h, int cut_w, int mode, hipStream_t stream) {
    gz::clear_stale_error();
    if (!x0 || !params || !y || R0 < 0 || R1 < 0 || (long long)R0 + R1 < 1 || (long long)R0 + R1 > 0x7fffffffll)
        return GZ_ERR_BAD_SHAPE;
    if ((!x1 && R1 != 0) || mode < 0 || mode > 2 || C < 1 || H < 1 || W < 1 || cut_h < 0 || cut_w < 0)
        return GZ_ERR_BAD_SHAPE;
    if (C > 4 || H < 4 || W < 4 || (long long)C * H * W > DA_MAX_ELEMS) return GZ_ERR_UNSUPPORTED;
    const int R = R0 + R1;
    const uintptr_t row = (uintptr_t)C * H * W * 4;
    const uintptr_t yb = (uintptr_t)y, ye = yb + row * R;
    const uintptr_t s0 = (uintptr_t)x0, s1 = (uintptr_t)x1;
    if (R0 > 0 && yb < s0 + row * R0 && s0 < ye) return GZ_ERR_BAD_SHAPE;
    if (R1 > 0 && yb < s1 + row * R1 && s1 < ye) return GZ_ERR_BAD_SHAPE;

    DiffAugArgs a;
    a.x0 = x0, a.x1 = x1, a.params = params, a.y = y;
    a.R0 = R0, a.H = H, a.W = W, a.HW = H * W, a.cut_h = cut_h, a.cut_w = cut_w, a.mode = mode;
    a.inv_c = 1.0f / (float)C;
    a.inv_l = 1.0f / (float)(C * H * W);
    a.div_w = make_fastdiv((uint32_t)W);
    // the fewest lanes whose register share of the sample stays within 16 float4 (18 at C = 3)
    static const int cap[5] = {0, 16, 8, 6, 4};
    const int units = (H * W + 3) / 4;
    int threads = 256;
    while (threads < DA_MAX_THREADS && (units + threads - 1) / threads > cap[C]) threads *= 2;
    const int nu = (units + threads - 1) / threads;
    switch (C) {
        case 1: return diffaug_launch<1>(a, R, nu, threads, stream);
        case 2: return diffaug_launch<2>(a, R, nu, threads, stream);
        case 3: return diffaug_launch<3>(a, R, nu, threads, stream);
        default: return diffaug_launch<4>(a, R, nu, threads, stream);
    }
}

}  // extern "C"
