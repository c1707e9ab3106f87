// Adaptive discriminator augmentation (Karras et al. 2020) on the DiffAugment launch: gz_diffaug (gz_diffaug.hip, left as
// it is) with a gate per sample and group, the two pixel-blitting transforms x-flip and rot90, and the controller that
// moves the gate probability p from r_t = E[sign(D(real))] without the host reading anything.
//
//     y = A' x + k,   A' = Mask . Shift . Q . Con . Sat,   Q x = rot90(flip_w(x) if f else x, k)
//     Q is a permutation (Q^T = Q^-1) that commutes with Con . Sat: the channel mean is per pixel, the sample mean is
//     invariant.                  A'^T g = Con . Sat . Q^T . Shift^T . Mask g = Q^T . Con . Sat . Shift^T . Mask g
//
// The walk of gz_diffaug stays: one workgroup per sample, a lane owns units of 4 consecutive pixels in all C channels,
// the sample rests in registers between the fixed-order sum and the colour maps.  The orientation of a sample is
// workgroup-uniform and decides between two routes:
//
//   k even (o in {0, 2, 4, 6}: identity, rot180, flip_w, flip_h; all involutions that keep rows rows).  Q is folded into
//     the source offset of the lane's unit: modes 0/1 map the shifted position through Q, mode 2 maps the output position
//     through Q before the shift.  A unit's 4 sources are a forward or a REVERSED run of one source row, fetched by one
//     16-byte load where aligned; a wave still reads whole rows.  No LDS.
//   k odd (transposing).  A lane that computed its sources as above would read 4 rows, a wave 64 rows.  Instead the
//     lanes load in row order (modes 0/1: the source as it lies; mode 2: the masked, shifted-back g exactly as
//     gz_diffaug mode 2 loads it), sum, colour in place -- Con . Sat commute with Q -- and then, one channel plane at
//     a time, write each element to its permuted position in an LDS plane (ds_write_b32), barrier, read the plane
//     back in output order (modes 0/1: at the shifted position, zero where the shift or the box kills it; mode 2: as
//     it lies) and store 16 bytes per unit.  Global memory sees row-contiguous runs on both sides.
//
// The LDS plane: row r starts at r (W + 1) + (r >> 5) floats.  ds_write_b32 / ds_read_b32 bank on (a / 4) mod 32 per
// half wave.  The transposing side is the write: the 32 lanes of a half hold source columns 4 l + j, which become plane
// rows 4 l + j (or their mirror), so instruction j writes addresses 4 l (W + 1) + (l >> 3) + const = 4 l + (l >> 3) (mod
// 32, W a multiple of 32): 32 different banks.  (Pitch W: one bank.  Pitch W + 1 alone: 4 l, 8 banks, 4-way.)  At W = 64
// a half wave spans two source rows and is 2-way, which a ds_write_b32 hides.  The read-back side walks rows: lane l
// reads dwords 4 l + j, 8 banks per instruction, 4-way (8 LDS cycles instead of 2 per wave instruction) -- inherent to
// 4 consecutive dwords per lane read as dwords, and the row starts are not 16-byte aligned for a ds_read_b128.  Per
// sample of 3x128x128 that is 768 wave instructions each way, ~10^4 LDS cycles against ~6 * 10^4 cycles of the CU's
// share of HBM traffic for the same sample; DESIGN.md 3.5.5 has the measured classes.
// 128 x 129 + 4 floats = 66064 bytes, above the 64 KB a launch gets by default: the launcher raises the kernel's
// dynamic-LDS limit (hipFuncSetAttribute) when the plane needs it.  Launches that cannot turn (blit bit 1 clear) use the
// instantiation without the staged route and without LDS.
//
// The mean is the reduction of gz_diffaug, unchanged: longest chain of dependent additions 18 + 2 + 6 + 4 = 30, a tree of
// 10 levels, so the bound of DESIGN.md 3.5.4 holds as it stands.
#include "gz_common.h"
#include "../../include/gz_ops.h"

namespace gz {

constexpr int ADA_MAX_THREADS = 1024;
constexpr int ADA_MAX_ELEMS = 65536;
constexpr int ADA_MAX_TURN_SIDE = 128;

struct AdaArgs {
    const float* x0;
    const float* x1;
    const float* params;
    const float* p;
    float* y;
    int R0, H, W, HW, cut_h, cut_w, mode, blit;
    float inv_c, inv_l;
    FastDiv div_w;
};

// a float holding an integer -> int in [lo, hi]; NaN becomes 0 (0 lies in every range used).  Shifts, box corner and
// orientation code come from device memory: whatever they hold, no index derived from them leaves the sample.
__device__ __forceinline__ int ada_int(float v, int lo, int hi) {
    v = fminf(fmaxf(v, (float)lo), (float)hi);
    return v == v ? (int)v : 0;
}

__device__ __forceinline__ float ada_block_sum(float v, float* part) {
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

// (Q x)[h, w] = x[ada_map(o, h, w)] for the orientation code o = k + 4 f.  k odd only ever runs with H == W.
__device__ __forceinline__ void ada_map(int o, int H, int W, int& h, int& w) {
    const int a = h, b = w;
    switch (o & 3) {
        case 1: h = b, w = H - 1 - a; break;
        case 2: h = H - 1 - a, w = W - 1 - b; break;
        case 3: h = W - 1 - b, w = a; break;
        default: break;
    }
    if (o & 4) w = W - 1 - w;
}

// the inverse permutation's code: rot90 and rot270 swap, the six others are involutions
__device__ __forceinline__ int ada_inverse(int o) { return o == 1 ? 3 : o == 3 ? 1 : o; }

struct AdaWalk {
    int H, W, th, tw, dhm, dwm, h0, h1, w0, w1;
};

// The 4 pixels p0 .. p0 + 3 of a unit (row hh, column ww at p0): each is mapped through `pre`, shifted by the walk
// modulo the image, tested against the shift's wrap and the box (at the shifted position if `box_at_src`, else at the
// unshifted one), mapped through `post`, and returned as h * pitch + (h >> skew) + w; -1 beyond the plane.
__device__ __forceinline__ unsigned ada_unit(const AdaWalk& k, int p0, int HW, int hh, int ww, int pre, int post,
                                             bool box_at_src, int pitch, int skew, int (&off)[4]) {
    unsigned dead = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        off[j] = -1;
        if (p0 + j < HW) {
            int h = hh, w = ww;
            ada_map(pre, k.H, k.W, h, w);
            int hs = h + k.dhm, ws = w + k.dwm;
            if (hs >= k.H) hs -= k.H;
            if (ws >= k.W) ws -= k.W;
            const bool wrapped = (unsigned)(h + k.th) >= (unsigned)k.H || (unsigned)(w + k.tw) >= (unsigned)k.W;
            const int ch = box_at_src ? hs : h, cw = box_at_src ? ws : w;
            const bool cut = ch >= k.h0 && ch < k.h1 && cw >= k.w0 && cw < k.w1;
            if (wrapped || cut) dead |= 1u << j;
            ada_map(post, k.H, k.W, hs, ws);
            off[j] = hs * pitch + (hs >> skew) + ws;
        }
        if (++ww == k.W) { ww = 0; ++hh; }
    }
    return dead;
}

constexpr int ADA_NOSKEW = 31;      // h >> 31 == 0 for h >= 0
constexpr int ADA_SKEW = 5;

template <int C, int NU, bool TURNS>
__global__ __launch_bounds__(ADA_MAX_THREADS) void ada_diffaug_kernel(const AdaArgs a) {
    __shared__ float part[16];
    extern __shared__ float plane[];          // TURNS only: H (W + 1) + (H >> 5) floats
    const int n = blockIdx.x;
    const int H = a.H, W = a.W, HW = a.HW, mode = a.mode;
    const size_t L = (size_t)C * HW;
    const float* __restrict__ src = n < a.R0 ? a.x0 + (size_t)n * L : a.x1 + (size_t)(n - a.R0) * L;
    float* __restrict__ dst = a.y + (size_t)n * L;
    const float* __restrict__ pr = a.params + (size_t)n * 16;

    const bool all = a.p == nullptr;
    const float pv = all ? 0.f : a.p[0];
    const bool on_color = all || pr[8] < pv, on_shift = all || pr[9] < pv, on_cut = all || pr[10] < pv;
    const bool on_flip = (a.blit & 1) && (all || pr[11] < pv), on_rot = (a.blit & 2) && (all || pr[12] < pv);

    const float b = mode == 0 && on_color ? pr[0] : 0.f, s = pr[1], cc = pr[2];
    int th = on_shift ? ada_int(pr[3], -H, H) : 0, tw = on_shift ? ada_int(pr[4], -W, W) : 0;
    const int h0 = ada_int(pr[5], -(1 << 20), 1 << 20), w0 = ada_int(pr[6], -(1 << 20), 1 << 20);
    const int code = ada_int(pr[7], 0, 7);
    const int o = (on_flip ? code & 4 : 0) | (on_rot ? code & 3 : 0);
    const bool turn = TURNS && (o & 1);
    if (mode == 2) { th = -th; tw = -tw; }
    int dhm = th % H, dwm = tw % W;          // the shift modulo the image, in [0, H) x [0, W)
    if (dhm < 0) dhm += H;
    if (dwm < 0) dwm += W;
    const AdaWalk shifted = {H, W, th, tw, dhm, dwm, h0, h0 + (on_cut ? a.cut_h : 0), w0, w0 + (on_cut ? a.cut_w : 0)};
    const AdaWalk still = {H, W, 0, 0, 0, 0, 0, 0, 0, 0};
    // the load: a turning sample loads in row order (modes 0/1 as the source lies, mode 2 shifted back and masked),
    // every other folds Q into the offsets -- mode 2 before the shift, modes 0/1 after it
    const bool load_still = turn && mode != 2;
    const int load_pre = turn ? 0 : mode == 2 ? o : 0, load_post = turn ? 0 : mode == 2 ? 0 : o;

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
        const int hh = (int)fdiv((uint32_t)p0, a.div_w), ww = p0 - hh * W;
        int off[4];
        dead[u] = ada_unit(load_still ? still : shifted, p0, HW, hh, ww, load_pre, load_post, mode == 2, W, ADA_NOSKEW,
                           off);
        const bool full = p0 + 4 <= HW;
        const bool fwd = full && off[1] == off[0] + 1 && off[2] == off[0] + 2 && off[3] == off[0] + 3;
        const bool rev = full && off[1] == off[0] - 1 && off[2] == off[0] - 2 && off[3] == off[0] - 3;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float* pl = src + (size_t)c * HW;
            if (fwd && (((uintptr_t)(pl + off[0])) & 15) == 0) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(pl + off[0]);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[u][c][j] = t[j];
            } else if (rev && (((uintptr_t)(pl + off[3])) & 15) == 0) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(pl + off[3]);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[u][c][j] = t[3 - j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (off[j] >= 0) v[u][c][j] = pl[off[j]];
            }
            if (mode == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((dead[u] >> j) & 1u) v[u][c][j] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += v[u][c][j];
        }
    }

    if (on_color) {                           // workgroup-uniform: a sample with colour off does no colour arithmetic
        const float total = ada_block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), part);
        const float M = total * a.inv_l + b;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float m = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    v[u][c][j] += b;
                    m += v[u][c][j];
                }
                m = C == 1 ? m : m * a.inv_c;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float x2 = m + s * (v[u][c][j] - m);
                    v[u][c][j] = M + cc * (x2 - M);
                }
            }
        }
    }
    if (mode != 2) {                          // (a turning sample has no dead bits yet: its mask acts at the read-back)
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((dead[u] >> j) & 1u) v[u][c][j] = 0.f;
    }

    if constexpr (TURNS) {
        if (turn) {
            // modes 0/1: source position r holds (Q x) at Q^-1's image of r; mode 2: (Q^T z)[map(r)] = z[r]
            const int put = mode == 2 ? o : ada_inverse(o);
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int p0 = 4 * (u * (int)blockDim.x + (int)threadIdx.x);
                    if (p0 >= HW) continue;
                    const int hh = (int)fdiv((uint32_t)p0, a.div_w), ww = p0 - hh * W;
                    int off[4];
                    ada_unit(still, p0, HW, hh, ww, put, 0, false, W + 1, ADA_SKEW, off);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (off[j] >= 0) plane[off[j]] = v[u][c][j];
                }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int p0 = 4 * (u * (int)blockDim.x + (int)threadIdx.x);
                    if (p0 >= HW) continue;
                    const int hh = (int)fdiv((uint32_t)p0, a.div_w), ww = p0 - hh * W;
                    int off[4];
                    const unsigned gone = ada_unit(mode == 2 ? still : shifted, p0, HW, hh, ww, 0, 0, false, W + 1,
                                                   ADA_SKEW, off);
                    float t[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) t[j] = off[j] >= 0 && !((gone >> j) & 1u) ? plane[off[j]] : 0.f;
                    float* q = dst + (size_t)c * HW + p0;
                    if (p0 + 4 <= HW && (((uintptr_t)q) & 15) == 0) {
                        f32x4 t4;
#pragma unroll
                        for (int j = 0; j < 4; ++j) t4[j] = t[j];
                        *reinterpret_cast<f32x4*>(q) = t4;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (p0 + j < HW) q[j] = t[j];
                    }
                }
                __syncthreads();
            }
            return;
        }
    }

#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int p0 = 4 * (u * (int)blockDim.x + (int)threadIdx.x);
        if (p0 >= HW) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float* q = dst + (size_t)c * HW + p0;
            if (p0 + 4 <= HW && (((uintptr_t)q) & 15) == 0) {
                f32x4 t;
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = v[u][c][j];
                *reinterpret_cast<f32x4*>(q) = t;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (p0 + j < HW) q[j] = v[u][c][j];
            }
        }
    }
}

template <int C, int NU, bool TURNS>
static int ada_launch_one(const AdaArgs& a, int R, int threads, size_t lds, hipStream_t stream) {
    if (lds > 65536 - 64) {                   // beyond the default limit of a launch: part[] is static, the plane dynamic
        const int rc = hip_status(hipFuncSetAttribute(reinterpret_cast<const void*>(&ada_diffaug_kernel<C, NU, TURNS>),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (rc != GZ_OK) return rc;
    }
    hipLaunchKernelGGL((ada_diffaug_kernel<C, NU, TURNS>), dim3(R), dim3(threads), lds, stream, a);
    return launch_status();
}

template <int C>
static int ada_launch(const AdaArgs& a, int R, int nu, int threads, size_t lds, hipStream_t stream) {
#define GZ_ADA_CASE(NU)                                                                                      \
    if (nu <= NU)                                                                                            \
        return lds ? ada_launch_one<C, NU, true>(a, R, threads, lds, stream)                                 \
                   : ada_launch_one<C, NU, false>(a, R, threads, 0, stream);
    GZ_ADA_CASE(1)
    GZ_ADA_CASE(2)
    GZ_ADA_CASE(4)
    if constexpr (C == 3) { GZ_ADA_CASE(6) }
    if constexpr (C <= 2) { GZ_ADA_CASE(8) }
    if constexpr (C == 1) { GZ_ADA_CASE(16) }
#undef GZ_ADA_CASE
    return GZ_ERR_UNSUPPORTED;
}

// ---- the controller: state = {sum_sign, count, p, last_r} ------------------------------------------------------------
constexpr int ADA_OBS_THREADS = 256;

__global__ __launch_bounds__(ADA_OBS_THREADS) void ada_observe_kernel(const float* __restrict__ logits, int n,
                                                                      float* __restrict__ state) {
    __shared__ float part[ADA_OBS_THREADS / 64];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += ADA_OBS_THREADS) {
        const float x = logits[i];
        s += (float)((int)(x > 0.f) - (int)(x < 0.f));        // NaN and +-0: 0
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        state[0] += (part[0] + part[1]) + (part[2] + part[3]);
        state[1] += (float)n;
    }
}

__global__ void ada_update_kernel(float* __restrict__ state, float target, float step) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float count = state[1];
    if (!(count > 0.f)) return;
    const float r = state[0] / count;
    const float d = r - target;
    const float sg = (float)((int)(d > 0.f) - (int)(d < 0.f));
    state[2] = fminf(fmaxf(state[2] + step * sg, 0.f), 1.f);
    state[3] = r;
    state[0] = 0.f;
    state[1] = 0.f;
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_diffaug_gated(const float* x0, const float* x1, const float* params, const float* p, float* y, int R0, int R1,
                     int C, int H, int W, int cut_h, int cut_w, int blit, int mode, hipStream_t stream) {
    gz::clear_stale_error();
    if (!x0 || !params || !y || R0 < 0 || R1 < 0 || (long long)R0 + R1 < 1 || (long long)R0 + R1 > 0x7fffffffll)
        return GZ_ERR_BAD_SHAPE;
    if ((!x1 && R1 != 0) || mode < 0 || mode > 2 || C < 1 || H < 1 || W < 1 || cut_h < 0 || cut_w < 0)
        return GZ_ERR_BAD_SHAPE;
    if (blit < 0 || blit > 3) return GZ_ERR_BAD_SHAPE;
    if (C > 4 || H < 4 || W < 4 || (long long)C * H * W > ADA_MAX_ELEMS) return GZ_ERR_UNSUPPORTED;
    if ((blit & 2) && (H != W || H > ADA_MAX_TURN_SIDE)) return GZ_ERR_UNSUPPORTED;
    const int R = R0 + R1;
    const uintptr_t row = (uintptr_t)C * H * W * 4;
    const uintptr_t yb = (uintptr_t)y, ye = yb + row * R;
    const uintptr_t s0 = (uintptr_t)x0, s1 = (uintptr_t)x1;
    if (R0 > 0 && yb < s0 + row * R0 && s0 < ye) return GZ_ERR_BAD_SHAPE;
    if (R1 > 0 && yb < s1 + row * R1 && s1 < ye) return GZ_ERR_BAD_SHAPE;

    AdaArgs a;
    a.x0 = x0, a.x1 = x1, a.params = params, a.p = p, a.y = y;
    a.R0 = R0, a.H = H, a.W = W, a.HW = H * W, a.cut_h = cut_h, a.cut_w = cut_w, a.mode = mode, a.blit = blit;
    a.inv_c = 1.0f / (float)C;
    a.inv_l = 1.0f / (float)(C * H * W);
    a.div_w = make_fastdiv((uint32_t)W);
    // the fewest lanes whose register share of the sample stays within 16 float4 (18 at C = 3), as gz_diffaug
    static const int cap[5] = {0, 16, 8, 6, 4};
    const int units = (H * W + 3) / 4;
    int threads = 256;
    while (threads < ADA_MAX_THREADS && (units + threads - 1) / threads > cap[C]) threads *= 2;
    const int nu = (units + threads - 1) / threads;
    const size_t lds = (blit & 2) ? sizeof(float) * ((size_t)H * (W + 1) + (H >> 5)) : 0;
    switch (C) {
        case 1: return ada_launch<1>(a, R, nu, threads, lds, stream);
        case 2: return ada_launch<2>(a, R, nu, threads, lds, stream);
        case 3: return ada_launch<3>(a, R, nu, threads, lds, stream);
        default: return ada_launch<4>(a, R, nu, threads, lds, stream);
    }
}

int gz_ada_observe(const float* logits, int n, float* state, hipStream_t stream) {
    gz::clear_stale_error();
    if (!logits || !state || n < 1) return GZ_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(ada_observe_kernel, dim3(1), dim3(ADA_OBS_THREADS), 0, stream, logits, n, state);
    return launch_status();
}

int gz_ada_update(float* state, float target, float step, hipStream_t stream) {
    gz::clear_stale_error();
    if (!state || !(step >= 0.f) || !(step <= 3.4028234e38f) || !(target >= -3.4028234e38f && target <= 3.4028234e38f))
        return GZ_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(ada_update_kernel, dim3(1), dim3(64), 0, stream, state, target, step);
    return launch_status();
}

}  // extern "C"
