// What runs around the convolution launches of a step, on their weights: the packers that turn a weight tensor into
// the [k][mn] images the launchers of gz_conv_{fwd,dgrad,wgrad}.hip / gz_conv_direct.hip read (gz_conv2d_pack_*; the layout rules both
// sides must agree on are in gz_pack_layout.h), and the sums of the weight-gradient slabs a split launch leaves behind
// (launch_reduce_*: per launch; gz_reduce_multi: one launch for many gradients).  No kernel here uses the implicit-GEMM
// skeletons.
#include "gz_pack_layout.h"
#include "gz_reduce.h"
#include "../../include/gz_ops.h"

namespace gz {

// The pack kernels exist twice: as their own launches (bx / by / gx = blockIdx / gridDim) and as the bodies of
// pack_multi_kernel, which re-packs every weight of a network in one launch (a job table maps a block to its tensor).
// dst[c][ld] (c < COLS) = src[r][c] transposed: dst[c*ld + r] = src[r*COLS + c]; zero for r in [R, ld)
__device__ __forceinline__ void transpose_pad_body(const float* __restrict__ src, float* __restrict__ dst, int R,
                                                   int COLS, int ld, int bx, int by, float scale = 1.f) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int c0 = bx * 32, r0 = by * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int r = r0 + ty + 8 * i, c = c0 + tx;
        tile[ty + 8 * i][tx] = (r < R && c < COLS) ? src[(long long)r * COLS + c] * scale : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = c0 + ty + 8 * i, r = r0 + tx;
        if (c < COLS && r < ld) dst[(long long)c * ld + r] = tile[tx][ty + 8 * i];
    }
}

__global__ __launch_bounds__(256) void transpose_pad_kernel(const float* __restrict__ src,
                                                            float* __restrict__ dst, int R, int COLS, int ld) {
    transpose_pad_body(src, dst, R, COLS, ld, blockIdx.x, blockIdx.y);
}

// wp[(tap, c)][ld] = w[ko][c][tap], c padded to a multiple of BK with zero rows
__device__ __forceinline__ void pack_fwd_tap_body(const float* __restrict__ w, float* __restrict__ wp, int K, int C,
                                                  int taps, int cpad, int ld, int bx, int gx, float scale = 1.f) {
    const long long total = (long long)taps * cpad * ld;
    for (long long i = (long long)bx * 256 + threadIdx.x; i < total; i += (long long)gx * 256) {
        int ko = (int)(i % ld);
        long long row = i / ld;
        int c = (int)(row % cpad), tap = (int)(row / cpad);
        wp[i] = (ko < K && c < C) ? w[((long long)ko * C + c) * taps + tap] * scale : 0.f;
    }
}

__global__ __launch_bounds__(256) void pack_fwd_tap_kernel(const float* __restrict__ w, float* __restrict__ wp, int K,
                                                           int C, int taps, int cpad, int ld) {
    pack_fwd_tap_body(w, wp, K, C, taps, cpad, ld, blockIdx.x, gridDim.x);
}

// wp[phase][(tap, ko)][ldc] = w[ko][c][ky][kx] over the phase's own ny x nx taps (tap = ty * nx + tx), ko padded
// to a multiple of BK; the unused tail of the phase's fixed-size TY*TX*kpad-row region is never read
__device__ __forceinline__ void pack_dgrad_tap_body(const float* __restrict__ w, float* __restrict__ wp, int K, int C,
                                                    int KH, int KW, int S, int P, int TY, int TX, int kpad, int ldc,
                                                    int bx, int phase, int gx, float scale = 1.f) {
    const int py = phase / S, px = phase % S;
    const int ry = (py + P) % S, rx = (px + P) % S;
    const int ny = dg_taps(KH, S, P, py), nx = dg_taps(KW, S, P, px);
    float* dst = wp + (long long)phase * TY * TX * kpad * ldc;
    const long long total = (long long)ny * nx * kpad * ldc;
    for (long long i = (long long)bx * 256 + threadIdx.x; i < total; i += (long long)gx * 256) {
        int c = (int)(i % ldc);
        long long row = i / ldc;
        int ko = (int)(row % kpad), tap = (int)(row / kpad);
        int ky = ry + S * (tap / nx), kx = rx + S * (tap % nx);
        dst[i] = (ko < K && c < C) ? w[(((long long)ko * C + c) * KH + ky) * KW + kx] * scale : 0.f;
    }
}

__global__ __launch_bounds__(256) void pack_dgrad_tap_kernel(const float* __restrict__ w, float* __restrict__ wp, int K,
                                                             int C, int KH, int KW, int S, int P, int TY, int TX,
                                                             int kpad, int ldc) {
    pack_dgrad_tap_body(w, wp, K, C, KH, KW, S, P, TY, TX, kpad, ldc, blockIdx.x, blockIdx.y, gridDim.x);
}

// dgrad pack: wp[phase][(ko, ty, tx)][ldc] = w[ko][c][ky][kx], ky = ((py+P)%S) + S*ty.  A phase only has the taps
// whose ky < KH (kx < KW): ny(py) * nx(px) of them (dg_taps); its rows are packed tightly and the rest of the
// phase's fixed-size K*TY*TX-row region is zero.  (k5 s2: 9/6/6/4 taps instead of 4 x 9.)
__device__ __forceinline__ void pack_dgrad_body(const float* __restrict__ w, float* __restrict__ wp, int K, int C,
                                                int KH, int KW, int S, int P, int TY, int TX, int ldc, int ko,
                                                int phase, float scale = 1.f) {
    const int py = phase / S, px = phase % S;
    const int ry = (py + P) % S, rx = (px + P) % S;
    const int ny = dg_taps(KH, S, P, py), nx = dg_taps(KW, S, P, px);
    const int taps = ny * nx, pad = TY * TX - taps;
    float* dst = wp + (long long)phase * K * TY * TX * ldc;
    for (int i = threadIdx.x; i < taps * ldc; i += 256) {
        int tap = i / ldc, c = i - tap * ldc;
        int ky = ry + S * (tap / nx), kx = rx + S * (tap % nx);
        dst[((long long)ko * taps + tap) * ldc + c] =
            c < C ? w[(((long long)ko * C + c) * KH + ky) * KW + kx] * scale : 0.f;
    }
    for (int i = threadIdx.x; i < pad * ldc; i += 256)
        dst[((long long)K * taps + (long long)ko * pad) * ldc + i] = 0.f;
}

// The k4 s2 p1 case of the same image (every DCGAN layer), one workgroup per ko and ALL four phases (round 5): the body
// above reads w[ko][c][ky][kx] along c -- a 64-byte stride, one 64-byte segment per lane and load -- once per phase.
// Here the C x 16 values of the ko are read once, contiguously (16-byte loads), turned in LDS 64 channels at a time,
// and leave as the sixteen (phase, tap) rows with 16-byte stores.  Same bytes out, bit for bit.
__device__ __forceinline__ void pack_dgrad_k4_body(const float* __restrict__ w, float* __restrict__ wp, int K, int C,
                                                   int ldc, int ko, float scale = 1.f) {
    __shared__ float tile[64][17];
    const int t = threadIdx.x;
    const int r = t >> 4, cs = (t & 15) * 4;                  // output row (ky, kx) and channel quad of this thread
    const int ky = r >> 2, kx = r & 3;
    const int phase = ((ky + 1) & 1) * 2 + ((kx + 1) & 1), tap = (ky >> 1) * 2 + (kx >> 1);
    float* dst = wp + (((long long)phase * K + ko) * 4 + tap) * ldc;
    const float* src = w + (long long)ko * C * 16;
    for (int c0 = 0; c0 < ldc; c0 += 64) {
        const int c = c0 + (t >> 2), e = (t & 3) * 4;         // this thread's 4 consecutive (ky, kx) values of channel c
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c < C) v = *reinterpret_cast<const f32x4*>(src + (long long)c * 16 + e);
        __syncthreads();
        tile[t >> 2][e + 0] = v.x * scale;
        tile[t >> 2][e + 1] = v.y * scale;
        tile[t >> 2][e + 2] = v.z * scale;
        tile[t >> 2][e + 3] = v.w * scale;
        __syncthreads();
        if (c0 + cs < ldc) {
            f32x4 o = {tile[cs][r], tile[cs + 1][r], tile[cs + 2][r], tile[cs + 3][r]};
            *reinterpret_cast<f32x4*>(dst + c0 + cs) = o;
        }
    }
}

__global__ __launch_bounds__(256) void pack_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wp,
                                                         int K, int C, int KH, int KW, int S, int P, int TY,
                                                         int TX, int ldc) {
    pack_dgrad_body(w, wp, K, C, KH, KW, S, P, TY, TX, ldc, blockIdx.x, blockIdx.y);
}

// One launch for many packs: jobs[j] describes one (weight, packed image) pair and the grid it would have had as a
// launch of its own; block b belongs to the job with block0 <= b < block0 + gx * gy.
struct PackJob {
    const float* w;
    float* wp;
    int kind;                 // 0 transpose_pad (forward), 1 forward tap-major, 2 dgrad, 3 dgrad tap-major
    int K, C, KH, KW, S, P;
    int gx, gy, block0;
};

__global__ __launch_bounds__(256) void pack_multi_kernel(const PackJob* __restrict__ jobs, int njobs) {
    const int b = blockIdx.x;
    int j = 0;
    while (j + 1 < njobs && jobs[j + 1].block0 <= b) ++j;
    const PackJob jb = jobs[j];
    const int l = b - jb.block0, bx = l % jb.gx, by = l / jb.gx;
    const int TY = (jb.KH + jb.S - 1) / jb.S, TX = (jb.KW + jb.S - 1) / jb.S;
    switch (jb.kind) {
        case 0: transpose_pad_body(jb.w, jb.wp, jb.K, jb.C * jb.KH * jb.KW, round4(jb.K), bx, by); break;
        case 1: pack_fwd_tap_body(jb.w, jb.wp, jb.K, jb.C, jb.KH * jb.KW, round_bk(jb.C), round4(jb.K), bx, jb.gx); break;
        case 2: pack_dgrad_body(jb.w, jb.wp, jb.K, jb.C, jb.KH, jb.KW, jb.S, jb.P, TY, TX, round4(jb.C), bx, by); break;
        case 5: pack_dgrad_k4_body(jb.w, jb.wp, jb.K, jb.C, round4(jb.C), bx); break;
        default:
            pack_dgrad_tap_body(jb.w, jb.wp, jb.K, jb.C, jb.KH, jb.KW, jb.S, jb.P, TY, TX, round_bk(jb.K), round4(jb.C), bx,
                                by, jb.gx);
    }
}

// The same bodies with the job table passed BY VALUE and an optional scale 1 / sigma[0] read from the device:
// spectral normalisation's w = weight_orig / sigma is a fresh tensor at every discriminator call, so its images cannot
// live in the persistent table above; one launch writes w itself (kind 4) and both packed images of every
// spectral-normalised layer (functional.spectral_normalize_multi) -- they were a div_scalar and two pack launches per
// layer and call.
constexpr int PACK_TABLE_MAX = 12;
struct PackTable {
    int njobs, pad;
    PackJob jobs[PACK_TABLE_MAX];
    const float* sigma[PACK_TABLE_MAX];
};

__global__ __launch_bounds__(256) void pack_table_kernel(PackTable t) {
    const int b = blockIdx.x;
    int j = 0;
    while (j + 1 < t.njobs && t.jobs[j + 1].block0 <= b) ++j;
    const PackJob& jb = t.jobs[j];
    const float scale = t.sigma[j] ? 1.f / t.sigma[j][0] : 1.f;
    const int l = b - jb.block0, bx = l % jb.gx, by = l / jb.gx;
    const int TY = (jb.KH + jb.S - 1) / jb.S, TX = (jb.KW + jb.S - 1) / jb.S;
    switch (jb.kind) {
        case 0: transpose_pad_body(jb.w, jb.wp, jb.K, jb.C * jb.KH * jb.KW, round4(jb.K), bx, by, scale); break;
        case 1:
            pack_fwd_tap_body(jb.w, jb.wp, jb.K, jb.C, jb.KH * jb.KW, round_bk(jb.C), round4(jb.K), bx, jb.gx, scale);
            break;
        case 2:
            pack_dgrad_body(jb.w, jb.wp, jb.K, jb.C, jb.KH, jb.KW, jb.S, jb.P, TY, TX, round4(jb.C), bx, by, scale);
            break;
        case 3:
            pack_dgrad_tap_body(jb.w, jb.wp, jb.K, jb.C, jb.KH, jb.KW, jb.S, jb.P, TY, TX, round_bk(jb.K), round4(jb.C), bx,
                                by, jb.gx, scale);
            break;
        case 5: pack_dgrad_k4_body(jb.w, jb.wp, jb.K, jb.C, round4(jb.C), bx, scale); break;
        default: {      // 4: wp = w * scale, same layout
            const long long total = (long long)jb.K * jb.C * jb.KH * jb.KW;
            for (long long i = (long long)bx * 256 + threadIdx.x; i < total; i += (long long)jb.gx * 256)
                jb.wp[i] = jb.w[i] * scale;
        }
    }
}

// out[i] = sum_s slab[s][i].  Small weight tensors reach here with hundreds of slabs (split-K over a 1M-long
// reduction), so the slabs are spread over the 16 wavefronts of a workgroup (64 outputs per workgroup, fixed
// summation order) instead of being walked by one thread.
__global__ __launch_bounds__(256) void reduce_few_slabs_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                               int S, long long count) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += slab[(long long)s * count + i];
    out[i] = acc;
}

constexpr int RS_WAVES = 16;
__global__ __launch_bounds__(64 * RS_WAVES) void reduce_slabs_kernel(const float* __restrict__ slab,
                                                                     float* __restrict__ out, int S,
                                                                     long long count, long long stride,
                                                                     float* __restrict__ out2, long long split) {
    __shared__ float part[RS_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + lane;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (i < count) {
        const float* p = slab + i;
        int s = wave;
        for (; s + 3 * RS_WAVES < S; s += 4 * RS_WAVES) {        // `stride` = slab row length (>= count)
            a0 += p[(long long)s * stride];
            a1 += p[(long long)(s + RS_WAVES) * stride];
            a2 += p[(long long)(s + 2 * RS_WAVES) * stride];
            a3 += p[(long long)(s + 3 * RS_WAVES) * stride];
        }
        for (; s < S; s += RS_WAVES) a0 += p[(long long)s * stride];
    }
    part[wave][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (wave == 0 && i < count) {
        float acc = 0.f;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) acc += part[w][lane];
        if (out2 && i >= split) out2[i - split] = acc;     // tail of the slab row: the fused bias gradient
        else out[i] = acc;
    }
}

void launch_reduce_few_slabs(const float* slab, float* out, int S, long long count, hipStream_t st) {
    hipLaunchKernelGGL(reduce_few_slabs_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, slab, out, S, count);
}

void launch_reduce_slabs(const float* slab, float* out, int S, long long count, long long stride, float* out2,
                         long long split, hipStream_t st) {
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64 * RS_WAVES), 0, st, slab, out, S,
                       count, stride, out2, split);
}

// Round 4: ONE launch sums the slabs of MANY weight gradients (the pack_multi idea applied to the other end of the
// step).  A split weight-gradient launch may leave its slabs unreduced (gz_conv2d_wgrad_partial); at the end of a
// backward pass -- or when a gradient bucket of the data-parallel exchange is complete -- gz_reduce_multi adds, per
// parameter, the slabs of every launch that contributed (a discriminator used on a real and a fake batch has two
// sources) and either writes or ACCUMULATES into the gradient (beta = 1: p.grad already holds earlier contributions;
// under data parallelism p.grad is a view of the flat exchange buffer).  Replaces, per DCGAN pair, 12 reduce launches
// + 11 framework `add_` launches of gradient accumulation by 2-4 launches.  The table travels as a kernel argument
// (no staging copy).  Summation order is fixed: wavefront w of a workgroup takes slabs w, w+4, ... of source 0, then
// of source 1, ...; the four partial sums meet in LDS in wavefront order.
constexpr int REDUCE_MAX_JOBS = 24;
struct ReduceJob {
    float* out;
    long long count;           // floats, a multiple of 4
    int beta, nsrc, block0, pad;
    ReduceSrc src[REDUCE_MAX_SRC];
};
struct ReduceTable {
    int njobs, pad;
    ReduceJob jobs[REDUCE_MAX_JOBS];
};

__global__ __launch_bounds__(256) void reduce_multi_kernel(ReduceTable t) {
    __shared__ f32x4 part[3][64];
    const int b = blockIdx.x;
    int j = 0;
    while (j + 1 < t.njobs && t.jobs[j + 1].block0 <= b) ++j;
    const ReduceJob& jb = t.jobs[j];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = ((long long)(b - jb.block0) * 64 + lane) * 4;
    const bool live = i < jb.count;
    const f32x4 r0 = reduce_sources(jb.src, jb.nsrc, i, live, lane, wave, part);
    if (wave == 0 && live) {
        f32x4 r = r0;
        f32x4* o = reinterpret_cast<f32x4*>(jb.out + i);
        if (jb.beta) r += *o;
        *o = r;
    }
}

}  // namespace gz

using namespace gz;

extern "C" {

long long gz_conv2d_pack_fwd_elems(int K, int C, int KH, int KW) {
    return (long long)(fwd_tap_major(C, KH, KW) ? round_bk(C) : C) * KH * KW * round4(K);
}

long long gz_conv2d_pack_dgrad_elems(int K, int C, int KH, int KW, int S) {
    int TY = (KH + S - 1) / S, TX = (KW + S - 1) / S;
    return (long long)S * S * (dgrad_tap_major(K, KH, KW, S) ? round_bk(K) : K) * TY * TX * round4(C);
}

int gz_conv2d_pack_fwd(const float* w, float* wp, int K, int C, int KH, int KW, hipStream_t stream) {
    gz::clear_stale_error();
    if (K <= 0 || C <= 0 || KH <= 0 || KW <= 0) return GZ_ERR_BAD_SHAPE;
    int Kg = C * KH * KW, ld = round4(K);
    if (fwd_tap_major(C, KH, KW)) {
        long long total = (long long)KH * KW * round_bk(C) * ld;
        hipLaunchKernelGGL(pack_fwd_tap_kernel, dim3((unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256)),
                           dim3(256), 0, stream, w, wp, K, C, KH * KW, round_bk(C), ld);
        return launch_status();
    }
    dim3 grid((Kg + 31) / 32, (ld + 31) / 32);
    hipLaunchKernelGGL(transpose_pad_kernel, grid, dim3(256), 0, stream, w, wp, K, Kg, ld);
    return launch_status();
}

int gz_conv2d_pack_dgrad(const float* w, float* wp, int K, int C, int KH, int KW, int S, int P,
                         hipStream_t stream) {
    gz::clear_stale_error();
    if (K <= 0 || C <= 0 || KH <= 0 || KW <= 0 || S <= 0) return GZ_ERR_BAD_SHAPE;
    int TY = (KH + S - 1) / S, TX = (KW + S - 1) / S;
    if (dgrad_tap_major(K, KH, KW, S)) {
        long long total = (long long)TY * TX * round_bk(K) * round4(C);
        unsigned bx = (unsigned)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
        hipLaunchKernelGGL(pack_dgrad_tap_kernel, dim3(bx, S * S), dim3(256), 0, stream, w, wp, K, C, KH, KW, S, P, TY,
                           TX, round_bk(K), round4(C));
        return launch_status();
    }
    hipLaunchKernelGGL(pack_dgrad_kernel, dim3(K, S * S), dim3(256), 0, stream, w, wp, K, C, KH, KW, S, P, TY, TX,
                       round4(C));
    return launch_status();
}

size_t gz_conv2d_pack_job_bytes(void) { return sizeof(PackJob); }

int gz_conv2d_pack_job(void* job_out, const float* w, float* wp, int is_dgrad, int K, int C, int KH, int KW, int S, int P,
                       int block0) {
    if (!job_out || K <= 0 || C <= 0 || KH <= 0 || KW <= 0 || S <= 0) return GZ_ERR_BAD_SHAPE;
    PackJob jb{w, wp, 0, K, C, KH, KW, S, P, 1, 1, block0};
    const int TY = (KH + S - 1) / S, TX = (KW + S - 1) / S;
    if (!is_dgrad) {
        if (fwd_tap_major(C, KH, KW)) {
            const long long total = (long long)KH * KW * round_bk(C) * round4(K);
            jb.kind = 1;
            jb.gx = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
        } else {
            jb.kind = 0;
            jb.gx = (C * KH * KW + 31) / 32;
            jb.gy = (round4(K) + 31) / 32;
        }
    } else if (dgrad_tap_major(K, KH, KW, S)) {
        const long long total = (long long)TY * TX * round_bk(K) * round4(C);
        jb.kind = 3;
        jb.gx = (int)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
        jb.gy = S * S;
    } else if (KH == 4 && KW == 4 && S == 2 && P == 1 && !knobs().no_pack_k4 && (((uintptr_t)w | (uintptr_t)wp) & 15) == 0) {
        jb.kind = 5;          // the whole ko in one workgroup, contiguous reads (pack_dgrad_k4_body)
        jb.gx = K;
        jb.gy = 1;
    } else {
        jb.kind = 2;
        jb.gx = K;
        jb.gy = S * S;
    }
    *reinterpret_cast<PackJob*>(job_out) = jb;
    return jb.gx * jb.gy;
}

int gz_conv2d_pack_multi(const void* jobs_dev, int njobs, int total_blocks, hipStream_t stream) {
    gz::clear_stale_error();
    if (!jobs_dev || njobs <= 0 || total_blocks <= 0) return GZ_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(pack_multi_kernel, dim3(total_blocks), dim3(256), 0, stream,
                       reinterpret_cast<const PackJob*>(jobs_dev), njobs);
    return launch_status();
}

int gz_conv2d_pack_table_max_jobs(void) { return PACK_TABLE_MAX; }
size_t gz_conv2d_pack_table_bytes(void) { return sizeof(PackTable); }

/* what: 0 the forward image, 1 the dgrad image, 2 a plain copy (w * scale in w's own layout) */
int gz_conv2d_pack_table_add(void* table_host, const float* w, float* wp, const float* sigma, int what, int K, int C, int KH,
                             int KW, int S, int P) {
    PackTable* t = reinterpret_cast<PackTable*>(table_host);
    if (!t || !w || !wp || what < 0 || what > 2) return GZ_ERR_BAD_SHAPE;
    if (t->njobs < 0 || t->njobs >= PACK_TABLE_MAX) return GZ_ERR_UNSUPPORTED;
    PackJob jb;
    if (what == 2) {
        if (K <= 0 || C <= 0 || KH <= 0 || KW <= 0) return GZ_ERR_BAD_SHAPE;
        const long long total = (long long)K * C * KH * KW;
        jb = PackJob{w, wp, 4, K, C, KH, KW, 1, 0, (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256), 1, 0};
    } else {
        const int n = gz_conv2d_pack_job(&jb, w, wp, what, K, C, KH, KW, S, P, 0);
        if (n < 0) return n;
    }
    t->jobs[t->njobs] = jb;
    t->sigma[t->njobs] = sigma;
    ++t->njobs;
    return GZ_OK;
}

int gz_conv2d_pack_table_launch(void* table_host, hipStream_t stream) {
    gz::clear_stale_error();
    PackTable* t = reinterpret_cast<PackTable*>(table_host);
    if (!t || t->njobs <= 0 || t->njobs > PACK_TABLE_MAX) return GZ_ERR_BAD_SHAPE;
    long long blocks = 0;
    for (int j = 0; j < t->njobs; ++j) {
        t->jobs[j].block0 = (int)blocks;
        blocks += (long long)t->jobs[j].gx * t->jobs[j].gy;
    }
    if (blocks <= 0 || blocks >= (1ll << 31)) return GZ_ERR_TOO_LARGE;
    hipLaunchKernelGGL(pack_table_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, *t);
    return launch_status();
}

long long gz_conv2d_pack_fwd_any_elems(int K, int C, int KH, int KW) {
    return (long long)round_bk(C) * KH * KW * round4(K);
}

int gz_conv2d_pack_fwd_any(const float* w, float* wp, int K, int C, int KH, int KW, hipStream_t stream) {
    gz::clear_stale_error();
    if (K <= 0 || C <= 0 || KH <= 0 || KW <= 0) return GZ_ERR_BAD_SHAPE;
    const int ld = round4(K);
    long long total = (long long)KH * KW * round_bk(C) * ld;
    hipLaunchKernelGGL(pack_fwd_tap_kernel, dim3((unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256)),
                       dim3(256), 0, stream, w, wp, K, C, KH * KW, round_bk(C), ld);
    return launch_status();
}

int gz_reduce_multi_max_jobs(void) { return REDUCE_MAX_JOBS; }
int gz_reduce_multi_max_sources(void) { return REDUCE_MAX_SRC; }
size_t gz_reduce_multi_table_bytes(void) { return sizeof(ReduceTable); }

/* table_host: a ReduceTable filled through gz_reduce_multi_add (host memory; copied into the kernel argument) */
int gz_reduce_multi_add(void* table_host, float* out, long long count, int beta, const float* slabs, int nz,
                        long long stride) {
    ReduceTable* t = reinterpret_cast<ReduceTable*>(table_host);
    // slabs == NULL, nz == 0: a contribution that is exactly ZERO (a bias in front of a normalisation over its own
    // plane): the job exists -- with beta = 0 the gradient is written as zeros by the same launch that sums the others,
    // instead of a fill launch per such parameter -- but reads nothing
    const bool zero_src = !slabs && nz == 0;
    if (!t || !out || (!slabs && !zero_src) || count <= 0 || (count & 3) || (stride & 3) || (!zero_src && nz < 1) ||
        (((uintptr_t)out | (uintptr_t)slabs) & 15))
        return GZ_ERR_BAD_SHAPE;
    for (int j = 0; j < t->njobs; ++j)
        if (t->jobs[j].out == out) {            // another contribution to the same gradient
            ReduceJob& jb = t->jobs[j];
            if (zero_src) return jb.count == count ? GZ_OK : GZ_ERR_UNSUPPORTED;
            if (jb.count != count || jb.nsrc >= REDUCE_MAX_SRC) return GZ_ERR_UNSUPPORTED;
            jb.src[jb.nsrc++] = ReduceSrc{slabs, stride, nz, 0};
            return GZ_OK;
        }
    if (t->njobs >= REDUCE_MAX_JOBS) return GZ_ERR_UNSUPPORTED;
    ReduceJob& jb = t->jobs[t->njobs++];
    jb.out = out;
    jb.count = count;
    jb.beta = beta ? 1 : 0;
    jb.nsrc = zero_src ? 0 : 1;
    jb.block0 = 0;
    jb.src[0] = ReduceSrc{slabs, stride, nz, 0};
    return GZ_OK;
}

int gz_reduce_multi(void* table_host, hipStream_t stream) {
    gz::clear_stale_error();
    ReduceTable* t = reinterpret_cast<ReduceTable*>(table_host);
    if (!t || t->njobs <= 0 || t->njobs > REDUCE_MAX_JOBS) return GZ_ERR_BAD_SHAPE;
    long long blocks = 0;
    for (int j = 0; j < t->njobs; ++j) {
        t->jobs[j].block0 = (int)blocks;
        blocks += (t->jobs[j].count + 255) / 256;
    }
    if (blocks <= 0 || blocks >= (1ll << 31)) return GZ_ERR_TOO_LARGE;
    hipLaunchKernelGGL(reduce_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, *t);
    return launch_status();
}

}  // extern "C"
