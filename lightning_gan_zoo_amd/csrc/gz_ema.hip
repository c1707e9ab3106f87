// Generator weight averaging (reference core/submodules/gan_stability/train.py:144-153, update_average):
//     avg = beta * avg + (1 - beta) * src      for every parameter of the generator,
// as ONE launch over any number of tensors.  The job table lives in device memory (the addresses of the parameters and
// of their averages never change, so it is built once per averaged generator -- the gz_conv2d_pack_multi pattern); a
// workgroup finds its tensor by binary search over the table's first-block prefix sums, so there is no cap on the
// number of tensors.  12 bytes per parameter: read avg, read src, write avg.
#include "gz_common.h"
#include "../../include/gz_ops.h"

namespace gz {

constexpr int EMA_THREADS = 256;
constexpr int EMA_CHUNK = 4096;      // elements per workgroup (OPT_CHUNK of gz_optim.hip)
constexpr int EMA_VEC = EMA_CHUNK / (EMA_THREADS * 4);      // float4 per thread

typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gfloat4;

struct EmaJob {
    float* avg;
    const float* src;
    long long n;
    int first_block;          // prefix sum of the chunk counts of the jobs in front of this one
    int vec4;                 // avg and src are both 16-byte aligned: float4 loads / stores
};

// Two multiplies and one add, no FMA contraction: the float4 path, the scalar path and the ragged tail round alike, and
// the result has the bits of torch's float32 evaluation of `beta * avg + (1. - beta) * src`.
__device__ __forceinline__ float ema_one(float a, float s, float beta, float omb) {
#pragma clang fp contract(off)
    const float x = beta * a;
    const float y = omb * s;
    return x + y;
}

__global__ __launch_bounds__(EMA_THREADS) void ema_kernel(const EmaJob* __restrict__ jobs, int count, float beta,
                                                          float omb) {
    const int b = blockIdx.x;
    int lo = 0, hi = count - 1;              // the LAST job with first_block <= b (empty jobs share their successor's)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const EmaJob jb = jobs[lo];
    const long long base = (long long)(b - jb.first_block) * EMA_CHUNK;
    const long long n = jb.n;
    if (base < 0 || base >= n) return;       // (a grid larger than the table's own block count writes nothing)
    // (pointers read from a table are generic to the compiler: say that they are global, or every access is a flat one)
    gfloat* avg = (gfloat*)jb.avg;
    const gfloat* src = (const gfloat*)jb.src;
    if (jb.vec4) {
        f32x4 a[EMA_VEC], s[EMA_VEC];
        // every load of the chunk is issued before the first store: avg and src may not be told apart by the compiler
#pragma unroll
        for (int k = 0; k < EMA_VEC; ++k) {
            const long long e = base + (long long)(k * EMA_THREADS + threadIdx.x) * 4;
            if (e + 4 <= n) {
                a[k] = *(const gfloat4*)(avg + e);
                s[k] = *(const gfloat4*)(src + e);
            }
        }
#pragma unroll
        for (int k = 0; k < EMA_VEC; ++k) {
            const long long e = base + (long long)(k * EMA_THREADS + threadIdx.x) * 4;
            if (e + 4 <= n) {
                f32x4 r;
                r[0] = ema_one(a[k][0], s[k][0], beta, omb);
                r[1] = ema_one(a[k][1], s[k][1], beta, omb);
                r[2] = ema_one(a[k][2], s[k][2], beta, omb);
                r[3] = ema_one(a[k][3], s[k][3], beta, omb);
                *(gfloat4*)(avg + e) = r;
            } else {
                for (long long q = e; q < n; ++q) avg[q] = ema_one(avg[q], src[q], beta, omb);      // ragged tail
            }
        }
        return;
    }
    for (int i = threadIdx.x; i < EMA_CHUNK; i += EMA_THREADS) {
        const long long e = base + i;
        if (e >= n) break;
        avg[e] = ema_one(avg[e], src[e], beta, omb);
    }
}

}  // namespace gz

using namespace gz;

extern "C" {

size_t gz_ema_job_bytes(void) { return sizeof(EmaJob); }

int gz_ema_job(void* job_out, float* avg, const float* src, long long numel, int first_block) {
    if (!job_out || numel < 0 || first_block < 0) return GZ_ERR_BAD_SHAPE;
    if (numel > 0) {
        if (!avg || !src) return GZ_ERR_BAD_SHAPE;
        const uintptr_t a = (uintptr_t)avg, s = (uintptr_t)src, bytes = (uintptr_t)numel * 4;
        if (a < s + bytes && s < a + bytes) return GZ_ERR_BAD_SHAPE;       // the update is not defined on overlapping ranges
    }
    const long long blocks = (numel + EMA_CHUNK - 1) / EMA_CHUNK;
    if (blocks + first_block > 0x7fffffffll) return GZ_ERR_TOO_LARGE;
    EmaJob jb{avg, src, numel, first_block, ((((uintptr_t)avg | (uintptr_t)src) & 15) == 0) ? 1 : 0};
    *reinterpret_cast<EmaJob*>(job_out) = jb;
    return (int)blocks;
}

int gz_ema_update(const void* jobs_dev, int count, int total_blocks, float beta, float one_minus_beta,
                  hipStream_t stream) {
    gz::clear_stale_error();
    if (!jobs_dev || count <= 0 || total_blocks < 0) return GZ_ERR_BAD_SHAPE;
    if (total_blocks == 0) return GZ_OK;                                   // every job is empty
    hipLaunchKernelGGL(ema_kernel, dim3(total_blocks), dim3(EMA_THREADS), 0, stream,
                       reinterpret_cast<const EmaJob*>(jobs_dev), count, beta, one_minus_beta);
    return launch_status();
}

}  // extern "C"
