// Common definitions for the gfx950 (MI355X / CDNA4) kernels of the GAN training step.
// Everything here is fp32: the parity target is the reference's PyTorch-CPU fp32 path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GZ_OK 0
#define GZ_ERR_BAD_SHAPE (-1)
#define GZ_ERR_UNSUPPORTED (-2)
#define GZ_ERR_WORKSPACE (-3)
#define GZ_ERR_HIP (-4)
#define GZ_ERR_TOO_LARGE (-5)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace gz {

// activation codes shared by the C ABI and the kernels
enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU = 2, ACT_TANH = 3 };

__device__ __forceinline__ float act_fwd(float v, int act, float slope) {
    switch (act) {
        case ACT_RELU: return v > 0.f ? v : 0.f;
        case ACT_LRELU: return v > 0.f ? v : v * slope;
        case ACT_TANH: return tanhf(v);
        default: return v;
    }
}

// derivative of the activation expressed through its OUTPUT o (valid for slope > 0)
__device__ __forceinline__ float act_bwd_from_out(float o, int act, float slope) {
    switch (act) {
        case ACT_RELU: return o > 0.f ? 1.f : 0.f;
        case ACT_LRELU: return o > 0.f ? 1.f : slope;
        case ACT_TANH: return 1.f - o * o;
        default: return 1.f;
    }
}

// Unsigned division by a run-time invariant (n < 2^31), branch-free.
struct FastDiv {
    uint32_t d, mul, sh1, sh2;
};

inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    f.mul = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    f.sh1 = l < 1 ? l : 1;
    f.sh2 = l > 0 ? l - 1 : 0;
    return f;
}

__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
    uint32_t t = __umulhi(n, f.mul);
    return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

// the one expression of the input step: (x / 255 - mean) / std as x * scale + shift.  Every kernel that turns a grey
// level into a float calls it (gz_resnet.hip's two input kernels, gz_infer.hip's fused Inception input), so the compiler
// contracts (or does not contract) the multiply-add the same way in all of them and their results agree bit for bit.
__device__ __forceinline__ float u8_norm(unsigned char v, float scale, float shift) { return (float)v * scale + shift; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Raw buffer loads: a voffset >= num_records (OOB for one) reads as 0 without a branch.
constexpr uint32_t OOB = 0x80000000u;  // voffset that is out of range for every tensor (< 2 GiB)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ f32x4 bload4(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// 2-D convolution geometry
// x: [N, C, H, W]   ("image side": conv input, dgrad output)
// y: [N, K, OH, OW] ("feature side": conv output, dgrad input)
// w: [K, C, KH, KW] (Conv2d weight; a ConvTranspose2d weight [Cin_T, Cout_T, KH, KW]
//                    is the same array with K = Cin_T, C = Cout_T)
struct ConvShape {
    int N, C, H, W, K, OH, OW;
};

inline const char*& last_error_slot() {
    static thread_local const char* msg = "";
    return msg;
}

inline int hip_status(hipError_t e) {
    if (e == hipSuccess) return GZ_OK;
    last_error_slot() = hipGetErrorString(e);
    return GZ_ERR_HIP;
}

inline int launch_status() { return hip_status(hipGetLastError()); }

// hipGetLastError is sticky per host thread: an unrelated, already-handled failure inside another
// library (e.g. a pointer-attribute query on host memory) would otherwise be reported by the next
// launcher.  Every C-ABI entry point clears it before its own launches.
inline void clear_stale_error() { (void)hipGetLastError(); }

}  // namespace gz
