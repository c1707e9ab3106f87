// Part of the fp32 implicit-GEMM core (see gz_igemm.h): the epilogues (accumulators -> row-major / NCHW / transposed-
// convolution phases, bias + activation, BatchNorm partial statistics), shared by both skeletons.
#pragma once
#include "gz_igemm_loaders.h"

namespace gz {

// ---------------------------------------------------------------------------
// epilogues.  Accumulator map of v_mfma_f32_32x32x2_f32: lane l, register r holds
//   C[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31]
// ---------------------------------------------------------------------------

// ---------------------------------------------------------------------------
// BatchNorm statistics from the accumulators (round 2; SURVEY 7.4 / VERDICT r1 item 6): per output channel the sum
// and the sum of squares over the tile's pixels, so that the separate read of the whole feature map (row_sums_kernel)
// disappears.  In the transposed-accumulator layout a lane owns a pixel and its 16 registers are 16 channels; the 32
// lanes of a half-wave are reduced with a halving butterfly: at step k the lanes whose bit k is clear keep the lower
// half of the surviving registers, the others the upper half, each adding what its partner sends -- 8 + 4 + 2 + 1 + 1
// shuffles for 16 registers instead of 16 x 5.  Afterwards lane l of the half holds register
// r = (b0 << 3) | (b1 << 2) | (b2 << 1) | b3 (b_k = bit k of l).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float half_wave_reduce16(const float (&v)[16], int lane) {
    float t[8], u[4], w[2];
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4, b3 = lane & 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = (b0 ? v[k + 8] : v[k]) + __shfl_xor(b0 ? v[k] : v[k + 8], 1, 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = (b1 ? t[k + 4] : t[k]) + __shfl_xor(b1 ? t[k] : t[k + 4], 2, 64);
#pragma unroll
    for (int k = 0; k < 2; ++k) w[k] = (b2 ? u[k + 2] : u[k]) + __shfl_xor(b2 ? u[k] : u[k + 2], 4, 64);
    float x = (b3 ? w[1] : w[0]) + __shfl_xor(b3 ? w[0] : w[1], 8, 64);
    return x + __shfl_xor(x, 16, 64);
}

// stats[row][ch] = (sum, sum of squares) over the pixels this wavefront owns (TM x 32 per half-wave), for its TN x 32
// channels.  Pixels past the end of the tensor hold exact zeros (their A rows were out of range) and add nothing.
template <int TM, int TN>
__device__ __forceinline__ void tile_channel_stats(f32x16 (&acc)[TM][TN], f32x2* __restrict__ stats, long long row,
                                                   int CH, int n_base, int lane) {
    const int half = lane >> 5;
    const int r = ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        float s1[16], s2[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const float v = acc[i][j][q];
                a += v;
                b = fmaf(v, v, b);
            }
            s1[q] = a;
            s2[q] = b;
        }
        const float t1 = half_wave_reduce16(s1, lane), t2 = half_wave_reduce16(s2, lane);
        const int ch = n_base + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if ((lane & 16) == 0 && ch < CH) stats[row * CH + ch] = f32x2{t1, t2};
    }
}

// C[z][m][n] row-major (n contiguous): wgrad slabs, plain GEMM.  Optional bias[n] + activation.
struct EpiRowMajor {
    static constexpr bool SWAP = false;   // lanes run along n, the contiguous dimension of the row-major output
    struct Params {
        float* c;
        int M, N, ldc;
        long long slab_stride;   // elements between split-K slabs / batches (z and y)
        const float* bias;       // per column, may be null
        int act;
        float slope;
    };
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        float* c = p.c + (long long)(z + y) * p.slab_stride;
        const int col_l = lane & 31, half = lane >> 5;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            int n = n_base + j * 32 + col_l;
            if (n >= p.N) continue;
            float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    int m = m_base + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (m < p.M) c[(long long)m * p.ldc + n] = act_fwd(acc[i][j][r] + bv, p.act, p.slope);
                }
            }
        }
    }
};

// NCHW feature map: row m = (n, pix), column = channel.  Pixels are the contiguous dimension, so the tile is
// accumulated transposed (SWAP: the MFMA operands trade places, D'[channel][m]): a lane owns one pixel, its 16
// registers are 16 channels, and every store instruction writes 32 consecutive pixels of one channel (128 B
// per half-wave) instead of 64 pieces in 64 different channel planes.  Optional bias[channel] + activation.
struct EpiNCHW {
    static constexpr bool SWAP = true;
    struct Params {
        float* out;
        int M, CH, HW;           // M = N*HW rows, CH channels
        FastDiv div_hw;
        const float* bias;
        int act;
        float slope;
        f32x2* stats;            // optional [rows][CH] partial BatchNorm statistics (bias null, act none); row = m_base / (TM*32)
    };
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        const int col_l = lane & 31, half = lane >> 5;
        if (p.stats) tile_channel_stats<TM, TN>(acc, p.stats, m_base / (TM * 32), p.CH, n_base, lane);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_base + i * 32 + col_l;
            if (m >= p.M) continue;
            const uint32_t n = fdiv((uint32_t)m, p.div_hw);
            const uint32_t pix = (uint32_t)m - n * (uint32_t)p.HW;
            float* base = p.out + (long long)n * p.CH * p.HW + pix;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = n_base + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (ch < p.CH) {
                        float bv = p.bias ? p.bias[ch] : 0.f;
                        base[(long long)ch * p.HW] = act_fwd(acc[i][j][r] + bv, p.act, p.slope);
                    }
                }
            }
        }
    }
};

// dgrad / transposed-conv output: row m = (n, a, b) of phase y=(py,px) goes to
// x[n][c][S*a+py][S*b+px].  Accumulated transposed like EpiNCHW: a store instruction covers 32 consecutive b of
// one channel (every S-th float of a row).  Optional bias[c] + activation.
template <int S>
struct EpiPhase {
    static constexpr bool SWAP = true;
    struct Params {
        float* out;
        int M, C, H, W, AH, AW;
        FastDiv div_ahw, div_aw;
        const float* bias;
        int act;
        float slope;
        f32x2* stats;            // optional [S*S phases x rows_per_phase][C] partial BatchNorm statistics
        int stats_rows;          // rows per phase = tiles_m * BM / (TM*32)
    };
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        const int col_l = lane & 31, half = lane >> 5;
        if (p.stats)
            tile_channel_stats<TM, TN>(acc, p.stats, (long long)y * p.stats_rows + m_base / (TM * 32), p.C, n_base, lane);
        const int py = y / S, px = y % S;
        const long long chs = (long long)p.H * p.W;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_base + i * 32 + col_l;
            if (m >= p.M) continue;
            uint32_t n = fdiv((uint32_t)m, p.div_ahw);
            uint32_t pix = (uint32_t)m - n * (uint32_t)(p.AH * p.AW);
            uint32_t a = fdiv(pix, p.div_aw);
            uint32_t b = pix - a * (uint32_t)p.AW;
            float* base = p.out + ((long long)n * p.C * p.H + (S * a + py)) * p.W + (S * b + px);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = n_base + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (c < p.C) {
                        float bv = p.bias ? p.bias[c] : 0.f;
                        base[(long long)c * chs] = act_fwd(acc[i][j][r] + bv, p.act, p.slope);
                    }
                }
            }
        }
    }
};

// 3-D transposed-conv output: row m = (n, a, b, c) of phase y = (pd, py, px) goes to
// x[n][ch][S*a+pd][S*b+py][S*c+px] (transposed accumulation, lanes along c).  Optional bias[ch] + activation.
template <int S>
struct EpiPhase3D {
    static constexpr bool SWAP = true;
    struct Params {
        float* out;
        int M, C, D, H, W, AD, AH, AW;
        FastDiv div_adhw, div_ahw, div_aw;
        const float* bias;
        int act;
        float slope;
    };
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        const int col_l = lane & 31, half = lane >> 5;
        const int pd = y / (S * S), py = (y / S) % S, px = y % S;
        const long long chs = (long long)p.D * p.H * p.W;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_base + i * 32 + col_l;
            if (m >= p.M) continue;
            uint32_t n = fdiv((uint32_t)m, p.div_adhw);
            uint32_t v = (uint32_t)m - n * (uint32_t)(p.AD * p.AH * p.AW);
            uint32_t a = fdiv(v, p.div_ahw);
            v -= a * (uint32_t)(p.AH * p.AW);
            uint32_t b = fdiv(v, p.div_aw);
            uint32_t c = v - b * (uint32_t)p.AW;
            float* base = p.out + (long long)n * p.C * chs + ((long long)(S * a + pd) * p.H + (S * b + py)) * p.W +
                          (S * c + px);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = n_base + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (ch < p.C) {
                        float bv = p.bias ? p.bias[ch] : 0.f;
                        base[(long long)ch * chs] = act_fwd(acc[i][j][r] + bv, p.act, p.slope);
                    }
                }
            }
        }
    }
};

// EpiPhase3D with the lean store path of EpiPhaseB (below) for the igemm2 skeleton, and ONLY that path: a bias is added
// on the way (the only epilogue HoloGAN's ConvTranspose3d layers have); the caller guarantees whole 32-channel blocks
// (C a multiple of 64) and applies an activation, if any, afterwards (p.act is ignored).
template <int S>
struct EpiPhase3DB {
    static constexpr bool SWAP = true;
    using Params = typename EpiPhase3D<S>::Params;
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        const int col_l = lane & 31, half = lane >> 5;
        const int pd = y / (S * S), py = (y / S) % S, px = y % S;
        const uint32_t chs = (uint32_t)(p.D * p.H * p.W) * 4u;           // bytes between channel volumes
        __amdgpu_buffer_rsrc_t rsrc = make_rsrc(p.out, (uint32_t)(p.M / (p.AD * p.AH * p.AW)) * (uint32_t)p.C * chs);
        uint32_t voff[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_base + i * 32 + col_l;
            const uint32_t n = fdiv((uint32_t)m, p.div_adhw);
            uint32_t v = (uint32_t)m - n * (uint32_t)(p.AD * p.AH * p.AW);
            const uint32_t a = fdiv(v, p.div_ahw);
            v -= a * (uint32_t)(p.AH * p.AW);
            const uint32_t b = fdiv(v, p.div_aw);
            const uint32_t c = v - b * (uint32_t)p.AW;
            const uint32_t o = (((n * (uint32_t)p.C + 4u * half) * (uint32_t)p.D + (S * a + pd)) * (uint32_t)p.H + (S * b + py)) *
                                   (uint32_t)p.W + (S * c + px);
            voff[i] = m < p.M ? o * 4u : OOB;
        }
        const uint32_t soff = (uint32_t)n_base * chs;
        // (n_base is wave-uniform; the two half-waves sit four channels apart.  Known cost: hipcc hoists the 32 bias loads
        // and the accumulator reads above the first store, and the 256x128 instantiation ends up with ~190 bytes of
        // scratch per lane in this epilogue -- without the bias it needs 51 VGPRs.  HoloGAN's block1 launch is split, so
        // its epilogue runs in splitk_finish_kernel, where registers are not scarce.)
        const float* bias = p.bias ? p.bias + n_base : nullptr;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cl = j * 32 + (r & 3) + 8 * (r >> 2);
                const uint32_t so = soff + (uint32_t)cl * chs;
                const float b0 = bias ? bias[cl] : 0.f, b1 = bias ? bias[cl + 4] : 0.f;
                const float bv = half ? b1 : b0;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const float v = acc[i][j][r] + bv;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rsrc, voff[i], so, 0);
                }
            }
        }
    }
};

// EpiRowMajor with the lean store path (weight-gradient slabs of the igemm2 skeleton): no bias / activation and the
// wavefront's rows inside the matrix -> buffer_store from the accumulator registers, column offset per lane, row
// through the scalar offset.
struct EpiRowMajorB {
    static constexpr bool SWAP = false;
    using Params = EpiRowMajor::Params;
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        const bool fast = !p.bias && p.act == ACT_NONE && m_base + TM * 32 <= p.M;       // wave-uniform
        if (!fast) {
            EpiRowMajor::template store<TM, TN>(p, acc, m_base, n_base, lane, y, z);
            return;
        }
        const int col_l = lane & 31, half = lane >> 5;
        float* c = p.c + (long long)(z + y) * p.slab_stride;
        __amdgpu_buffer_rsrc_t rsrc = make_rsrc(c, (uint32_t)p.M * (uint32_t)p.ldc * 4u);
        const uint32_t rs = (uint32_t)p.ldc * 4u;
        uint32_t voff[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n_base + j * 32 + col_l;
            voff[j] = n < p.N ? (uint32_t)n * 4u + 4u * half * rs : OOB;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t so = (uint32_t)(m_base + i * 32 + (r & 3) + 8 * (r >> 2)) * rs;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const float v = acc[i][j][r];
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rsrc, voff[j], so, 0);
                }
            }
        }
    }
};

// EpiNCHW with the lean store path of EpiPhaseB (below): no bias / activation, channel block inside the tensor ->
// buffer_store straight from the accumulator registers, per-lane byte offset once per 32-pixel block, channel through
// the scalar offset.
struct EpiNCHWB {
    static constexpr bool SWAP = true;
    using Params = EpiNCHW::Params;
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        const bool fast = !p.bias && p.act == ACT_NONE && n_base + TN * 32 <= p.CH;       // wave-uniform
        if (!fast) {
            EpiNCHW::template store<TM, TN>(p, acc, m_base, n_base, lane, y, z);
            return;
        }
        const int col_l = lane & 31, half = lane >> 5;
        if (p.stats) tile_channel_stats<TM, TN>(acc, p.stats, m_base / (TM * 32), p.CH, n_base, lane);
        const uint32_t chs = (uint32_t)p.HW * 4u;
        __amdgpu_buffer_rsrc_t rsrc = make_rsrc(p.out, (uint32_t)(p.M / p.HW) * (uint32_t)p.CH * chs);
        uint32_t voff[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_base + i * 32 + col_l;
            const uint32_t n = fdiv((uint32_t)m, p.div_hw);
            const uint32_t pix = (uint32_t)m - n * (uint32_t)p.HW;
            voff[i] = m < p.M ? ((n * (uint32_t)p.CH + 4u * half) * (uint32_t)p.HW + pix) * 4u : OOB;
        }
        const uint32_t soff = (uint32_t)n_base * chs;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t so = soff + (uint32_t)(j * 32 + (r & 3) + 8 * (r >> 2)) * chs;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const float v = acc[i][j][r];
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rsrc, voff[i], so, 0);
                }
            }
        }
    }
};

// The lean NCHW store WITH per-channel bias and ReLU (round 6: the evaluation path -- BatchNorm folded into weights +
// bias, then ReLU; csrc/gz_conv_fwd.hip run_fwd_any2).  A type of its own: adding bias / activation to EpiNCHWB's fast path
// made EVERY igemm2 instantiation spill (round 4).  Channel blocks outside the tensor take EpiNCHW's element-wise path.
struct EpiNCHWBiasAct {
    static constexpr bool SWAP = true;
    struct Params {
        float* out;              // channel 0 of THIS launch's output inside image 0 of the destination
        int M, CH, HW;           // M = N*HW rows, CH channels of this launch
        FastDiv div_hw;
        const float* bias;
        int act;
        float slope;
        int CHD;                 // channels per image of the destination (>= CH: a channel slice of a concatenation)
    };
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        const bool fast = p.bias && (p.act == ACT_NONE || p.act == ACT_RELU) && n_base + TN * 32 <= p.CH;   // wave-uniform
        const int col_l = lane & 31, half = lane >> 5;
        if (!fast) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = m_base + i * 32 + col_l;
                if (m >= p.M) continue;
                const uint32_t n = fdiv((uint32_t)m, p.div_hw);
                const uint32_t pix = (uint32_t)m - n * (uint32_t)p.HW;
                float* base = p.out + (long long)n * p.CHD * p.HW + pix;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ch = n_base + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        if (ch < p.CH) {
                            float bv = p.bias ? p.bias[ch] : 0.f;
                            base[(long long)ch * p.HW] = act_fwd(acc[i][j][r] + bv, p.act, p.slope);
                        }
                    }
                }
            }
            return;
        }
        const uint32_t chs = (uint32_t)p.HW * 4u;
        const uint32_t images = (uint32_t)(p.M / p.HW);
        __amdgpu_buffer_rsrc_t rsrc = make_rsrc(p.out, ((images - 1u) * (uint32_t)p.CHD + (uint32_t)p.CH) * chs);
        uint32_t voff[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_base + i * 32 + col_l;
            const uint32_t n = fdiv((uint32_t)m, p.div_hw);
            const uint32_t pix = (uint32_t)m - n * (uint32_t)p.HW;
            voff[i] = m < p.M ? ((n * (uint32_t)p.CHD + 4u * half) * (uint32_t)p.HW + pix) * 4u : OOB;
        }
        const uint32_t soff = (uint32_t)n_base * chs;
        const float floor_v = p.act == ACT_RELU ? 0.f : -3.402823466e38f;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int chl = j * 32 + (r & 3) + 8 * (r >> 2);
                const uint32_t so = soff + (uint32_t)chl * chs;
                const float bv = p.bias[n_base + chl + 4 * half];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const float v = fmaxf(acc[i][j][r] + bv, floor_v);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rsrc, voff[i], so, 0);
                }
            }
        }
    }
};

// EpiPhase with a lean store path for the igemm2 skeleton, where a workgroup's epilogue is NOT hidden behind three
// other resident workgroups: when there is no bias / activation and the wavefront's channel block lies inside the
// tensor, an accumulator goes out as  v_accvgpr_read + buffer_store  with a per-lane byte offset computed once per
// 32-pixel block (pixel decode, 4 VGPRs) and the channel advanced through the SCALAR offset -- ~3 instructions per
// store instead of ~20 (address arithmetic, predicates and branches per element; 34-55 k cycles per 128 accumulators
// measured with in-kernel stamps).  Pixels past M carry an out-of-range offset (dropped by the range check).
template <int S>
struct EpiPhaseB {
    static constexpr bool SWAP = true;
    using Params = typename EpiPhase<S>::Params;
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        const bool fast = !p.bias && p.act == ACT_NONE && n_base + TN * 32 <= p.C;       // wave-uniform
        if (!fast) {
            EpiPhase<S>::template store<TM, TN>(p, acc, m_base, n_base, lane, y, z);
            return;
        }
        const int col_l = lane & 31, half = lane >> 5;
        if (p.stats)
            tile_channel_stats<TM, TN>(acc, p.stats, (long long)y * p.stats_rows + m_base / (TM * 32), p.C, n_base, lane);
        const int py = y / S, px = y % S;
        const uint32_t chs = (uint32_t)(p.H * p.W) * 4u;                 // bytes between channel planes
        __amdgpu_buffer_rsrc_t rsrc = make_rsrc(p.out, (uint32_t)(p.M / (p.AH * p.AW)) * (uint32_t)p.C * chs);
        uint32_t voff[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_base + i * 32 + col_l;
            const uint32_t n = fdiv((uint32_t)m, p.div_ahw);
            const uint32_t pix = (uint32_t)m - n * (uint32_t)(p.AH * p.AW);
            const uint32_t a = fdiv(pix, p.div_aw);
            const uint32_t b = pix - a * (uint32_t)p.AW;
            const uint32_t o = ((n * (uint32_t)p.C + 4u * half) * (uint32_t)p.H + (S * a + py)) * (uint32_t)p.W + (S * b + px);
            voff[i] = m < p.M ? o * 4u : OOB;
        }
        uint32_t soff = (uint32_t)n_base * chs;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t so = soff + (uint32_t)(j * 32 + (r & 3) + 8 * (r >> 2)) * chs;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const float v = acc[i][j][r];      // (bit_cast of the vector-element expression itself reads element 0)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rsrc, voff[i], so, 0);
                }
            }
        }
    }
};

// All four output phases of a stride-2 transposed convolution in the accumulator blocks (round 6, ConvDg5A2): block
// j = 2 py + px of the SAME 32 channels.  A lane owns pixel (a, b), so its values for a channel are a 2 x 2 patch of the
// output: two 8-byte stores (rows 2a and 2a + 1 at x = 2b), 32 lanes = 256 contiguous bytes each -- whole 64-byte lines
// leave the CU.  (EpiPhaseB's 4-byte stores at stride 8 filled half of every line and relied on the L2 to merge the
// other column phase's workgroup -- which, with phases of unequal length ordered longest first, ran much later: 177 MB
// written for a 67 MB tensor, profiles/r05_traffic_pmc_detail.json.)  n_base in image columns: tile_n * 128 (+ j * 32
// from the split-K finish pass: single 4-byte stores of that phase).
struct EpiPhaseQuadB {
    static constexpr bool SWAP = true;
    using Params = typename EpiPhase<2>::Params;
    template <int TM, int TN>
    __device__ __forceinline__ static void store(const Params& p, f32x16 (&acc)[TM][TN], int m_base,
                                                 int n_base, int lane, int y, int z) {
        static_assert(TN == 1 || TN == 4, "all four phases or one phase block");
        const int col_l = lane & 31, half = lane >> 5;
        const int chan_base = (n_base >> 7) * 32;
        const int j1 = TN == 1 ? ((n_base & 127) >> 5) : 0;
        const uint32_t chs = (uint32_t)(p.H * p.W) * 4u;                 // bytes between channel planes
        __amdgpu_buffer_rsrc_t rsrc = make_rsrc(p.out, (uint32_t)(p.M / (p.AH * p.AW)) * (uint32_t)p.C * chs);
        uint32_t voff[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_base + i * 32 + col_l;
            const uint32_t n = fdiv((uint32_t)m, p.div_ahw);
            const uint32_t pix = (uint32_t)m - n * (uint32_t)(p.AH * p.AW);
            const uint32_t a = fdiv(pix, p.div_aw);
            const uint32_t b = pix - a * (uint32_t)p.AW;
            const uint32_t o = ((n * (uint32_t)p.C + 4u * half) * (uint32_t)p.H + (2 * a + (j1 >> 1))) * (uint32_t)p.W + (2 * b + (j1 & 1));
            voff[i] = (m < p.M && chan_base < p.C) ? o * 4u : OOB;
        }
        const uint32_t row = (uint32_t)p.W * 4u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t so = (uint32_t)(chan_base + (r & 3) + 8 * (r >> 2)) * chs;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if constexpr (TN == 4) {
                    typedef int v2i __attribute__((ext_vector_type(2)));
                    const float v0 = acc[i][0][r], v1 = acc[i][1][r], v2 = acc[i][2][r], v3 = acc[i][3][r];
                    v2i top, bot;
                    top.x = __builtin_bit_cast(int, v0); top.y = __builtin_bit_cast(int, v1);
                    bot.x = __builtin_bit_cast(int, v2); bot.y = __builtin_bit_cast(int, v3);
                    __builtin_amdgcn_raw_buffer_store_b64(top, rsrc, voff[i], so, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(bot, rsrc, voff[i], so + row, 0);
                } else {
                    const float v = acc[i][0][r];
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rsrc, voff[i], so, 0);
                }
            }
        }
    }
};

}  // namespace gz
