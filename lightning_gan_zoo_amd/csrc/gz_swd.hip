// Sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, section 5 and appendix) from the images
// alone (eval.swd_device).  Five launchers, all plain wave64 vector code:
//
//   swd_pyramid_kernel<S>   one workgroup per plane.  G_0 is staged in LDS; per level  T = down along W (S x S/2),
//                           G' = down of T along H (S/2 x S/2), V = up of G' along H (S x S/2, into T's space),
//                           L = G - up of V along W, written straight to the level's place in the packed output.  G' is
//                           the next level's G; nothing but x and the levels crosses HBM.  LDS: S^2 + S^2/2 floats per
//                           level above the coarsest, 256 for the coarsest: 127 KiB at S = 128.
//   swd_stats_kernel        per-channel sums of v - v0 and (v - v0)^2 over the gathered patch values, fp64, a fixed number
//                           of workgroups that depends on the row count alone; swd_stats_finish_kernel adds them in
//                           workgroup order and writes mean and population standard deviation.
//   swd_project_kernel      128 rows x 128 directions per workgroup of 512 threads.  The normalised descriptors go to LDS
//                           as desc[k][row] (lanes = rows: conflict-free), the directions as dirs[k][j]; wave w = (row
//                           half, direction group of 32): a thread owns one row and 32 directions, reads x_k once and its
//                           wave's 32 directions as broadcasts; a patch row's 7 products form one fma chain, the 7 C
//                           chains are added in order.  The workgroup loads its directions once and walks row tiles.
//   swd_sort_block_kernel   bitonic sort (or the merge tail of a longer phase) of SORT_BLOCK keys in one workgroup of 1024
//                           threads, 16 consecutive keys per thread: strides 1 .. 8 in registers, 16 .. 512 by lane
//                           exchange (the partner thread is 1 .. 32 lanes away), 1024 .. 8192 through LDS.
//   swd_sort_global_kernel  one compare-exchange stride >= SORT_BLOCK: a thread owns four consecutive keys (16 bytes) and
//                           the four a stride further.  swd_sort_global2_kernel: two such strides in one pass, four groups
//                           of four keys per thread; a phase's strides go two to a pass while two are left.
//   swd_distance_kernel     |a - b| of a row chunk of one column in fp64; swd_distance_finish_kernel adds the chunks and
//                           columns of a repeat in order.
//
// Keys are compared as integers: bits ^ ((bits >> 31) & 0x7fffffff) as a signed int orders every non-NaN float the way
// its value does (-0.0 below +0.0) and is its own inverse.  Bitonic networks compare fixed pairs, so equal keys need no
// care, and padding with +inf (the largest key) makes every length a power of two.
//
// No atomics, and every reduction runs in an order fixed by the shapes: two calls give equal bits.  Every index into an
// operand is checked against its count; offsets are 64-bit.
#include "gz_common.h"
#include "../../include/gz_ops.h"

namespace gz {

// ---------------------------------------------------------------------------------------------------------------------
// pyramid
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SWD_COARSEST = 16;
constexpr int SWD_MAX_LEVELS = 4;

constexpr int swd_pyr_lds_floats(int s) { return s <= SWD_COARSEST ? s * s : s * s + s * s / 2 + swd_pyr_lds_floats(s / 2); }
constexpr int swd_pyr_threads(int s) { return s >= 64 ? 1024 : 256; }

__device__ __forceinline__ int swd_mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ __forceinline__ float swd_tap(int t) { return t == 2 ? 0.375f : ((t == 1 || t == 3) ? 0.25f : 0.0625f); }

struct SwdPyrOut {
    float* level[SWD_MAX_LEVELS];     // this plane's place in each level
};

// Every tap sum is one chain of fused multiply-adds from 0, t = 0 .. 4.  The first one, 2^-4 x + 0, is exact, so a down stage
// rounds 4 times; an up stage multiplies the odd (inserted) samples, which are 0, and adds nothing for them: at most 2
// roundings.  The tests' error bound counts exactly these.
// the levels from size S down, G (S x S) already in LDS at g and visible to every thread; `space` is free LDS behind it
template <int S, int THREADS>
__device__ __forceinline__ void swd_pyr_levels(const float* g, float* space, const SwdPyrOut& out, int l) {
    const int tid = threadIdx.x;
    if constexpr (S <= SWD_COARSEST) {
        for (int i = tid; i < S * S; i += THREADS) out.level[l][i] = g[i];
    } else {
        constexpr int H = S / 2;
        float* t = space;              // [S][H]: T, then V
        float* gn = space + S * H;     // [H][H]
        for (int i = tid; i < S * H; i += THREADS) {
            const int r = i / H, c = i % H;
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 5; ++q) v = __builtin_fmaf(swd_tap(q), g[r * S + swd_mirror(2 * c + q - 2, S)], v);
            t[i] = v;
        }
        __syncthreads();
        for (int i = tid; i < H * H; i += THREADS) {
            const int r = i / H, c = i % H;
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 5; ++q) v = __builtin_fmaf(swd_tap(q), t[swd_mirror(2 * r + q - 2, S) * H + c], v);
            gn[i] = v;
        }
        __syncthreads();
        for (int i = tid; i < S * H; i += THREADS) {
            const int r = i / H, c = i % H;
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const int k = swd_mirror(r + q - 2, S);
                v = __builtin_fmaf(2.f * swd_tap(q), (k & 1) ? 0.f : gn[(k >> 1) * H + c], v);
            }
            t[i] = v;
        }
        __syncthreads();
        for (int i = tid; i < S * S; i += THREADS) {
            const int r = i / S, c = i % S;
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const int k = swd_mirror(c + q - 2, S);
                v = __builtin_fmaf(2.f * swd_tap(q), (k & 1) ? 0.f : t[r * H + (k >> 1)], v);
            }
            out.level[l][i] = g[i] - v;
        }
        // (the next level reads gn and writes behind it: nothing it touches is still being read here)
        swd_pyr_levels<H, THREADS>(gn, gn + H * H, out, l + 1);
    }
}

template <int S>
__global__ __launch_bounds__(swd_pyr_threads(S)) void swd_pyramid_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                         long long planes) {
    constexpr int THREADS = swd_pyr_threads(S);
    __shared__ __attribute__((aligned(16))) float lds[swd_pyr_lds_floats(S)];
    const long long plane = blockIdx.x;
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(x + plane * (S * S));
    for (int i = threadIdx.x; i < S * S / 4; i += THREADS) reinterpret_cast<f32x4*>(lds)[i] = src[i];
    SwdPyrOut o;
    long long off = 0;
    int s = S;
#pragma unroll
    for (int l = 0; l < SWD_MAX_LEVELS; ++l) {
        o.level[l] = out + off + plane * (s * s);
        off += planes * (s * s);
        if (s > SWD_COARSEST) s >>= 1;
    }
    __syncthreads();
    swd_pyr_levels<S, THREADS>(lds, lds + S * S, o, 0);
}

inline int swd_levels(int S) {
    switch (S) {
        case 16: return 1;
        case 32: return 2;
        case 64: return 3;
        case 128: return 4;
        default: return 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// patches
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SWD_PATCH = 7, SWD_TAPS = 49, SWD_MAX_C = 3, SWD_MAX_D = SWD_TAPS * SWD_MAX_C;

struct SwdPatches {
    const float* level;
    const int* pos;
    long long rows;
    int C, H, P;
};

// the address of tap 0 of channel 0 of a row's patch; a centre outside [3, H - 3) is clamped into it
__device__ __forceinline__ const float* swd_patch_origin(const SwdPatches& p, long long row) {
    const int cy = min(max(p.pos[2 * row], 3), p.H - 4), cx = min(max(p.pos[2 * row + 1], 3), p.H - 4);
    const long long image = row / p.P;
    return p.level + (image * p.C * p.H + (cy - 3)) * p.H + (cx - 3);
}

constexpr int SWD_STATS_THREADS = 256, SWD_STATS_MAX_BLOCKS = 256;

inline int swd_stats_blocks(long long rows) {
    const long long b = (rows + SWD_STATS_THREADS - 1) / SWD_STATS_THREADS;
    return (int)(b < SWD_STATS_MAX_BLOCKS ? b : SWD_STATS_MAX_BLOCKS);
}

// part[block][2 * c], [2 * c + 1]: the block's sums of v - v0_c and (v - v0_c)^2
__global__ __launch_bounds__(SWD_STATS_THREADS) void swd_stats_kernel(SwdPatches p, double* __restrict__ part) {
    __shared__ double sW[SWD_STATS_THREADS / 64][2 * SWD_MAX_C];
    const float* first = swd_patch_origin(p, 0);
    double s1[SWD_MAX_C], s2[SWD_MAX_C], v0[SWD_MAX_C];
#pragma unroll
    for (int c = 0; c < SWD_MAX_C; ++c) {
        s1[c] = s2[c] = 0.0;
        v0[c] = c < p.C ? (double)first[(long long)c * p.H * p.H] : 0.0;
    }
    for (long long row = (long long)blockIdx.x * SWD_STATS_THREADS + threadIdx.x; row < p.rows;
         row += (long long)gridDim.x * SWD_STATS_THREADS) {
        const float* o = swd_patch_origin(p, row);
#pragma unroll
        for (int c = 0; c < SWD_MAX_C; ++c) {
            if (c < p.C) {
                const float* oc = o + (long long)c * p.H * p.H;
                for (int dy = 0; dy < SWD_PATCH; ++dy)
#pragma unroll
                    for (int dx = 0; dx < SWD_PATCH; ++dx) {
                        const double d = (double)oc[dy * p.H + dx] - v0[c];
                        s1[c] += d;
                        s2[c] += d * d;
                    }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < SWD_MAX_C; ++c) {
        s1[c] = wave_sum_d(s1[c]);
        s2[c] = wave_sum_d(s2[c]);
        if ((threadIdx.x & 63) == 0) {
            sW[threadIdx.x >> 6][2 * c] = s1[c];
            sW[threadIdx.x >> 6][2 * c + 1] = s2[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * SWD_MAX_C) {
        double v = 0.0;
        for (int w = 0; w < SWD_STATS_THREADS / 64; ++w) v += sW[w][threadIdx.x];
        part[(size_t)blockIdx.x * (2 * SWD_MAX_C) + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void swd_stats_finish_kernel(SwdPatches p, const double* __restrict__ part, int blocks,
                                                              double* __restrict__ stats) {
    const int c = threadIdx.x;
    if (c >= p.C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < blocks; ++b) {
        s1 += part[(size_t)b * (2 * SWD_MAX_C) + 2 * c];
        s2 += part[(size_t)b * (2 * SWD_MAX_C) + 2 * c + 1];
    }
    const double count = (double)p.rows * SWD_TAPS;
    const double v0 = (double)swd_patch_origin(p, 0)[(long long)c * p.H * p.H];
    const double m = s1 / count, var = s2 / count - m * m;
    stats[c] = v0 + m;
    stats[p.C + c] = var > 0.0 ? sqrt(var) : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------
// projection
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SWD_PROJ_ROWS = 128, SWD_PROJ_DIRS = 128, SWD_PROJ_THREADS = 512, SWD_PROJ_OWN = 32;
constexpr int SWD_PROJ_MAX_GRID = 512;          // row workgroups per direction chunk: each walks tiles blockIdx.x, + grid, ..

__global__ __launch_bounds__(SWD_PROJ_THREADS) void swd_project_kernel(SwdPatches p, const double* __restrict__ stats,
                                                                       const float* __restrict__ dirs, int ndirs,
                                                                       float* __restrict__ proj, long long pitch,
                                                                       long long padded) {
    __shared__ __attribute__((aligned(16))) float sDesc[SWD_MAX_D * SWD_PROJ_ROWS];
    __shared__ __attribute__((aligned(16))) float sDirs[SWD_MAX_D * SWD_PROJ_DIRS];
    const int tid = threadIdx.x, D = SWD_TAPS * p.C;
    const int dir0 = blockIdx.y * SWD_PROJ_DIRS;
    const long long tiles = (p.rows + SWD_PROJ_ROWS - 1) / SWD_PROJ_ROWS;

    float mean[SWD_MAX_C], scale[SWD_MAX_C];
#pragma unroll
    for (int c = 0; c < SWD_MAX_C; ++c) {
        const double sd = c < p.C ? stats[p.C + c] : 0.0;
        mean[c] = c < p.C ? (float)stats[c] : 0.f;
        scale[c] = (float)(1.0 / (sd == 0.0 ? 1.0 : sd));
    }
    // sDirs[k][j] = dirs[dir0 + j][k], zero beyond ndirs: once per workgroup, which then walks its row tiles.  Lanes run
    // along k (coalesced reads), so a wave's LDS writes share a bank: 37 serialised writes per thread, paid once per
    // workgroup and not per tile
    for (int i = tid; i < SWD_PROJ_DIRS * D; i += SWD_PROJ_THREADS) {
        const int j = i / D, k = i - j * D;
        sDirs[k * SWD_PROJ_DIRS + j] = dir0 + j < ndirs ? dirs[(long long)(dir0 + j) * D + k] : 0.f;
    }
    const int wave = tid >> 6, lane = tid & 63;
    const int r = (wave & 1) * 64 + lane, j0 = (wave >> 1) * SWD_PROJ_OWN;      // j0 is the same in the whole wave
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long row0 = tile * SWD_PROJ_ROWS;
        // sDesc[k][row]: the normalised descriptors, zero beyond the last row.  The thread count is a multiple of the tile's
        // rows, so a thread gathers one row's elements k = tid / 128, + 4, ..: its patch origin is found once per tile
        static_assert(SWD_PROJ_THREADS % SWD_PROJ_ROWS == 0, "a thread must stay on one row of the tile");
        {
            const int rr = tid & (SWD_PROJ_ROWS - 1);
            const bool in = row0 + rr < p.rows;
            const float* origin = in ? swd_patch_origin(p, row0 + rr) : p.level;
            for (int k = tid / SWD_PROJ_ROWS; k < D; k += SWD_PROJ_THREADS / SWD_PROJ_ROWS) {
                float v = 0.f;
                if (in) {
                    const int c = k / SWD_TAPS, tap = k - c * SWD_TAPS, dy = tap / SWD_PATCH, dx = tap - dy * SWD_PATCH;
                    const float d = origin[((long long)c * p.H + dy) * p.H + dx];
                    v = (d - (c == 0 ? mean[0] : (c == 1 ? mean[1] : mean[2]))) *
                        (c == 0 ? scale[0] : (c == 1 ? scale[1] : scale[2]));
                }
                sDesc[k * SWD_PROJ_ROWS + rr] = v;
            }
        }
        __syncthreads();
        // one patch row (channel, dy) at a time: its 7 products in one chain from 0, dx ascending, then added to the
        // total, rows in (channel, dy) order -- 7 + 7 C roundings on any path instead of 49 C
        float acc[SWD_PROJ_OWN];
#pragma unroll
        for (int q = 0; q < SWD_PROJ_OWN; ++q) acc[q] = 0.f;
        for (int g = 0; g < D; g += SWD_PATCH) {
            float part[SWD_PROJ_OWN];
#pragma unroll
            for (int q = 0; q < SWD_PROJ_OWN; ++q) part[q] = 0.f;
#pragma unroll
            for (int dx = 0; dx < SWD_PATCH; ++dx) {
                const int k = g + dx;
                const float xk = sDesc[k * SWD_PROJ_ROWS + r];
                const f32x4* w = reinterpret_cast<const f32x4*>(sDirs + k * SWD_PROJ_DIRS + j0);
#pragma unroll
                for (int q = 0; q < SWD_PROJ_OWN / 4; ++q) {
                    const f32x4 d4 = w[q];
                    part[4 * q + 0] = __builtin_fmaf(xk, d4[0], part[4 * q + 0]);
                    part[4 * q + 1] = __builtin_fmaf(xk, d4[1], part[4 * q + 1]);
                    part[4 * q + 2] = __builtin_fmaf(xk, d4[2], part[4 * q + 2]);
                    part[4 * q + 3] = __builtin_fmaf(xk, d4[3], part[4 * q + 3]);
                }
            }
#pragma unroll
            for (int q = 0; q < SWD_PROJ_OWN; ++q) acc[q] += part[q];
        }
        if (row0 + r < p.rows) {
#pragma unroll
            for (int q = 0; q < SWD_PROJ_OWN; ++q)
                if (dir0 + j0 + q < ndirs) proj[(long long)(dir0 + j0 + q) * pitch + row0 + r] = acc[q];
        }
        __syncthreads();            // (the next tile's descriptors overwrite sDesc)
    }
    // the sort's padding: rows .. padded - 1 of this workgroup's directions, shared among the row workgroups
    for (long long i = p.rows + (long long)blockIdx.x * SWD_PROJ_THREADS + tid; i < padded;
         i += (long long)gridDim.x * SWD_PROJ_THREADS)
        for (int j = dir0; j < min(dir0 + SWD_PROJ_DIRS, ndirs); ++j) proj[(long long)j * pitch + i] = INFINITY;
}

// ---------------------------------------------------------------------------------------------------------------------
// sort
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SORT_BLOCK = 16384, SORT_THREADS = 1024, SORT_OWN = 16, SORT_GLOBAL_THREADS = 256;
constexpr int SORT_INF_KEY = 0x7f800000;        // +inf: its key is its bits

__device__ __forceinline__ int swd_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

// strides J < 16: both keys of a pair are this thread's; e0 = the index of v[0] in the column
template <int J>
__device__ __forceinline__ void swd_sort_regs(int (&v)[SORT_OWN], long long e0, long long k) {
#pragma unroll
    for (int i = 0; i < SORT_OWN; ++i) {
        if ((i & J) == 0) {
            const bool asc = ((e0 + i) & k) == 0;
            const int lo = min(v[i], v[i | J]), hi = max(v[i], v[i | J]);
            v[i] = asc ? lo : hi;
            v[i | J] = asc ? hi : lo;
        }
    }
}

// phases k = k_first .. k_last (doubling), each from stride min(k / 2, SORT_BLOCK / 2) down to 1, on the SORT_BLOCK keys
// of block blockIdx.x of column blockIdx.y.  Keys at or beyond `rows` are +inf whatever memory holds; keys at or beyond
// `padded` are neither compared with anything below it (k_last <= padded) nor written.
__global__ __launch_bounds__(SORT_THREADS) void swd_sort_block_kernel(float* __restrict__ data, long long rows,
                                                                      long long padded, long long pitch, long long k_first,
                                                                      long long k_last) {
    __shared__ __attribute__((aligned(16))) int sK[SORT_BLOCK];
    const int tid = threadIdx.x;
    int* col = reinterpret_cast<int*>(data) + (long long)blockIdx.y * pitch;
    const long long e0 = (long long)blockIdx.x * SORT_BLOCK + tid * SORT_OWN;
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    int v[SORT_OWN];
    if (e0 + SORT_OWN <= rows) {                          // (pitch % 4 == 0 and e0 % 16 == 0: 16-byte aligned)
#pragma unroll
        for (int i = 0; i < SORT_OWN / 4; ++i) {
            const i32x4 q = reinterpret_cast<const i32x4*>(col + e0)[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[4 * i + c] = swd_key(q[c]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < SORT_OWN; ++i) v[i] = e0 + i < rows ? swd_key(col[e0 + i]) : SORT_INF_KEY;
    }

    for (long long k = k_first; k <= k_last; k <<= 1) {
        const bool asc = (e0 & k) == 0;                   // (for k >= 16: the whole thread sorts one way)
        for (int j = (int)(k / 2 < SORT_BLOCK / 2 ? k / 2 : SORT_BLOCK / 2); j > 0; j >>= 1) {
            if (j >= 64 * SORT_OWN) {                     // the partner thread is in another wave
#pragma unroll
                for (int i = 0; i < SORT_OWN; ++i) sK[i * SORT_THREADS + tid] = v[i];
                __syncthreads();
                const int partner = tid ^ (j / SORT_OWN);
                const bool keep_min = ((tid & (j / SORT_OWN)) == 0) == asc;
#pragma unroll
                for (int i = 0; i < SORT_OWN; ++i) {
                    const int o = sK[i * SORT_THREADS + partner];
                    v[i] = keep_min ? min(v[i], o) : max(v[i], o);
                }
                __syncthreads();
            } else if (j >= SORT_OWN) {                   // the partner thread is a lane of this wave
                const int mask = j / SORT_OWN;
                const bool keep_min = ((tid & mask) == 0) == asc;
#pragma unroll
                for (int i = 0; i < SORT_OWN; ++i) {
                    const int o = __shfl_xor(v[i], mask, 64);
                    v[i] = keep_min ? min(v[i], o) : max(v[i], o);
                }
            } else {
                switch (j) {
                    case 8: swd_sort_regs<8>(v, e0, k); break;
                    case 4: swd_sort_regs<4>(v, e0, k); break;
                    case 2: swd_sort_regs<2>(v, e0, k); break;
                    default: swd_sort_regs<1>(v, e0, k); break;
                }
            }
        }
    }
    if (e0 + SORT_OWN <= padded) {
#pragma unroll
        for (int i = 0; i < SORT_OWN / 4; ++i) {
            i32x4 q;
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = swd_key(v[4 * i + c]);
            reinterpret_cast<i32x4*>(col + e0)[i] = q;
        }
    } else {
#pragma unroll
        for (int i = 0; i < SORT_OWN; ++i)
            if (e0 + i < padded) col[e0 + i] = swd_key(v[i]);
    }
}

// stride j >= SORT_BLOCK of phase k: thread t of column blockIdx.y owns keys e .. e + 3 and e + j .. e + j + 3, e the t-th
// multiple of 4 with bit j clear
__global__ __launch_bounds__(SORT_GLOBAL_THREADS) void swd_sort_global_kernel(float* __restrict__ data, long long padded,
                                                                              long long pitch, long long k, long long j) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const long long t = (long long)blockIdx.x * SORT_GLOBAL_THREADS + threadIdx.x;
    if (t >= padded / 8) return;
    const long long q = t * 4, e = ((q & ~(j - 1)) << 1) | (q & (j - 1));
    i32x4* col = reinterpret_cast<i32x4*>(reinterpret_cast<int*>(data) + (long long)blockIdx.y * pitch);
    i32x4 a = col[e / 4], b = col[(e + j) / 4];
    const bool asc = (e & k) == 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ka = swd_key(a[i]), kb = swd_key(b[i]);
        const int lo = min(ka, kb), hi = max(ka, kb);
        a[i] = swd_key(asc ? lo : hi);
        b[i] = swd_key(asc ? hi : lo);
    }
    col[e / 4] = a;
    col[(e + j) / 4] = b;
}

// strides j and j / 2 of phase k in one pass, both >= SORT_BLOCK: thread t owns four keys at each of e, e + j / 2, e + j and
// e + 3 j / 2, e the t-th multiple of 4 with bits j and j / 2 clear.  The four groups lie in one half of the phase's 2 k
// span, so they sort one way.
__global__ __launch_bounds__(SORT_GLOBAL_THREADS) void swd_sort_global2_kernel(float* __restrict__ data, long long padded,
                                                                               long long pitch, long long k, long long j) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const long long t = (long long)blockIdx.x * SORT_GLOBAL_THREADS + threadIdx.x;
    if (t >= padded / 16) return;
    const long long h = j >> 1, q = t * 4, e = ((q & ~(h - 1)) << 2) | (q & (h - 1));
    i32x4* col = reinterpret_cast<i32x4*>(reinterpret_cast<int*>(data) + (long long)blockIdx.y * pitch);
    i32x4 x[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) x[g] = col[(e + g * h) / 4];
    const bool asc = (e & k) == 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int key[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) key[g] = swd_key(x[g][i]);
#pragma unroll
        for (int s = 2; s > 0; s >>= 1) {                 // stride j pairs groups (0, 2), (1, 3); stride j / 2 (0, 1), (2, 3)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if ((g & s) == 0) {
                    const int lo = min(key[g], key[g | s]), hi = max(key[g], key[g | s]);
                    key[g] = asc ? lo : hi;
                    key[g | s] = asc ? hi : lo;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) x[g][i] = swd_key(key[g]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) col[(e + g * h) / 4] = x[g];
}

struct SortPlan {
    long long padded;
    int block_passes, global_passes;
};

inline bool swd_sort_plan(long long rows, SortPlan& p) {
    if (rows < 1 || rows > (1ll << 40)) return false;
    p.padded = 1;
    while (p.padded < rows) p.padded <<= 1;
    p.block_passes = 1;
    p.global_passes = 0;
    for (long long k = 2ll * SORT_BLOCK; k <= p.padded; k <<= 1) {
        ++p.block_passes;
        for (long long j = k / 2; j >= SORT_BLOCK; j >>= (j / 2 >= SORT_BLOCK ? 2 : 1)) ++p.global_passes;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// distance
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SWD_DIST_THREADS = 256, SWD_DIST_CHUNK = 16384;      // rows of one column per workgroup

inline long long swd_dist_chunks(long long rows) { return (rows + SWD_DIST_CHUNK - 1) / SWD_DIST_CHUNK; }

__global__ __launch_bounds__(SWD_DIST_THREADS) void swd_distance_kernel(const float* __restrict__ a,
                                                                        const float* __restrict__ b, long long rows,
                                                                        long long pitch, double* __restrict__ part) {
    __shared__ double sW[SWD_DIST_THREADS / 64];
    const float* ca = a + (long long)blockIdx.y * pitch;
    const float* cb = b + (long long)blockIdx.y * pitch;
    const long long r0 = (long long)blockIdx.x * SWD_DIST_CHUNK;
    const long long r1 = r0 + SWD_DIST_CHUNK < rows ? r0 + SWD_DIST_CHUNK : rows;
    double s = 0.0;
    for (long long r = r0 + threadIdx.x; r < r1; r += SWD_DIST_THREADS) s += fabs((double)ca[r] - (double)cb[r]);
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int w = 0; w < SWD_DIST_THREADS / 64; ++w) v += sW[w];
        part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = v;
    }
}

// block q: the count partials of repeat q, thread-strided in index order, butterfly, waves in order
__global__ __launch_bounds__(SWD_DIST_THREADS) void swd_distance_finish_kernel(const double* __restrict__ part,
                                                                               long long count, double* __restrict__ out) {
    __shared__ double sW[SWD_DIST_THREADS / 64];
    const double* p = part + (size_t)blockIdx.x * (size_t)count;
    double s = 0.0;
    for (long long i = threadIdx.x; i < count; i += SWD_DIST_THREADS) s += p[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int w = 0; w < SWD_DIST_THREADS / 64; ++w) v += sW[w];
        out[blockIdx.x] = v;
    }
}

inline bool swd_patches_ok(int n, int C, int H, int P) {
    return n >= 1 && (C == 1 || C == 3) && swd_levels(H) > 0 && P >= 1;
}

template <int S>
inline int swd_pyramid_launch(const float* x, long long planes, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(swd_pyramid_kernel<S>, dim3((unsigned)planes), dim3(swd_pyr_threads(S)), 0, stream, x, out, planes);
    return launch_status();
}

}  // namespace gz

using namespace gz;

extern "C" {

int gz_swd_pyramid_describe(int N, int C, int S, int* levels, long long* offsets) {
    if (!levels || !offsets || N < 1 || (C != 1 && C != 3)) return GZ_ERR_BAD_SHAPE;
    const int L = swd_levels(S);
    if (L == 0) return GZ_ERR_UNSUPPORTED;
    long long off = 0;
    for (int l = 0; l < L; ++l) {
        offsets[l] = off;
        off += (long long)N * C * (S >> l) * (S >> l);
    }
    offsets[L] = off;
    *levels = L;
    return GZ_OK;
}

int gz_swd_pyramid(const float* x, int N, int C, int S, float* out, long long out_elems, hipStream_t stream) {
    gz::clear_stale_error();
    if (!x || !out || N < 1 || (C != 1 && C != 3) || (reinterpret_cast<uintptr_t>(x) & 15) != 0) return GZ_ERR_BAD_SHAPE;
    int levels;
    long long offsets[SWD_MAX_LEVELS + 1];
    const int rc = gz_swd_pyramid_describe(N, C, S, &levels, offsets);
    if (rc != GZ_OK) return rc;
    if (out_elems < offsets[levels]) return GZ_ERR_WORKSPACE;
    const long long planes = (long long)N * C;
    if (planes > 0x7fffffffll) return GZ_ERR_TOO_LARGE;
    switch (S) {
        case 16: return swd_pyramid_launch<16>(x, planes, out, stream);
        case 32: return swd_pyramid_launch<32>(x, planes, out, stream);
        case 64: return swd_pyramid_launch<64>(x, planes, out, stream);
        default: return swd_pyramid_launch<128>(x, planes, out, stream);
    }
}

size_t gz_swd_channel_stats_workspace_bytes(int n, int C, int H, int P) {
    if (!swd_patches_ok(n, C, H, P)) return 0;
    return (size_t)swd_stats_blocks((long long)n * P) * 2 * SWD_MAX_C * sizeof(double);
}

int gz_swd_channel_stats(const float* level, int n, int C, int H, const int* pos, int P, double* stats, void* workspace,
                         size_t ws_bytes, hipStream_t stream) {
    gz::clear_stale_error();
    if (!level || !pos || !stats || !workspace || !swd_patches_ok(n, C, H, P)) return GZ_ERR_BAD_SHAPE;
    if (ws_bytes < gz_swd_channel_stats_workspace_bytes(n, C, H, P)) return GZ_ERR_WORKSPACE;
    const SwdPatches p{level, pos, (long long)n * P, C, H, P};
    const int blocks = swd_stats_blocks(p.rows);
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(swd_stats_kernel, dim3((unsigned)blocks), dim3(SWD_STATS_THREADS), 0, stream, p, part);
    const int rc = launch_status();
    if (rc != GZ_OK) return rc;
    hipLaunchKernelGGL(swd_stats_finish_kernel, dim3(1), dim3(64), 0, stream, p, (const double*)part, blocks, stats);
    return launch_status();
}

int gz_swd_sort_plan(long long rows, int* block, long long* padded, int* block_passes, int* global_passes) {
    SortPlan p;
    if (!block || !padded || !block_passes || !global_passes || !swd_sort_plan(rows, p)) return GZ_ERR_BAD_SHAPE;
    *block = SORT_BLOCK;
    *padded = p.padded;
    *block_passes = p.block_passes;
    *global_passes = p.global_passes;
    return GZ_OK;
}

int gz_swd_project(const float* level, int n, int C, int H, const int* pos, int P, const double* stats, const float* dirs,
                   int ndirs, float* proj, long long pitch, hipStream_t stream) {
    gz::clear_stale_error();
    if (!level || !pos || !stats || !dirs || !proj || ndirs < 1 || !swd_patches_ok(n, C, H, P)) return GZ_ERR_BAD_SHAPE;
    SortPlan sp;
    const SwdPatches p{level, pos, (long long)n * P, C, H, P};
    if (!swd_sort_plan(p.rows, sp) || pitch < sp.padded) return GZ_ERR_BAD_SHAPE;
    const long long tiles = (p.rows + SWD_PROJ_ROWS - 1) / SWD_PROJ_ROWS, gy = (ndirs + SWD_PROJ_DIRS - 1) / SWD_PROJ_DIRS;
    const long long gx = tiles < SWD_PROJ_MAX_GRID ? tiles : SWD_PROJ_MAX_GRID;
    if (gy > 65535) return GZ_ERR_TOO_LARGE;
    hipLaunchKernelGGL(swd_project_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(SWD_PROJ_THREADS), 0, stream, p, stats,
                       dirs, ndirs, proj, pitch, sp.padded);
    return launch_status();
}

int gz_swd_sort_columns(float* data, long long rows, int cols, long long pitch, hipStream_t stream) {
    gz::clear_stale_error();
    SortPlan p;
    if (!data || cols < 1 || !swd_sort_plan(rows, p) || pitch < p.padded || pitch % 4 != 0 ||
        (reinterpret_cast<uintptr_t>(data) & 15) != 0)
        return GZ_ERR_BAD_SHAPE;
    if (cols > 65535 || p.padded / SORT_BLOCK > 0x7fffffffll) return GZ_ERR_TOO_LARGE;
    const long long blocks = p.padded <= SORT_BLOCK ? 1 : p.padded / SORT_BLOCK;
    const long long first = p.padded < SORT_BLOCK ? p.padded : SORT_BLOCK;
    int rc;
    hipLaunchKernelGGL(swd_sort_block_kernel, dim3((unsigned)blocks, (unsigned)cols), dim3(SORT_THREADS), 0, stream, data,
                       rows, p.padded, pitch, 2ll, first);
    if ((rc = launch_status()) != GZ_OK) return rc;
    for (long long k = 2ll * SORT_BLOCK; k <= p.padded; k <<= 1) {
        // the phase's strides k / 2 .. SORT_BLOCK, two to a pass while two are left
        for (long long j = k / 2; j >= SORT_BLOCK;) {
            const bool two = j / 2 >= SORT_BLOCK;
            const long long threads = two ? p.padded / 16 : p.padded / 8;
            const dim3 grid((unsigned)((threads + SORT_GLOBAL_THREADS - 1) / SORT_GLOBAL_THREADS), (unsigned)cols);
            if (two)
                hipLaunchKernelGGL(swd_sort_global2_kernel, grid, dim3(SORT_GLOBAL_THREADS), 0, stream, data, p.padded, pitch,
                                   k, j);
            else
                hipLaunchKernelGGL(swd_sort_global_kernel, grid, dim3(SORT_GLOBAL_THREADS), 0, stream, data, p.padded, pitch,
                                   k, j);
            if ((rc = launch_status()) != GZ_OK) return rc;
            j >>= two ? 2 : 1;
        }
        // (the keys at or beyond `rows` are +inf in memory by now: the first pass wrote them)
        hipLaunchKernelGGL(swd_sort_block_kernel, dim3((unsigned)blocks, (unsigned)cols), dim3(SORT_THREADS), 0, stream,
                           data, p.padded, p.padded, pitch, k, k);
        if ((rc = launch_status()) != GZ_OK) return rc;
    }
    return GZ_OK;
}

size_t gz_swd_distance_workspace_bytes(long long rows, int cols_per_repeat, int repeats) {
    if (rows < 1 || cols_per_repeat < 1 || repeats < 1 || (long long)cols_per_repeat * repeats > 65535) return 0;
    return (size_t)swd_dist_chunks(rows) * cols_per_repeat * repeats * sizeof(double);
}

int gz_swd_distance(const float* a, long long rows_a, const float* b, long long rows_b, int cols_per_repeat, int repeats,
                    long long pitch, double* out, void* workspace, size_t ws_bytes, hipStream_t stream) {
    gz::clear_stale_error();
    if (!a || !b || !out || !workspace || rows_a < 1 || rows_a != rows_b || cols_per_repeat < 1 || repeats < 1 ||
        pitch < rows_a)
        return GZ_ERR_BAD_SHAPE;
    const long long chunks = swd_dist_chunks(rows_a), cols = (long long)cols_per_repeat * repeats;
    if (cols > 65535 || chunks > 0x7fffffffll) return GZ_ERR_TOO_LARGE;
    if (ws_bytes < gz_swd_distance_workspace_bytes(rows_a, cols_per_repeat, repeats)) return GZ_ERR_WORKSPACE;
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(swd_distance_kernel, dim3((unsigned)chunks, (unsigned)cols), dim3(SWD_DIST_THREADS), 0, stream, a, b,
                       rows_a, pitch, part);
    const int rc = launch_status();
    if (rc != GZ_OK) return rc;
    hipLaunchKernelGGL(swd_distance_finish_kernel, dim3((unsigned)repeats), dim3(SWD_DIST_THREADS), 0, stream,
                       (const double*)part, chunks * cols_per_repeat, out);
    return launch_status();
}

}  // extern "C"
