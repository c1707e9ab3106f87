// fp32 implicit-GEMM core for gfx950: v_mfma_f32_32x32x2_f32 tiles fed from LDS.
//
//   C[m][n] = sum_k A[m][k] * B[k][n]
//
// One 256-thread workgroup (4 wavefronts of 64) owns a BM x BN tile of C.  K is
// walked in chunks of BK=16.  Both operands live in LDS as [k][mn] images with
// the M/N index contiguous: lane l of a wave feeds the MFMA with
//   A[m = l&31][k = l>>5]   and   B[k = l>>5][n = l&31]
// (one dword each), so a fragment read is a conflict-free ds_read_b32 of 32
// consecutive words per half-wave and NCHW's pixel-contiguity maps straight onto
// the M (forward / dgrad) or K (wgrad) axis without any transposition in HBM.
//
// Staging is global -> VGPR -> LDS, software pipelined over two LDS buffers: the
// loads of chunk t+1 are issued before the MFMAs of chunk t and written to the
// other buffer after them; one barrier per chunk.  Loads are raw buffer loads:
// out-of-image taps / tails get a voffset >= num_records and read as 0 without
// a branch.  fp32-input MFMA runs at 256 FLOP/clk/CU (= 157 TF peak), i.e. a
// 128x128x16 chunk takes 2048 clk/CU, which leaves the memory pipeline ~8 B/clk/CU
// to fill -- the loaders are deliberately simple.
//
// "Loader" concept (A or B operand):
//   struct Params;  static constexpr int LD;        // LDS leading dimension
//   void init(const Params&, int tile, int y, int tid);
//   void issue(int chunk);                          // global -> registers
//   void commit(float* lds);                        // registers -> lds[k*LD + mn]
// "Epilogue" concept:
//   struct Params;
//   void store(const Params&, acc, m_base, n_base, lane, y, z);
//
// The core is split by role (one 3.7 k-line file before round 5), this header being the one the .hip units include:
//   gz_igemm_loaders.h    primitives (raw buffer loads, LDS-DMA), TileCfg, LoaderDefaults, the round-1/2 operand loaders
//   gz_igemm_epilogues.h  epilogues of both skeletons
//   gz_igemm_core.h       GridMap, what the four launchers share (make_grid, launch_big_lds, the split-K finish pass),
//                         igemm_kernel (rounds 1-2) and launch_igemm
// the igemm2 skeleton (rounds 3-6):
//   gz_igemm2.h           TileCfg2, ring depth / barrier interval per instantiation, LDS sizes
//   gz_igemm2_loaders.h   the LDS-DMA loaders of igemm2_kernel
//   gz_igemm2_kstep.h     k-step primitives (LDS reads, MFMA rows, waits), static_for, the stamp probe and GZ2_EXP_* switches
//   gz_igemm2_kernel.h    igemm2_kernel, the KG = 2 rules, launch_igemm2
//   gz_igemm2_wg.h        the weight-gradient kernels igemm2r / igemm2w, their loaders and launchers
#pragma once
#include "gz_igemm2_kernel.h"
#include "gz_igemm2_wg.h"

namespace gz {

// the tile configurations the convolution dispatchers launch (their ids: TileId, gz_conv_choice.h)
using Cfg128x128 = TileCfg<2, 2, 2, 2>;
using Cfg128x64 = TileCfg<2, 2, 2, 1>;
using Cfg128x32 = TileCfg<4, 1, 1, 1>;
using Cfg64x64 = TileCfg<2, 2, 1, 1>;

// round 3 (igemm2, gz_igemm2_kernel.h): one wavefront per SIMD, 128x128 / 128x64 accumulators per wavefront
using Cfg256x256 = TileCfg2<2, 2, 4, 1>;
using Cfg256x128 = TileCfg2<2, 2, 2, 2>;
using Cfg512x64 = TileCfg2<4, 1, 2, 2>;       // 64 output channels in all (D.block1-size input gradients)
using Cfg128x256 = TileCfg2<1, 4, 2, 2>;      // weight gradient with 128 output channels
// round 4: 256 x 64 (wavefronts 2 x 2 of 128 x 32, 64 accumulator registers): twice the tiles of 256x128 for launches
// that would otherwise put one workgroup on a CU or split their reduction; three workgroups per CU (37-42 KB of LDS)
using Cfg256x64 = TileCfg2<2, 2, 1, 3>;

}  // namespace gz
