// The vocabulary of a launch choice, shared by gz_conv.hip (conv2d) and gz_conv3d.hip (conv3d): tile configurations and
// their ids, skeleton kinds, loaders, the facts only a call knows, and the Choice the choose_* functions of both files
// return.  choose_* answers "which kernel does this launch take" once per op: launch_* switch on the answer, the
// workspace sizes are read from it, gz_conv2d_plan / gz_conv3d_plan print it.
#pragma once
#include "gz_igemm.h"

namespace gz {

using Cfg128x128 = TileCfg<2, 2, 2, 2>;
using Cfg128x64 = TileCfg<2, 2, 2, 1>;
using Cfg128x32 = TileCfg<4, 1, 1, 1>;
using Cfg64x64 = TileCfg<2, 2, 1, 1>;

// round 3 (gz_igemm.h, igemm2): one wavefront per SIMD, 128x128 / 128x64 accumulators per wavefront
using Cfg256x256 = TileCfg2<2, 2, 4, 1>;
using Cfg256x128 = TileCfg2<2, 2, 2, 2>;
using Cfg512x64 = TileCfg2<4, 1, 2, 2>;       // 64 output channels in all (D.block1-size input gradients)
using Cfg128x256 = TileCfg2<1, 4, 2, 2>;      // weight gradient with 128 output channels
// round 4: 256 x 64 (wavefronts 2 x 2 of 128 x 32, 64 accumulator registers): twice the tiles of 256x128 for launches
// that would otherwise put one workgroup on a CU or split their reduction; three workgroups per CU (37-42 KB of LDS)
using Cfg256x64 = TileCfg2<2, 2, 1, 3>;

enum TileId { T128x128 = 0, T128x64 = 1, T128x32 = 2, T64x64 = 3, T256x256 = 4, T256x128 = 5, T512x64 = 6, T128x256 = 7,
              T256x64 = 8,
              T256x128P = 9 };   // (a label only: ConvDg5A2's 256 pixels x (2 column phases x 64 channels), gz_conv2d_tile)
inline bool is_tile2(TileId t) { return t >= T256x256; }

inline const char* tile_text(TileId t) {
    switch (t) {
        case T128x128: return "128x128";
        case T128x64: return "128x64";
        case T128x32: return "128x32";
        case T64x64: return "64x64";
        case T256x256: return "256x256";
        case T256x128: return "256x128";
        case T512x64: return "512x64";
        case T256x64: return "256x64";
        case T256x128P: return "256x(4x32)";
        default: return "128x256";
    }
}

enum Kind { KUnsupported, KDirect, KIgemm, KIgemm2, KIgemm2w, KIgemm2r, KDg5 };
enum Loader {
    LGeneric,       // the skeleton's element-wise loaders (ConvFwdALoader / K4V, ConvDgALoader, WgALoader + WgBLoader)
    LTap,           // igemm: tap-major reduction
    LRow4,          // igemm: the k4 s2 p1 row loaders (16-byte pieces)
    LWgRow,         // igemm Wg: whole row segments (WgALoaderRow + WgBLoaderRow)
    LRows2,         // igemm2: the geometry's own raw-row loaders (ConvFwdA2 / ConvDgA2)
    LGather2,       // igemm2: ConvTapA2 / ConvDgTapA2 (conv3d: Conv3DTapA2 / Conv3DDgTapA2)
    LPlane2,        // igemm2: 1x1 as a plain GEMM (PlaneA2)
    LFewk,          // direct 3x3 kernels for <= 4 output channels
    LSmallch,       // direct 3x3 MFMA 16x16x4 kernels
    LSmallc,        // direct k4 s2 p1 Dg onto <= 4 channels (ks == 0: the one-position kernel)
    LSmallc5,       // ... 5x5 s2 p2
    LFewc           // direct k4 s2 p1 Wg with <= 4 image channels
};
// what the planner cannot know from the shape; `in` is what the A loader reads (x for F, y for Dg, both operands for Wg)
struct Facts {
    bool in16, out16, out8;      // alignment of the tensors
    size_t ws_bytes;             // workspace available (0: none)
    bool epilogue;               // a bias or an activation is present
    bool stats;                  // BatchNorm statistics are requested: no direct kernel carries them
    bool in4;                    // `in` is 4-byte aligned (the 4-byte LDS-DMA gathers of conv3d's forward ask)
};
// 16-byte aligned tensors, a workspace of the advertised size, no bias / activation: what gz_conv*_plan describes
static const Facts kIdeal{true, true, true, ~(size_t)0, false, false, true};
inline Facts facts_of(const void* in, const void* out, const void* ws, size_t ws_bytes, bool epilogue, bool stats) {
    return Facts{((uintptr_t)in & 15) == 0, ((uintptr_t)out & 15) == 0, ((uintptr_t)out & 7) == 0, ws ? ws_bytes : 0,
                 epilogue, stats, ((uintptr_t)in & 3) == 0};
}
struct Choice {
    Kind kind;
    Loader loader;
    TileId tile;
    int splits;          // reduction splits asked of the launcher (a transposed conv3d: of its longest phase)
    int slabs;           // z-slices (workspace slabs) that gives (a transposed conv3d: summed over the phases)
    int ks, cw;          // LSmallc / LSmallc5: wavefronts sharing the channel loop; igemm2w: pixel-chunk width
    int wave_groups;     // igemm2: 2 when the launcher runs two wave groups per workgroup
    bool ws_short;       // the plan wanted slabs the workspace cannot hold (what follows is the op's: see launch_*)
};
inline Choice choice_of(Kind kind, Loader loader, TileId tile) { return Choice{kind, loader, tile, 1, 1, 0, 0, 1, false}; }
// a split plan needs a workspace: none at all, or one smaller than `need`, and the launch does not run split
inline bool ws_lacks(const Facts& f, size_t need) { return f.ws_bytes == 0 || f.ws_bytes < need; }
// a weight gradient writes one slab of `count` floats per split: as many splits as the workspace holds, unsplit below 2
inline int wg_fit_splits(int splits, size_t ws_bytes, long long count) {
    if (splits <= 1) return splits;
    const long long max_splits = (long long)(ws_bytes / 4) / count;
    return max_splits < 2 ? 1 : (splits > max_splits ? (int)max_splits : splits);
}

}  // namespace gz
