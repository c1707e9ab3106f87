// The vocabulary of a launch choice, shared by conv2d (gz_conv2d_choose.h and the units that read it), its direct kernels (gz_conv_direct.hip) and
// gz_conv3d.hip (conv3d): tile ids, skeleton kinds, loaders, the facts only a call knows, and the Choice the choose_*
// functions of both dispatchers return.  choose_* answers "which kernel does this launch take" once per op: launch_*
// switch on the answer, the workspace sizes are read from it, gz_conv2d_plan / gz_conv3d_plan print it.  Plain host
// data: no skeleton is included here (the tile configurations the ids stand for are in gz_igemm.h).
#pragma once
#include "gz_common.h"

namespace gz {

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
    LTap,           // igemm: tap-major reduction (TapGatherLoader over the form's TapGeo*: Conv*ALoaderTap)
    LRow4,          // igemm: the k4 s2 p1 row loaders (16-byte pieces)
    LWgRow,         // igemm Wg: whole row segments (WgALoaderRow + WgBLoaderRow)
    LRows2,         // igemm2: the geometry's own raw-row loaders (ConvFwdA2 / ConvDgA2)
    LGather2,       // igemm2: TapGatherA2 over the same geometries: ConvTapA2 / ConvDgTapA2 (conv3d: Conv3DTapA2 / Conv3DDgTapA2)
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


// what every conv2d entry point checks of its arguments before it chooses
inline bool shape_ok(const ConvShape& s, int KH, int KW, int S, int P) {
    if (s.N <= 0 || s.C <= 0 || s.K <= 0 || s.H <= 0 || s.W <= 0) return false;
    if (s.OH != (s.H + 2 * P - KH) / S + 1 || s.OW != (s.W + 2 * P - KW) / S + 1) return false;
    return true;
}

inline bool too_large(long long elems) { return elems * 4 >= (1ll << 31); }

}  // namespace gz
