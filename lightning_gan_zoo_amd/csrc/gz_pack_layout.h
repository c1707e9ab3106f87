// The layout of the packed weight images: what the packers (gz_pack.hip) write and what the launchers that read them
// (gz_conv_{fwd,dgrad,wgrad}.hip, gz_conv_direct.hip, the loaders of gz_igemm_loaders.h) must agree on -- the reduction chunk the images
// are padded to, the taps of a transposed convolution's phase, and the rules that make an image tap-major.
#pragma once
#include "gz_common.h"
#include "gz_knobs.h"

namespace gz {

constexpr int BK = 16;
// number of kernel taps k = ((parity + P) % S) + S*t below KS that a transposed-conv output phase of that parity has
__host__ __device__ constexpr int dg_taps(int KS, int S, int P, int parity) {
    return (KS - ((parity + P) % S) + S - 1) / S;
}

constexpr int round_bk(int v) { return (v + BK - 1) / BK * BK; }
__host__ __device__ constexpr int round4(int v) { return (v + 3) & ~3; }

// Tap-major reduction order (gz_igemm_loaders.h: the TapGeo* geometries under TapGatherLoader / TapGatherA2) is used
// when the tap count does not divide a chunk (3x3, 5x5) and there are enough channels to fill the BK-wide channel blocks.
inline bool fwd_tap_major(int C, int KH, int KW) {
    return !knobs().no_tapmajor && (BK % (KH * KW) != 0) && C >= BK;
}

inline bool dgrad_tap_major(int K, int KH, int KW, int S) {
    const bool off = knobs().no_tapmajor;
    const int taps = ((KH + S - 1) / S) * ((KW + S - 1) / S);
    const bool fixed = (KH % S == 0) && (KW % S == 0) && (BK % taps == 0);
    return !off && !fixed && K >= BK;
}

}  // namespace gz
