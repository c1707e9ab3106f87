// What gz_conv_fwd.hip calls of gz_conv_fwd_igemm.hip.  The forward family is the largest of the three, so its launchers
// are two units by skeleton: the igemm2 launchers stay with launch_fwd and the entry points, the igemm_kernel launchers
// (run_fwd, run_fwd_any) are reached through the two functions below.  Neither decides anything: the tile, the loader
// and the splits are the Choice's (gz_conv2d_choose.h).
#pragma once
#include "gz_conv2d_choose.h"

namespace gz {

// a forward Choice whose tile is one of the four igemm_kernel tiles (instantiated for the geometries of GZ_GEOM_DISPATCH)
template <class G>
int launch_fwd_igemm(const Choice& c, const float* x, const float* wp, const float* bias, float* y, const ConvShape& s,
                     int act, float slope, float* slab, float* stats, hipStream_t st);

// run-time geometry (gz_conv2d_fwd_any) on the igemm_kernel tile `sp.tile`
int launch_fwd_any_igemm(const SplitPlan& sp, const float* x, const float* wp, const float* bias, float* y,
                         const ConvShape& s, const AnyGeom& g, int act, float slope, float* slab, hipStream_t st);

}  // namespace gz
