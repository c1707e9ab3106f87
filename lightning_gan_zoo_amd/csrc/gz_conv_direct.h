// What the conv2d dispatcher (choose_*: gz_conv2d_choose.h; launch_*: gz_conv_{fwd,dgrad,wgrad}.hip) calls of the direct kernels (gz_conv_direct.hip): per family the predicate that
// admits a shape, the sizing helper whose answer goes into the Choice or the workspace size, and the launcher.  The
// kernels, their templates and the switches over their template parameters stay on the other side.
#pragma once
#include "gz_conv_choice.h"

namespace gz {

// Dg onto <= 4 image channels: k4 s2 p1 (ks = smallc_split(...): the four-positions kernel, ks = 0: one position per
// lane; mask: the fused activation backward of gz_conv2d_dgrad_act) and 5x5 s2 p2
bool smallc_four_pos(const ConvShape& s);
bool dgrad_direct5_ok(const ConvShape& s);
int smallc_split(long long M4, int K);
int run_dgrad_smallc(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act, float slope,
                     hipStream_t st, int ks, const float* mask = nullptr, float mask_neg = 0.f);
int run_dgrad_smallc5(const float* y, const float* wp, const float* bias, float* x, const ConvShape& s, int act, float slope,
                      hipStream_t st, int ks);

// F / Dg of 3x3 s1 p1 layers with few channels (ld: LFewk or LSmallch)
bool conv3_fewk_ok(int CI, int CO, int H, int W);
bool conv3_smallch_ok(int N, int CI, int CO, int H, int W);
int run_conv3_smallch(const float* in, const float* wp, const float* bias, float* out, int N, int CI, int CO, int H, int W,
                      int tap_major, int flip, int act, float slope, hipStream_t st, Loader ld);

// Wg of 3x3 s1 p1 layers with few channels (ld: LFewk or LSmallch; wgrad_smallch_blocks: slab rows of either)
bool wgrad_fewk_ok(const ConvShape& s);
bool wgrad_smallch_ok(const ConvShape& s, int KH, int KW, int S, int P);
int wgrad_smallch_blocks(const ConvShape& s);
int run_wgrad_smallch(const float* x, const float* y, float* dw, float* dbias, float* ws, size_t ws_bytes, const ConvShape& s,
                      Loader ld, hipStream_t st);

// Wg of k4 s2 p1 layers with <= 4 image channels (fwd_out != nullptr: the fused activation-backward form)
bool wgrad_k4s2p1_fewc_ok(const ConvShape& s);
int wgrad_k4s2p1_fewc_blocks(const ConvShape& s);
int run_wgrad_k4s2p1_fewc(const float* x, const float* y, const float* fwd_out, int act, float slope, float* dw, float* ws,
                          size_t ws_bytes, const ConvShape& s, hipStream_t st);

}  // namespace gz
