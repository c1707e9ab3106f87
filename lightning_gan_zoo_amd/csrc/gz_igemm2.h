// Part of the fp32 implicit-GEMM core (see gz_igemm.h), igemm2 skeleton: tile configuration, ring depth and barrier interval
// per instantiation, LDS sizes.
#pragma once
#include "gz_igemm_core.h"

namespace gz {

constexpr int STAGES2 = 3;      // igemm2w_kernel's ring, and the default depth of igemm2_kernel's (igemm2_depth below)
// Ring depth of igemm2_kernel per instantiation.  The three stages were sized for the 128 x 128 wave tile: 128 MFMAs
// = 8192 cycles per chunk, a prefetch distance of two chunks.  The 128 x 32 wave tile (TN = 1) has 2048 cycles per
// chunk.  Depth D (barrier interval 1): the prologue issues chunks 0 .. D-2 and waits for chunk 0, chunk t+D-1 is issued
// during chunk t into the stage chunk t-1 was read from, and the counted wait of chunk t leaves (D-2) * NP pieces in
// flight.  The candidates are compared with -D builds of the library.  Measured: at three stages the
// counted wait never waits, depth 4 and 5 change nothing; what the TN = 1 loop loses it loses at the barrier, so what
// ships for TN = 1 is the barrier interval below with the stages it needs (6 = three pairs, or 4 = two pairs where
// three workgroups share the CU's LDS), and TN = 2 keeps 3 / 1.
// tests/test_igemm2_ring_gpu.py reads the four TN1 #defines below and sizes its cases around them.
#ifndef GZ2_DEPTH_TN1_KG2
#define GZ2_DEPTH_TN1_KG2 6
#endif
#ifndef GZ2_DEPTH_TN1_KG1
#define GZ2_DEPTH_TN1_KG1 4
#endif
#ifndef GZ2_DEPTH_TN2_KG2
#define GZ2_DEPTH_TN2_KG2 3
#endif
#ifndef GZ2_DEPTH_TN2_KG1
#define GZ2_DEPTH_TN2_KG1 3
#endif
// Barrier interval of the same instantiations: chunks per counted wait + s_barrier.  With interval 2 the ring is handled
// in PAIRS of stages -- the loop body is two chunks (16 k-steps, 64 MFMAs per wavefront at TN = 1: what the skeleton was
// sized for), the depth counts pairs' stages (a multiple of 2), the pieces of pair p+P-1 are issued during pair p.
#ifndef GZ2_BARRIER_TN1_KG2
#define GZ2_BARRIER_TN1_KG2 2
#endif
#ifndef GZ2_BARRIER_TN1_KG1
#define GZ2_BARRIER_TN1_KG1 2
#endif
constexpr uint32_t SOFF_OOB = 0x80000000u;      // scalar offset that puts every lane of a buffer access out of range

template <int WM_, int WN_, int TN_, int OCC_, int TM_ = 4>
struct TileCfg2 {
    static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_, OCC = OCC_;    // OCC: workgroups per CU (= waves / SIMD)
    static constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    static_assert(WM * WN == 4, "4 wavefronts per workgroup, one per SIMD");
};

// Stages of the LDS-DMA ring (see GZ2_DEPTH_* above): deeper than three only for the 16-byte row loaders of the k4 s2 p1
// layers on 256-row tiles (8 LDS rows per A image: a stage is 12-17 KB), where the LDS is there -- the gathers' stages
// are 20 KB and more and keep three.
constexpr size_t LDS_PER_CU = 160 * 1024;
template <class AL, class BL>
constexpr int igemm2_stage_floats() { return AL::ROWS * AL::LD + AL::EXTRA + BL::ROWS * BL::LD; }
// LDS of a workgroup whose ring(s) have `depth` stages (KG = 2: two rings, or the parked accumulators if those are larger)
template <class Cfg, class AL, class BL, int KG>
constexpr size_t igemm2_lds_bytes_at(int depth) {
    if (KG == 1) return (size_t)(depth * igemm2_stage_floats<AL, BL>() + 32) * 4;
    const size_t rings = (size_t)(2 * ((depth * igemm2_stage_floats<AL, BL>() + 63) / 64 * 64) + 32) * 4;
    const size_t park = (size_t)Cfg::TM * Cfg::TN * 16 * NT * 4;
    return rings > park ? rings : park;
}
// The instantiations GZ2_DEPTH_* / GZ2_BARRIER_* speak of.  One exception, explicit: ConvFwdA2 with 64 output columns
// per row (its zeroed region is 388 floats per stage) fits neither six stages in two rings nor four stages three times
// into a CU's LDS and keeps 3 / 1.  Nothing else is lowered behind a -D build's back: igemm2_kernel asserts that what
// these return fits.
template <class Cfg, class AL, class BL, int KG>
constexpr bool igemm2_tunable() {
    return Cfg::BM == 256 && (AL::ROWSHARE || AL::FWDROWS) && !AL::DUALMODE && AL::OW_C < 64;
}
template <class Cfg, class AL, class BL, int KG>
constexpr int igemm2_interval() {      // chunks per counted wait + barrier
    if (igemm2_tunable<Cfg, AL, BL, KG>() && Cfg::TN == 1) return KG == 2 ? GZ2_BARRIER_TN1_KG2 : GZ2_BARRIER_TN1_KG1;
    return 1;
}
template <class Cfg, class AL, class BL, int KG>
constexpr int igemm2_depth() {         // stages of the ring (a multiple of the interval)
    if (igemm2_tunable<Cfg, AL, BL, KG>()) {
        if (Cfg::TN == 1) return KG == 2 ? GZ2_DEPTH_TN1_KG2 : GZ2_DEPTH_TN1_KG1;
        if (Cfg::TN == 2) return KG == 2 ? GZ2_DEPTH_TN2_KG2 : GZ2_DEPTH_TN2_KG1;
    }
    return STAGES2;
}
template <class Cfg, class AL, class BL, int KG>
constexpr int igemm2_ring_floats() {
    return ((igemm2_depth<Cfg, AL, BL, KG>() * igemm2_stage_floats<AL, BL>() + 63) / 64) * 64;
}
template <class Cfg, class AL, class BL>
constexpr size_t igemm2_lds_bytes() { return igemm2_lds_bytes_at<Cfg, AL, BL, 1>(igemm2_depth<Cfg, AL, BL, 1>()); }
template <class Cfg, class AL, class BL>
constexpr size_t igemm2_lds_bytes_kg2() { return igemm2_lds_bytes_at<Cfg, AL, BL, 2>(igemm2_depth<Cfg, AL, BL, 2>()); }

}  // namespace gz
