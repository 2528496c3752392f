// What every MFMA header shares: vector types, the workgroup's shape, the prefetch distance, the compile-time loop and the
// tuning switches of the kernel (one block, below).
#pragma once
#include "nwe_host.h"

namespace nwe {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

#define LDS_AS __attribute__((address_space(3)))

constexpr int PD = 3;   // A fragments are read PD k-steps ahead of their MFMAs
// A LONG chunk (>= 16 k-steps, three-pass mode) has at least this many pieces per wave; it keeps the (hi, lo) tiles of its last
// k-step in a rotating tail slot instead of the chunk buffer, see Walker.
constexpr int kLongPieces = 8;

// ---- tuning switches ----------------------------------------------------------------------------------------------
// Every source-level switch of the MFMA kernel: default, meaning, recorded measurement.  The code reads the constants;
// `make variant NAME=x VFLAGS=-DNWE_DMA_STRIDE=1` builds the other arm of one.
#ifndef NWE_DMA_STRIDE
#define NWE_DMA_STRIDE 2   // DMA pieces go out every SECOND k-step where the tile is long enough (DmaPlan has the measurement); 1 = every k-step
#endif
#ifndef NWE_SPREAD_BIAS
#define NWE_SPREAD_BIAS 1   // the tile's four bias reads ride in the third gaps of k-steps 1..4 instead of all at its start: -0.25 % (375.5 vs 376.5 ms, alternating)
#endif
#ifndef NWE_ONE_WAIT
#define NWE_ONE_WAIT 1   // both fragments of the k-step are "used" in front of its first MFMA, so hipcc waits for them once (lgkmcnt)
#endif                   // instead of once per MFMA that consumes one: 16 fewer s_waitcnt per long tile, -0.35 % (372.2 vs 373.5 ms); 0 = off
#ifndef NWE_SPLIT_READS
#define NWE_SPLIT_READS 1   // the lo fragment is read in the k-step's THIRD gap, not beside the hi fragment: -0.45 % (362.4 vs 364.1 ms, alternating); 0 = both behind the first MFMA
#endif
#ifndef NWE_PEEL_SKIP
#define NWE_PEEL_SKIP 1   // the pair that takes gamma(x) is peeled out of the rolled loop: no run-time use_g tests inside the tiles (6 branches per tile of every first-of-pair layer), +16 tiles of code (110 KB): -0.8 % (364.4 vs 367.2 ms, alternating); 0 = one rolled loop
#endif
#ifndef NWE_COARSE_DENSITY_ONLY
#define NWE_COARSE_DENSITY_ONLY 1   // density-only coarse evaluations in lean frames (mlp_eval); 0 = every evaluation runs the view layer and rgb head
#endif
#ifndef NWE_COLOUR_SKIP
#define NWE_COLOUR_SKIP 1   // the hollow path of lean evaluations whose ray packet has no density (mlp_eval); 0 = not built.  The run-time switch is nwe_debug_set_colour_skip
#endif
// Cache policy of the weight stream (NWE_GLDS_POLICY, timing experiments): 0 default, 1 sc1 (bypass the CU's vector L1, which
// never sees a piece twice), 2 nt, 3 sc0 sc1, 4 sc1 nt.  It is spliced into an instruction string, so it stays a macro.
#ifndef NWE_GLDS_POLICY
#define NWE_GLDS_POLICY 0
#endif
#if NWE_GLDS_POLICY == 1
#define NWE_GLDS_POL " sc1"
#elif NWE_GLDS_POLICY == 2
#define NWE_GLDS_POL " nt"
#elif NWE_GLDS_POLICY == 3
#define NWE_GLDS_POL " sc0 sc1"
#elif NWE_GLDS_POLICY == 4
#define NWE_GLDS_POL " sc1 nt"
#else
#define NWE_GLDS_POL ""
#endif
constexpr int kDmaStride = NWE_DMA_STRIDE;
constexpr bool kSpreadBias = NWE_SPREAD_BIAS != 0, kOneWait = NWE_ONE_WAIT != 0, kSplitReads = NWE_SPLIT_READS != 0;
constexpr bool kPeelSkip = NWE_PEEL_SKIP != 0, kCoarseDensityOnly = NWE_COARSE_DENSITY_ONLY != 0, kColourSkip = NWE_COLOUR_SKIP != 0;
// -DNWE_STAMPS (`make stamps`): a DIAGNOSTIC build with in-kernel s_memtime stamps; NWE_STAMP(...) is its code, nothing otherwise.
#ifdef NWE_STAMPS
#define NWE_STAMP(...) __VA_ARGS__
#else
#define NWE_STAMP(...)
#endif
// Timing ablations of `make ablate` (results are garbage, only the cycle stamps mean anything): -DNWE_EXP_NODMA = no LDS-DMA
// pieces, -DNWE_EXP_NOSYNC = no per-tile wait and barrier, -DNWE_EXP_NOEPI = no epilogue at all.  Compile-time, because a
// run-time test would split every k-step into its own basic block.
#ifdef NWE_EXP_NODMA
constexpr bool kExpNoDma = true;
#else
constexpr bool kExpNoDma = false;
#endif
#ifdef NWE_EXP_NOSYNC
constexpr bool kExpNoSync = true;
#else
constexpr bool kExpNoSync = false;
#endif
#ifdef NWE_EXP_NOEPI
constexpr bool kExpNoEpi = true;
#else
constexpr bool kExpNoEpi = false;
#endif

// Compile-time loop: f(integral_constant<int, I>) for I in [I0, N).
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

}  // namespace nwe
