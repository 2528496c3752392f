// The deferred epilogue of a 32-row tile: bias, ReLU, fp16 hi/lo split into the next layer's B fragments, staged into the
// MFMA gaps of the following tile (see nwe_mfma_kernels.h for the design).
#pragma once
#include "nwe_mfma_config.h"

namespace nwe {

// A 32-row tile whose accumulator is complete but whose epilogue (scale, bias, ReLU, fp16 hi/lo split into the B
// fragments of the next layer) has not run yet.  The epilogue of tile t is issued piecewise BETWEEN the MFMAs of
// tile t+1 (a wave issues in order: VALU placed between two MFMAs executes while the matrix pipe works), so two
// of these alternate.  The bias is read when the tile starts and consumed one tile later, which also keeps its
// LDS latency off the MFMA chain.
struct Pend {
    f16v a;
    float4 bias[4];   // register 4g+i holds row 8g + 4h + i -> bias[g].{x,y,z,w}
};

// ReLU (lower = 0) or pass-through (lower = -inf) of an activation that KEEPS a NaN: v_maximum3_f32, one instruction like the
// v_max_f32 of fmaxf, which returns the other operand for a NaN.  An activation >= 65520 has hi = fp16(v) = inf and a NaN
// residual product in the next layer's accumulators; with fmaxf that NaN became a finite, wrong 0.  Kept, it reaches the raw
// outputs and the NWE_FLAG_* bits (include/nwe.h, "fp16 range").
__device__ __forceinline__ float act(float v, float lower) { return __builtin_elementwise_maximum(v, lower); }

__device__ __forceinline__ float pend_bias(const Pend& t, int r) {
    const float4 b = t.bias[r >> 2];
    return (r & 3) == 0 ? b.x : ((r & 3) == 1 ? b.y : ((r & 3) == 2 ? b.z : b.w));
}
__device__ __forceinline__ float pend_value(const Pend& t, int r, float inv_scale) { return __builtin_fmaf(t.a[r], inv_scale, pend_bias(t, r)); }

// Residuals v - hi of a packed fp16 pair hw = (fp16(v0), fp16(v1)) as fma(hi, -1, v) with the fp16 half read in place:
// v_fma_mix_f32 instead of v_cvt_f32_f16 + v_sub_f32 (same single rounding).  hipcc does not select it from C (it folds the -1
// into a subtraction first), hence the asm.
__device__ __forceinline__ void residual_pair(uint32_t hw, float v0, float v1, float& r0, float& r1) {
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hw), "v"(v0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hw), "v"(v1));
}

// Epilogue of a pending tile: v = max(acc/scale + bias, lower), hi = fp16(v), lo = fp16(v - hi); register r of the tile
// is element r&7 of the (r>>3)-th of its two output k-steps.  This is the FALLBACK form, one element per call (every
// second call packs a pair), used only by tiles too short for the staged plan below (EpiPlan::STAGED == false).
template <bool X3, bool DOT = false>
__device__ __forceinline__ void finish_elem(const Pend& t, int e, float inv_scale, float lower, float& keep, h8& hi0, h8& lo0,
                                            h8& hi1, h8& lo1, const float* dotw = nullptr, float* dot = nullptr) {
    const float v = act(pend_value(t, e, inv_scale), lower);
    if (DOT) *dot = __builtin_fmaf(dotw[8 * (e >> 2) + (e & 3)], v, *dot);   // dotw already points at this lane half's rows
    if ((e & 1) == 0) { keep = v; return; }
    const float v0 = keep, v1 = v;
    h2 hp;
    hp[0] = (_Float16)v0; hp[1] = (_Float16)v1;                        // one v_cvt_pk_f16_f32
    const _Float16 h0 = hp[0], h1 = hp[1];
    _Float16 l0 = (_Float16)0.f, l1 = (_Float16)0.f;
    if (X3) {
        float r0, r1;
        residual_pair(__builtin_bit_cast(uint32_t, hp), v0, v1, r0, r1);
        l0 = (_Float16)r0; l1 = (_Float16)r1;
    }
    if (e < 8) { hi0[e - 1] = h0; hi0[e] = h1; lo0[e - 1] = l0; lo0[e] = l1; }
    else { hi1[e - 9] = h0; hi1[e - 8] = h1; lo1[e - 9] = l0; lo1[e - 8] = l1; }
}

// ---- staged epilogue ----------------------------------------------------------------------------------------------
// With one wave per SIMD an instruction costs 4 issue cycles, a VALU op that consumes the result of the instruction right
// in front of it 8, and about six independent ones hide behind one 32-cycle MFMA (tools/ubench/mfma_issue.hip).  The
// epilogue of a pending tile is therefore cut into STAGES of mutually independent ops over a group of elements, one stage
// per MFMA gap: read accumulators | fma | max | pack hi | residual | pack lo | park hi | park lo.  Groups follow each other
// from gap 1 on; a plan exists when all of it fits in front of the k-steps that consume the outputs.
struct Epi {
    float v[16];        // activation in fp32
    float r[16];        // residual v - hi
    uint32_t hp[8];     // packed fp16 pairs: hi
    uint32_t lp[8];     // lo
    float dw[16];       // DOT tiles: the dot-product weights of the elements (read one stage ahead of their use)
};

// PM: bit q set = k-step q issues a DMA piece.  A piece costs ~16 issue cycles (it is priced like a four-dword store),
// so in the three-pass kernel it has the gap behind the k-step's second MFMA to itself.
template <bool X3, int NKH, int NQ, bool FEEDS, uint32_t PM>
struct EpiPlan {
    static constexpr int GPK = X3 ? 3 : 1;                 // MFMA gaps per k-step
    static constexpr int NS = X3 ? 8 : 5;                  // stages per group
    static constexpr int NGAPS = GPK * NQ;
    static constexpr int D0 = FEEDS ? GPK * (NKH - 2) - 1 : NGAPS - 1;   // last gap for outputs 0..7
    static constexpr int D1 = FEEDS ? GPK * (NKH - 1) - 1 : NGAPS - 1;   // ... 8..15
    static constexpr bool usable(int gi) { return gi >= 1 && gi < NGAPS && !(X3 && gi % GPK == 1 && ((PM >> (gi / GPK)) & 1u)); }
    static constexpr int gap_of(int n) {                    // gap of the n-th stage slot
        int c = -1;
        for (int gi = 0; gi < NGAPS; ++gi)
            if (usable(gi) && ++c == n) return gi;
        return 1 << 20;
    }
    static constexpr bool fits(int ng) { return gap_of((ng >= 2 ? ng / 2 : 1) * NS - 1) <= D0 && gap_of(ng * NS - 1) <= D1; }
    static constexpr int NG = fits(4) ? 4 : (fits(2) ? 2 : (fits(1) ? 1 : 0));   // 8 ops per gap (NG = 2) measures 4 % slower
    static constexpr bool STAGED = NG > 0;
    static constexpr int GS = STAGED ? 16 / NG : 16;
    static constexpr int slot_at(int gi) {                  // stage slot executed in gap gi, or -1
        if (!usable(gi)) return -1;
        int c = 0;
        for (int g = 0; g < gi; ++g) c += usable(g) ? 1 : 0;
        return c < NG * NS ? c : -1;
    }
};

__device__ __forceinline__ h8 pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    u4 t = {a, b, c, d};
    return __builtin_bit_cast(h8, t);
}

// Stage ST of group G of the plan.
// DOT: the tile's activations also feed a one-row linear layer (_alpha_linear on the last trunk layer's output): dot +=
// w[row] * v for every element, in fp32 on the vector ALU.  The weights of a group (dotw: this tile's row of the table in
// LDS, laid out like a bias row) are read in the group's fma stage and used one per later stage, so that the chain of
// dependent FMAs on `dot` never has two links in one MFMA gap.
// !ACT: the activations feed nothing but the dot product (drain_dot): stages from ST_PACK on do their dot FMAs only.
template <class P, bool X3, int G, int ST, bool DOT, bool ACT = true>
__device__ __forceinline__ void epi_stage(const Pend& t, Epi& E, float inv_scale, float lower, h8& y0h, h8& y0l, h8& y1h, h8& y1l,
                                          const float* dotw, float& dot) {
    constexpr int st = ST, e0 = G * P::GS;
    constexpr int ST_PACK = 3, ST_RES = 4, ST_PACKLO = 5, ST_PARK = X3 ? 6 : 4;
    static_assert(ACT || DOT, "a stage without activation output only serves the dot product");
    if constexpr (DOT) {
        static_assert(P::NS - ST_PACK >= 1, "no stage left for the dot product");
        constexpr int NDS = P::NS - ST_PACK;                       // stages that carry dot FMAs: ST_PACK .. NS-1
        if (st == 1) {
#pragma unroll
            for (int q = e0 / 4; q < (e0 + P::GS) / 4; ++q) {      // elements 4q..4q+3 = rows 8q + 4h + 0..3 (like Pend::bias)
                const float4 w4 = *reinterpret_cast<const float4*>(dotw + 8 * q);
                E.dw[4 * q] = w4.x; E.dw[4 * q + 1] = w4.y; E.dw[4 * q + 2] = w4.z; E.dw[4 * q + 3] = w4.w;
            }
        }
        if (st >= ST_PACK) {
#pragma unroll
            for (int e = e0; e < e0 + P::GS; ++e)
                if ((e - e0) % NDS == st - ST_PACK) {
                    dot = __builtin_fmaf(E.dw[e], E.v[e], dot);
                    asm volatile("" : "+v"(dot));   // HERE: the sum is only read at the end of the evaluation, and without a use LLVM
                }                                   // sinks every FMA (and keeps every activation alive) down to it
        }
    }
    if constexpr (!ACT && st >= ST_PACK) return;
    if (st == 0) {
#pragma unroll
        for (int e = e0; e < e0 + P::GS; ++e) {
            float a = t.a[e];
            asm volatile("" : "+v"(a));   // the accumulator-file read happens HERE, not fused in front of its fma
            E.v[e] = a;
        }
    } else if (st == 1) {
        // (v_pk_fma_f32 on element pairs - half the instructions, the same fma per element - measures 1.4 % SLOWER: 368.3 vs
        // 363.2 ms, alternating on one box; hipcc also needs asm for it and then for the ReLU, whose operand it no longer knows
        // to be canonical)
#pragma unroll
        for (int e = e0; e < e0 + P::GS; ++e) E.v[e] = __builtin_fmaf(E.v[e], inv_scale, pend_bias(t, e));
    } else if (st == 2) {
#pragma unroll
        for (int e = e0; e < e0 + P::GS; ++e) E.v[e] = act(E.v[e], lower);
    } else if (st == ST_PACK) {
#pragma unroll
        for (int p = e0 / 2; p < (e0 + P::GS) / 2; ++p) {
            h2 hp;
            hp[0] = (_Float16)E.v[2 * p]; hp[1] = (_Float16)E.v[2 * p + 1];   // one v_cvt_pk_f16_f32
            E.hp[p] = __builtin_bit_cast(uint32_t, hp);
            if (!X3) E.lp[p] = 0u;
        }
    } else if (X3 && st == ST_RES) {
#pragma unroll
        for (int p = e0 / 2; p < (e0 + P::GS) / 2; ++p) residual_pair(E.hp[p], E.v[2 * p], E.v[2 * p + 1], E.r[2 * p], E.r[2 * p + 1]);
    } else if (X3 && st == ST_PACKLO) {
#pragma unroll
        for (int p = e0 / 2; p < (e0 + P::GS) / 2; ++p) {
            h2 lp;
            lp[0] = (_Float16)E.r[2 * p]; lp[1] = (_Float16)E.r[2 * p + 1];
            E.lp[p] = __builtin_bit_cast(uint32_t, lp);
        }
    } else if (st == ST_PARK || st == ST_PARK + 1) {
        // Park finished output k-steps in the accumulator half of the register file, where the MFMAs read them directly
        // (as plain VGPR values the allocator moves half of them there anyway and copies each back in front of its use):
        // hi in this gap, lo in the next.  Output k-step 0 is complete with element 7, k-step 1 with element 15.
        const bool lo = st != ST_PARK;
        if (lo && !X3) return;
        const int last = e0 + P::GS - 1;
        if (last == 7 || (P::GS == 16)) {
            if (!lo) { y0h = pack4(E.hp[0], E.hp[1], E.hp[2], E.hp[3]); asm volatile("" : "+a"(y0h)); }
            else     { y0l = pack4(E.lp[0], E.lp[1], E.lp[2], E.lp[3]); asm volatile("" : "+a"(y0l)); }
        }
        if (last == 15) {
            if (!lo) { y1h = pack4(E.hp[4], E.hp[5], E.hp[6], E.hp[7]); asm volatile("" : "+a"(y1h)); }
            else     { y1l = pack4(E.lp[4], E.lp[5], E.lp[6], E.lp[7]); asm volatile("" : "+a"(y1l)); }
        }
    }
}

// Gap GI (0-based over the tile's main k-steps) of the plan: the stage of one group, or nothing.
template <class P, bool X3, int GI, bool DOT>
__device__ __forceinline__ void epi_gap(const Pend& t, Epi& E, float inv_scale, float lower, h8& y0h, h8& y0l, h8& y1h, h8& y1l,
                                        const float* dotw, float& dot) {
    constexpr int slot = P::slot_at(GI);
    if constexpr (slot >= 0) epi_stage<P, X3, slot / P::NS, slot % P::NS, DOT>(t, E, inv_scale, lower, y0h, y0l, y1h, y1l, dotw, dot);
}

// The epilogue of a pending tile whose activations feed only the dot product (the last trunk tile of a density-only evaluation,
// see mlp_eval): ReLU (lower = 0) and the tile's share of the dot product, with no MFMA around it.  P is the plan of the tile
// that runs this epilogue otherwise; its stages go in the same order, so the FMAs into `dot` are the same ones in the same
// order and the sum keeps its bits.  dotw: this lane half's rows of the tile's dot-table row, as tile_mma passes it.
template <class P, bool X3>
__device__ __forceinline__ void drain_dot(const Pend& t, float inv_scale, const float* dotw, float& dot) {
    if constexpr (P::STAGED) {
        Epi E;
        h8 d0, d1, d2, d3;
        static_for<0, P::NG * P::NS>([&](auto sc) __attribute__((always_inline)) {
            constexpr int s = decltype(sc)::value;
            epi_stage<P, X3, s / P::NS, s % P::NS, true, false>(t, E, inv_scale, 0.f, d0, d1, d2, d3, dotw, dot);
        });
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) dot = __builtin_fmaf(dotw[8 * (e >> 2) + (e & 3)], act(pend_value(t, e, inv_scale), 0.f), dot);
    }
}

}  // namespace nwe
