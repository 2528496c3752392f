// One MLP evaluation for a wave's 32 points: network shape, the tile loop, layers, encodings (see nwe_mfma_kernels.h).
#pragma once
#include <cfloat>

#include "nwe_mfma_epilogue.h"
#include "nwe_mfma_stream.h"

namespace nwe {

template <int W, int D>
struct Shape {
    static constexpr int NT = W / 32;    // 32-row tiles of a W-wide layer
    static constexpr int KH = W / 16;    // k-steps over a W-wide activation vector
    static constexpr int KG = 4;         // k-steps over gamma(x) (63 -> 64 slots)
    static constexpr int KD = 2;         // k-steps over gamma(d) (27 -> 32 slots)
    static constexpr int NTV = W / 64;   // row tiles of the view layer (W/2 outputs)
    static constexpr int KV = W / 32;    // k-steps over the view layer output
    // LDS-DMA pieces (1 KiB tiles) per wave and chunk: (hi, lo) per k-step, split evenly over the 4 waves
    static constexpr int N_L0 = 2 * KG / kWaves;
    static constexpr int N_H = 2 * KH / kWaves;
    static constexpr int N_S = 2 * (KH + KG) / kWaves;   // skip layer
    static constexpr int N_V = 2 * (KH + KD) / kWaves;
    static constexpr int N_RGB = 2 * KV / kWaves;
    static constexpr int CHUNK_BYTES = N_S * kWaves * kTileBytes;
    static constexpr int N_CHUNKS = NT + D * NT + 1 + NTV + 1;   // layer 0, D-1 trunk layers + feature, alpha, views, rgb (unfolded: the larger count)
    // FOLD (the product path): _feature_linear is folded into the view layer at pack time (-NT chunks) and _alpha_linear is not
    // a tile of the stream at all (-1): its single output row is a dot product with the last trunk layer's activations,
    // accumulated in fp32 on the vector ALU inside that layer's epilogue (see mlp_eval).  Its weights travel as NT extra
    // rows of the bias table (row rt, element i = weight of trunk feature 32 rt + i) plus one row whose element 0 is its bias.
    static constexpr int N_CHUNKS_FOLDED = N_CHUNKS - NT - 1;
    static constexpr int N_DOT_ROWS = NT + 1;
    // kFormNoViewDirs: layer 0, D-1 trunk layers, one chunk of _output_linear (nerf_model.py:42-43,78-79)
    static constexpr int N_CHUNKS_NOVIEW = D * NT + 1;
    static constexpr int n_chunks(int form) { return form == kFormFolded ? N_CHUNKS_FOLDED : (form == kFormNoViewDirs ? N_CHUNKS_NOVIEW : N_CHUNKS); }
    static constexpr int n_bias_rows(int form) { return n_chunks(form) + (form == kFormFolded ? N_DOT_ROWS : 0); }
};

__device__ __forceinline__ f16v zero_acc() {
    f16v zero;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero[r] = 0.f;
    return zero;
}

template <bool X3>
__device__ __forceinline__ void mma3(const h8& a_hi, const h8& a_lo, const h8& x_hi, const h8& x_lo, f16v& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, x_hi, acc, 0, 0, 0);
    if (X3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, x_hi, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, x_lo, acc, 0, 0, 0);
    }
}

struct Frags { h8 hi[PD + 1], lo[PD + 1]; };   // ring, slot = (k-step counter) mod (PD+1)

// One 32-row tile = NKP optional "pre" k-steps (gamma(x) of the skip layer, taken if use_g) + NKH main k-steps over
// X + NKD "post" k-steps (gamma(d) of the view layer).  Chunk layout in that order, (hi, lo) tile pair per k-step,
// lane-linear.  On entry the fragment ring holds this tile's first PD k-steps in slots PHASE..PHASE+PD-1; on exit
// it holds the next tile's.  The epilogue of the PREVIOUS tile (`prev` -> y*) runs in the MFMA gaps of the main
// k-steps by EpiPlan; FEEDS says that its outputs y* are the last two k-steps of X itself (first tile of a layer, rgb
// head), which sets the plan's deadline.  DMA (DmaPlan): this tile issues the pieces [PD, NB) (+2 if extraB) of chunk
// T+1 in its first k-steps and, after its barrier, pieces [0, min(PD, NA)) of chunk T+2 (NA pieces per wave, +2 if
// extraA; NA = 0: none).  HASNEXT: a tile follows in this pass (its first fragments are prefetched).
// DOT: the pending tile's epilogue also accumulates the dot product of its activations with the row `dot.row` of the dot table
// (32 floats in LDS, see epi_stage) into *dot.sum.
// The compile-time arguments are one TileCfg: KSteps<NKP, NKH, NKD, PHASE>, X3, Chunks<NB, NA, HASNEXT> and the epilogue flags
// kPend (a pending tile's epilogue runs here) | kFeeds | kDot.  The B fragments of the three segments are X, G and D; the
// pending tile's outputs y* are k-steps yk, yk + 1 of (Yhi, Ylo).
template <int NKP_, int NKH_, int NKD_ = 0, int PHASE_ = 0>
struct KSteps { static constexpr int NKP = NKP_, NKH = NKH_, NKD = NKD_, PHASE = PHASE_; };
template <int NB_, int NA_, bool HASNEXT_ = true>
struct Chunks { static constexpr int NB = NB_, NA = NA_; static constexpr bool HASNEXT = HASNEXT_; };
enum : unsigned { kNoEpi = 0, kPend = 1, kFeeds = 2, kDot = 4 };
template <class K, bool X3_, class CH, unsigned EPI>
struct TileCfg : K, CH {
    static constexpr bool X3 = X3_, PEND = (EPI & kPend) != 0, FEEDS = (EPI & kFeeds) != 0, DOT = (EPI & kDot) != 0;
    static_assert(PEND || EPI == kNoEpi, "outputs are fed and a dot product rides on a pending tile's epilogue");
};
struct TileDot { const float* row = nullptr; float* sum = nullptr; };

template <class C, class WalkerT>
__device__ __forceinline__ void tile_mma(WalkerT& wk, Frags& F, int lane, Pend& cur, const Pend& prev, float inv_scale, float lower,
                                         const h8* Xhi, const h8* Xlo, h8* Yhi, h8* Ylo, int yk, const h8* Dhi = nullptr, const h8* Dlo = nullptr,
                                         const TileDot& dot = {}, const h8* Ghi = nullptr, const h8* Glo = nullptr, bool use_g = false,
                                         bool extraB = false, bool extraA = false, int na_override = -1) {
    constexpr int NKP = C::NKP, NKH = C::NKH, NKD = C::NKD, PHASE = C::PHASE, NB = C::NB, NA = C::NA;
    constexpr bool X3 = C::X3, PEND = C::PEND, HASNEXT = C::HASNEXT, FEEDS = C::FEEDS, DOT = C::DOT;
    h8 &y0h = Yhi[yk], &y0l = Ylo[yk], &y1h = Yhi[yk + 1], &y1l = Ylo[yk + 1];
    float dot_dummy = 0.f;
    float& dot_ref = DOT ? *dot.sum : dot_dummy;
    const float* dotw = DOT ? dot.row + 4 * (lane >> 5) : nullptr;   // this lane half's rows 8q + 4h + i of the 32-float row
    constexpr int R = PD + 1;
    constexpr int NQ = NKH + NKD;            // k-steps after the optional pre segment
    constexpr int QSYNC = NQ - PD;           // the barrier sits in front of this k-step
    static_assert(QSYNC >= 0, "tile too short for the prefetch distance");
    static_assert(NKP % R == 0, "the optional segment must not shift the fragment ring");
    const float4* bp = reinterpret_cast<const float4*>(wk.bias_tab + wk.chunk * 32);
    const int h = lane >> 5;
    constexpr bool SPREAD_BIAS = X3 && kSpreadBias && (NKH + NKD) >= 6;
    if constexpr (!SPREAD_BIAS) {
#pragma unroll
        for (int g = 0; g < 4; ++g) cur.bias[g] = bp[2 * g + h];
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    }
    constexpr bool LONG_TILE = X3 && NQ >= 16;   // the (hi, lo) tiles of the last k-step live in the chunk's tail slot (Walker)
    static_assert(2 * 16 / kWaves == kLongPieces, "a tile of >= 16 k-steps is a chunk of >= kLongPieces pieces per wave");
    const char* cbase = wk.cur() + lane * 16;
    const char* nbase = wk.next() + lane * 16;
    const char* tbase = wk.tail() + lane * 16;
    bool pre_done = false;
    float ekeep = 0.f;   // even element of the epilogue pair in flight (unstaged fallback)
    Epi E;
    if (NKP > 0) {
        if (use_g) {   // pre segment: positions 0..NKP-1 of the chunk; reads stay inside this chunk
#pragma unroll
            for (int s = 0; s < NKP; ++s) {
                const int slot = (PHASE + s + PD) % R;
                F.hi[slot] = *reinterpret_cast<const h8*>(cbase + (2 * (s + PD)) * kTileBytes);
                if (X3) F.lo[slot] = *reinterpret_cast<const h8*>(cbase + (2 * (s + PD) + 1) * kTileBytes);
                const int use = (PHASE + s) % R;
                if (s == 0) {
                    cur.a = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.hi[use], Ghi[0], zero_acc(), 0, 0, 0);
                    if (X3) {
                        cur.a = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.lo[use], Ghi[0], cur.a, 0, 0, 0);
                        cur.a = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.hi[use], Glo[0], cur.a, 0, 0, 0);
                    }
                } else {
                    mma3<X3>(F.hi[use], F.lo[use], Ghi[s], Glo[s], cur.a);
                }
                __builtin_amdgcn_sched_group_barrier(0x100, X3 ? 2 : 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, X3 ? 3 : 1, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            cbase += NKP * 2 * kTileBytes;
            pre_done = true;
        }
    }
    static_for<0, NQ>([&](auto qc) __attribute__((always_inline)) {
        constexpr int q = decltype(qc)::value;
        const h8* Xh = q < NKH ? &Xhi[q] : &Dhi[q - NKH];
        const h8* Xl = q < NKH ? &Xlo[q] : &Dlo[q - NKH];
        if (q == QSYNC) {
            NWE_STAMP({ const unsigned long long t = __builtin_amdgcn_s_memtime(); wk.st_pre += t - wk.st_t0; wk.st_t0 = t; })
            wk.template sync<LONG_TILE>();
            NWE_STAMP({ const unsigned long long t = __builtin_amdgcn_s_memtime(); wk.st_wait += t - wk.st_t0; wk.st_t0 = t; })
            if (NA > 0) wk.begin(na_override >= 0 ? na_override : NA + (extraA ? 2 : 0), wk.b, 2);
        }
        // first MFMA of the k-step (hi.hi); everything else of the k-step is issued behind it, while it executes
        const int use = (PHASE + q) % R;
        if constexpr (X3 && kOneWait) asm volatile("" :: "v"(F.hi[use]), "v"(F.lo[use]));
        if (q == 0 && !(NKP > 0 && pre_done)) {
            cur.a = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.hi[use], *Xh, zero_acc(), 0, 0, 0);
        } else {
            cur.a = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.hi[use], *Xh, cur.a, 0, 0, 0);
        }
        // DMA piece of this k-step (DmaPlan).  In the three-pass kernel it goes behind the SECOND MFMA: a piece costs ~16
        // issue cycles and next to the two fragment reads it would overrun the 32 cycles of the MFMA it hides behind.
        auto dma = [&]() __attribute__((always_inline)) {
            using DP = DmaPlan<NB, NA, NQ>;
            if constexpr (q < QSYNC && DP::TOT > 0) {
#pragma unroll
                for (int j = DP::lo(q); j < DP::lo(q + 1); ++j) {
                    if (j < DP::REST) wk.piece(PD + j, NB >= kLongPieces ? NB - 2 : -1);
                    else if (extraB) wk.piece(NB + j - DP::REST);
                }
            }
            if constexpr (q >= QSYNC && NA > 0 && q - QSYNC < (NA < PD ? NA : PD)) wk.piece(q - QSYNC);
        };
        if constexpr (!X3) dma();
        // fragment read of position q+PD: this chunk, or the next tile's first k-steps (visible since the barrier)
        auto read_frag = [&](bool want_hi, bool want_lo) __attribute__((always_inline)) {
            if (LONG_TILE && q + PD == NQ - 1) {
                const int slot = (PHASE + q + PD) % R;   // the two reads that stay in flight across the barrier: the tail slot
                if (want_lo) F.lo[slot] = *reinterpret_cast<const h8*>(tbase + kTileBytes);
                if (want_hi) F.hi[slot] = *reinterpret_cast<const h8*>(tbase);
            } else if (q + PD < NQ) {
                const int slot = (PHASE + q + PD) % R;   // lo first: the first MFMA of the k-step needs hi, so one wait covers both
                if (X3 && want_lo) F.lo[slot] = *reinterpret_cast<const h8*>(cbase + (2 * (q + PD) + 1) * kTileBytes);
                if (want_hi) F.hi[slot] = *reinterpret_cast<const h8*>(cbase + (2 * (q + PD)) * kTileBytes);
            } else if (HASNEXT) {
                const int slot = (PHASE + q + PD) % R;
                if (X3 && want_lo) F.lo[slot] = *reinterpret_cast<const h8*>(nbase + (2 * (q + PD - NQ) + 1) * kTileBytes);
                if (want_hi) F.hi[slot] = *reinterpret_cast<const h8*>(nbase + (2 * (q + PD - NQ)) * kTileBytes);
            }
        };
        constexpr bool SPLIT_RD = X3 && kSplitReads;
        read_frag(true, !SPLIT_RD);
        using Plan = EpiPlan<X3, NKH, NQ, FEEDS, DmaPlan<NB, NA, NQ>::mask()>;
        constexpr int GPK = Plan::GPK;
        if constexpr (kExpNoEpi && PEND && q == 0) asm volatile("" :: "a"(prev.a));   // the pending accumulator is kept alive
        if constexpr (!kExpNoEpi && PEND && Plan::STAGED) epi_gap<Plan, X3, GPK * q, DOT>(prev, E, inv_scale, lower, y0h, y0l, y1h, y1l, dotw, dot_ref);
        if (!kExpNoEpi && PEND && !Plan::STAGED && q < NKH) {
            // short tiles whose outputs feed their own last k-steps have no room for the staged plan: element e runs in
            // k-step floor(e*(NKH-1)/16), so all sixteen are done one k-step before the tile's last
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if ((e * (NKH - 1)) / 16 == q) {
                    finish_elem<X3, DOT>(prev, e, inv_scale, lower, ekeep, y0h, y0l, y1h, y1l, dotw, &dot_ref);
                    if (e == 7) asm volatile("" : "+a"(y0h), "+a"(y0l));
                }
        }
        // Issue order: each MFMA opens its own scheduling region (hard fence behind every gap), the fragment reads and the
        // DMA piece follow the first one.  Inside a region the ops are independent of each other by construction, so the
        // order hipcc picks there costs nothing; without the fences it sinks the prefetch reads (issued PD k-steps early
        // on purpose) to their first use and clusters the epilogue into dependent chains at the end of the tile.
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (q + PD < NQ || HASNEXT) __builtin_amdgcn_sched_group_barrier(0x100, (X3 && !SPLIT_RD) ? 2 : 1, 0);
        if (X3) {
            __builtin_amdgcn_sched_barrier(0);
            cur.a = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.lo[use], *Xh, cur.a, 0, 0, 0);
            dma();
            if constexpr (!kExpNoEpi && PEND && Plan::STAGED) epi_gap<Plan, X3, GPK * q + 1, DOT>(prev, E, inv_scale, lower, y0h, y0l, y1h, y1l, dotw, dot_ref);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_barrier(0);
            cur.a = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.hi[use], *Xl, cur.a, 0, 0, 0);
            if constexpr (SPLIT_RD) read_frag(false, true);
            if constexpr (SPREAD_BIAS && q >= 1 && q <= 4) cur.bias[q - 1] = bp[2 * (q - 1) + h];
            if constexpr (!kExpNoEpi && PEND && Plan::STAGED) epi_gap<Plan, X3, GPK * q + 2, DOT>(prev, E, inv_scale, lower, y0h, y0l, y1h, y1l, dotw, dot_ref);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (SPLIT_RD && (q + PD < NQ || HASNEXT)) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (SPREAD_BIAS && q >= 1 && q <= 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    });
    // Keep the epilogue HERE: its results are only consumed by the next layer, so without a use at this point
    // LLVM sinks the whole epilogue of every tile of a layer to the layer's end (and keeps all their accumulators
    // alive), which is exactly the un-overlapped VALU block this structure is meant to remove.
    // The "a" constraint also parks the finished fragments in the accumulator half of the register file, where the
    // MFMAs read them directly; as plain VGPR values the allocator spills half of them there anyway and copies each
    // back (4 v_accvgpr_read + s_nop) in front of every MFMA that uses it.
    if (PEND) asm volatile("" : "+a"(y1h), "+a"(y1l));
    NWE_STAMP({ const unsigned long long t = __builtin_amdgcn_s_memtime(); wk.st_post += t - wk.st_t0; wk.st_t0 = t; })
    wk.tile_done();
}

// tile_mma of a HOLLOW wave (mlp_eval: a wave whose 32 rays all have sigma <= 0 owes the workgroup nothing of a colour tile but
// its quarter of the weight stream): no MFMA, no fragment read, no epilogue.  What it keeps is everything the other three waves
// count on - the same LDS-DMA pieces of the same chunks in the same order on the same side of the tile's one barrier, begin() of
// chunk T+2 behind it, tile_done() - for a tile without optional k-steps or extra pieces (the view tiles and the rgb head have
// neither).  The wait in front of the barrier is the full one: this wave multiplies with nothing, so it keeps no read in flight.
template <class C, class WalkerT>
__device__ __forceinline__ void tile_pass(WalkerT& wk) {
    constexpr int NQ = C::NKH + C::NKD, NB = C::NB, NA = C::NA;
    static_assert(C::NKP == 0, "a hollow tile has no optional k-steps");
    using DP = DmaPlan<NB, NA, NQ>;
    static_for<0, DP::REST>([&](auto jc) __attribute__((always_inline)) { wk.piece(PD + decltype(jc)::value, NB >= kLongPieces ? NB - 2 : -1); });
    wk.template sync<false>();
    if constexpr (NA > 0) {
        wk.begin(NA, wk.b, 2);
        static_for<0, (NA < PD ? NA : PD)>([&](auto jc) __attribute__((always_inline)) { wk.piece(decltype(jc)::value); });
    }
    wk.tile_done();
}

// A full layer of NT tiles reading X (+ gamma k-steps) and writing Y.  Tile rt accumulates into P[rt&1] while the
// epilogue of the tile before it runs: for rt = 0 that is the LAST tile of the previous layer (in P1, destined for
// k-steps 2*NT-2, 2*NT-1 of X itself), for rt > 0 tile rt-1 of this layer (destined for Y).  On return P1 holds
// this layer's last tile, still pending.  Chunk sizes for the DMA schedule, in pieces per wave: this layer's chunks
// N_THIS (+2 when use_g), the following layer's N_AFTER (+2 when extra_after), and `first_nb` = what tile 0 still
// has to issue of chunk T+1 (0 at the very start of a pass, where chunks 0 and 1 are streamed up front).  NA_LAST: what the
// layer's last tile starts of chunk T+2 - N_AFTER unless only ONE chunk follows the layer (kFormNoViewDirs: 0).  LAST_HASNEXT =
// false: nothing follows the layer in this evaluation (N_AFTER = 0), so its last tile prefetches no fragments either.
template <int NT, int NKP, int NKH, bool X3, bool PEND0, int N_AFTER, bool PASS_START, bool DOT = false, int NA_LAST = N_AFTER,
          bool LAST_HASNEXT = true, class WalkerT>
__device__ __forceinline__ void layer(WalkerT& wk, Frags& F, int lane, bool use_g, bool extra_after, const h8* Ghi, const h8* Glo,
                                      h8* Xhi, h8* Xlo, h8* Yhi, h8* Ylo, Pend& P0, Pend& P1, float inv_scale, float lower_prev,
                                      float lower, int na_last_override = -1, const float* dot_tab = nullptr, float* dot = nullptr) {
    static_assert(NT % 2 == 0 && NT >= 4, "tiles per layer must be even (accumulator ping-pong)");
    static_assert(LAST_HASNEXT || (N_AFTER == 0 && NA_LAST == 0), "a layer that ends the evaluation streams nothing behind it");
    constexpr int N_THIS = 2 * NKH / kWaves;
    using K = KSteps<NKP, NKH>;
    constexpr unsigned EPI = DOT ? kPend | kDot : kPend;
    // DOT: this layer's activations also feed a one-row linear layer; tile rt's share is accumulated with its epilogue, i.e. in
    // tile rt + 1 (row rt of dot_tab); the last tile's share rides on the epilogue the caller runs in the tile after the layer.
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) {
        Pend& cur = (rt & 1) ? P1 : P0;
        Pend& prev = (rt & 1) ? P0 : P1;
        // chunk T+1 / T+2 seen from tile rt: inside the layer both are this layer's; at its end the next layer's
        const bool ebB = rt + 1 < NT ? use_g : extra_after;
        const bool ebA = rt + 2 < NT ? use_g : extra_after;
        const TileDot drow = {DOT ? dot_tab + (rt - 1) * 32 : nullptr, dot};
        if (rt == 0) {
            constexpr int NB0 = PASS_START ? 0 : N_THIS;
            if constexpr (PEND0) {
                constexpr int L = 2 * NT - 2;   // the previous layer has as many tiles as X has k-step pairs
                tile_mma<TileCfg<K, X3, Chunks<NB0, N_THIS>, kPend | kFeeds>>(wk, F, lane, cur, prev, inv_scale, lower_prev, Xhi, Xlo, Xhi, Xlo, L,
                                                                              nullptr, nullptr, {}, Ghi, Glo, use_g, ebB, ebA);
            } else {
                h8 dh[2], dl[2];
                tile_mma<TileCfg<K, X3, Chunks<NB0, N_THIS>, kNoEpi>>(wk, F, lane, cur, prev, inv_scale, lower_prev, Xhi, Xlo, dh, dl, 0,
                                                                      nullptr, nullptr, {}, Ghi, Glo, use_g, ebB, ebA);
            }
        } else if (rt + 2 < NT) {
            tile_mma<TileCfg<K, X3, Chunks<N_THIS, N_THIS>, EPI>>(wk, F, lane, cur, prev, inv_scale, lower, Xhi, Xlo, Yhi, Ylo, 2 * rt - 2,
                                                                  nullptr, nullptr, drow, Ghi, Glo, use_g, ebB, ebA);
        } else if (rt + 1 < NT) {
            tile_mma<TileCfg<K, X3, Chunks<N_THIS, N_AFTER>, EPI>>(wk, F, lane, cur, prev, inv_scale, lower, Xhi, Xlo, Yhi, Ylo, 2 * rt - 2,
                                                                   nullptr, nullptr, drow, Ghi, Glo, use_g, ebB, ebA);
        } else {
            tile_mma<TileCfg<K, X3, Chunks<N_AFTER, NA_LAST, LAST_HASNEXT>, EPI>>(wk, F, lane, cur, prev, inv_scale, lower, Xhi, Xlo, Yhi, Ylo, 2 * rt - 2,
                                                                                  nullptr, nullptr, drow, Ghi, Glo, use_g, ebB, ebA, na_last_override);
        }
    }
}

// gamma(x) and gamma(d) slot maps (must match the packer, nwe_pack.cpp: gamma_col()):
//   lane half h computes bands [NB*h, NB*h + NB) for the three coordinates; slot q = 2*pair + {0: sin, 1: cos},
//   pair = band_local*3 + coord; after the 6*NB sin/cos slots: identity slots (h=0: x, y; h=1: z, pad).
template <int NB, int NK, bool X3>
__device__ __forceinline__ void encode(float vx, float vy, float vz, int h, h8* Ehi, h8* Elo) {
    float vals[NK * 8];
#pragma unroll
    for (int i = 0; i < NK * 8; ++i) vals[i] = 0.f;
    const float first = h ? (float)(1 << NB) : 1.f;   // 2^(NB*h): this lane half's lowest octave
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = c == 0 ? vx : (c == 1 ? vy : vz);
        float sn[NB], cs[NB];
        octave_sincos<NB>(v, first, sn, cs);             // embedding.py:36: fn(x * freq) for freq = first * 2^bl
#pragma unroll
        for (int bl = 0; bl < NB; ++bl) {
            vals[2 * (bl * 3 + c)] = sn[bl];
            vals[2 * (bl * 3 + c) + 1] = cs[bl];
        }
    }
    vals[6 * NB] = h ? vz : vx;
    vals[6 * NB + 1] = h ? 0.f : vy;
#pragma unroll
    for (int s = 0; s < NK; ++s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = vals[s * 8 + j];
            const _Float16 hh = (_Float16)v;
            Ehi[s][j] = hh;
            Elo[s][j] = X3 ? (_Float16)(v - (float)hh) : (_Float16)0.f;
        }
    }
}

// DMA schedule of view tile RT, in pieces per wave: chunk T+1 (NB) and chunk T+2 (NA).  Plan0: the epilogue plan of view tile 0,
// which in FOLD finishes the last trunk tile (drain_dot replays it where no view layer follows).
template <int W, int D, bool X3>
struct ViewDma {
    using S = Shape<W, D>;
    static constexpr int nb(int rt) { return rt + 1 < S::NTV ? S::N_V : S::N_RGB; }
    static constexpr int na(int rt) { return rt + 2 < S::NTV ? S::N_V : (rt + 2 == S::NTV ? S::N_RGB : 0); }
    using Plan0 = EpiPlan<X3, S::KH, S::KH + S::KD, true, DmaPlan<nb(0), na(0), S::KH + S::KD>::mask()>;
};

// View-layer tiles RT..END-1 (END = NTV unless the caller runs tile 0 apart; compile-time recursion: the DMA schedule and the ring phase depend on RT).  Each tile has
// KH + KD k-steps, which shifts the fragment ring by (KH+KD) mod (PD+1) per tile.
// SIGMA_TILE (the unfolded formulation): tile 0 follows the alpha tile, which has no activation output to finish; tile RT
// accumulates in P[(RT+1)&1].  !SIGMA_TILE (FOLD): tile 0 follows the last trunk tile directly (pending in P1) and runs its
// epilogue - ReLU into the last two k-steps of X itself, and the last share of the alpha dot product (row NT-1 of dot_tab) -
// so tile RT accumulates in P[RT&1].
template <int RT, int W, int D, bool X3, bool SIGMA_TILE, int END = W / 64, class WalkerT>
__device__ __forceinline__ void view_tiles(WalkerT& wk, Frags& F, int lane, h8* Ahi, h8* Alo, const h8* GDhi,
                                           const h8* GDlo, h8* Bhi, h8* Blo, Pend& P0, Pend& P1, float inv_scale,
                                           const float* dot_tab = nullptr, float* dot = nullptr) {
    using S = Shape<W, D>;
    constexpr int par = SIGMA_TILE ? (RT + 1) & 1 : RT & 1;
    Pend& cur = par ? P1 : P0;
    Pend& prev = par ? P0 : P1;
    constexpr int PH = (RT * (S::KH + S::KD)) % (PD + 1);
    constexpr int NB = ViewDma<W, D, X3>::nb(RT);   // chunk T+1
    constexpr int NA = ViewDma<W, D, X3>::na(RT);   // chunk T+2
    using K = KSteps<0, S::KH, S::KD, PH>;
    using CH = Chunks<NB, NA>;
    if constexpr (RT == 0 && SIGMA_TILE) {
        h8 dh[2], dl[2];
        tile_mma<TileCfg<K, X3, CH, kNoEpi>>(wk, F, lane, cur, prev, inv_scale, 0.f, Ahi, Alo, dh, dl, 0, GDhi, GDlo);
    } else if constexpr (RT == 0) {
        tile_mma<TileCfg<K, X3, CH, kPend | kFeeds | kDot>>(wk, F, lane, cur, prev, inv_scale, 0.f, Ahi, Alo, Ahi, Alo, 2 * S::NT - 2, GDhi, GDlo,
                                                            TileDot{dot_tab + (S::NT - 1) * 32, dot});
    } else {
        tile_mma<TileCfg<K, X3, CH, kPend>>(wk, F, lane, cur, prev, inv_scale, 0.f, Ahi, Alo, Bhi, Blo, 2 * RT - 2, GDhi, GDlo);
    }
    if constexpr (RT + 1 < END) view_tiles<RT + 1, W, D, X3, SIGMA_TILE, END>(wk, F, lane, Ahi, Alo, GDhi, GDlo, Bhi, Blo, P0, P1, inv_scale);
}

// View tiles RT..NTV-1 of a hollow wave (tile_pass): the chunks and the DMA schedule of view_tiles.
template <int RT, int W, int D, bool X3, class WalkerT>
__device__ __forceinline__ void view_pass(WalkerT& wk) {
    using S = Shape<W, D>;
    using V = ViewDma<W, D, X3>;
    tile_pass<TileCfg<KSteps<0, S::KH, S::KD>, X3, Chunks<V::nb(RT), V::na(RT)>, kNoEpi>>(wk);
    if constexpr (RT + 1 < S::NTV) view_pass<RT + 1, W, D, X3>(wk);
}

// Whether mlp_eval has the density-only path for a shape: every folded shape except those whose gamma(x) skip input enters the
// last trunk layer (6-deep with skips (4,)).  There the second copy of that layer carries the gamma(x) k-steps too, and the
// three-pass LEAN kernels spill (36 / 64 B of scratch per lane at 6x256); those shapes keep computing the coarse colour.
template <int D, int SKIP>
constexpr bool density_only_built(int form) {
    return kCoarseDensityOnly && form == kFormFolded && !(SKIP >= 0 && SKIP / 2 == D / 2 - 1);
}

// Whether the LEAN render kernels of a shape have the hollow path of mlp_eval (colour_skip): the folded shapes that have the
// density-only path.  In their lean frames the evaluations that are not density-only are exactly those of the pass that produces
// the outputs, so the one word per wave that allows the path (render kernel prologue) is that pass's.  The shapes without
// (6-deep with skips (4,)) evaluate a coarse colour nobody reads and keep evaluating every colour.
template <int D, int SKIP>
constexpr bool colour_skip_built(int form) {
    return kColourSkip && density_only_built<D, SKIP>(form);
}

// One MLP evaluation for the wave's 32 points.  nerf/models/nerf_model.py:45-83.
// Trunk layers run as pairs A->B, B->A so that the two activation register sets keep fixed names inside a rolled loop;
// every tile's epilogue is deferred into the next tile (see Pend).
//
// FOLD (the product path): _feature_linear has no activation (nerf_model.py:64) and feeds only the view layer (:66-70), so
// the packer multiplies it into the view layer's weights (nwe_pack.cpp: pack_mfma): trunk layers 1..D-1 = D/2 - 1 pairs and
// one single layer A->B, then _alpha_linear and the folded view layer both read B = h, the rgb head reads the view layer's
// output in A.  !FOLD evaluates the feature layer as the reference formulates it (D/2 pairs, the last pair's second layer
// is the feature layer without ReLU; alpha reads B, the view layer A); kept selectable for comparison.
// kFormNoViewDirs (use_view_dirs=False, nerf_model.py:42-43,78-79): the trunk as in FOLD (D/2 - 1 pairs and the single last
// layer A -> B, without the dot product), then ONE tile of _output_linear on B = h whose rows 0..3 are rgb_raw, sigma_raw
// (copies in rows 4..7 for the upper lane half; the reference ignores the fifth channel too: model_utils.py:62,71).
// density_only (wave-uniform; honoured where density_only_built): sigma is all the caller reads, so the evaluation ends with
// the trunk (see below) and returns o_r = o_g = o_b = 0.
// CSKIP (the LEAN render kernels where colour_skip_built; skip_word = the wave's word in LDS, see the prologue of the render
// kernel): an evaluation that is not density_only takes the hollow path below if the word is set and no ray of the wave has
// density.
// On entry chunks 0 and 1 of the stream are visible / in flight and F holds the first PD k-steps of chunk 0.
template <int W, int D, int SKIP, bool X3, int FORM, bool CSKIP = false, class WalkerT>
__device__ __forceinline__ void mlp_eval(WalkerT& wk, Frags& F, int lane, float inv_scale, h8* Ghi, h8* Glo, const char* gd_lds,
                                         const float* dot_tab, bool density_only, float& o_r, float& o_g, float& o_b, float& o_s,
                                         const int* skip_word = nullptr) {
    using S = Shape<W, D>;
    static_assert(D % 2 == 0, "trunk depth must be even");
    static_assert(SKIP < 0 || SKIP % 2 == 0, "skip layer index must be even");
    static_assert(S::NT % 2 == 0 && S::NTV % 2 == 0, "tile counts must be even");
    constexpr bool FOLD = FORM == kFormFolded, NOVIEW = FORM == kFormNoViewDirs;
    h8 Ahi[S::KH], Alo[S::KH], Bhi[S::KH], Blo[S::KH];
    Pend P0, P1;
    constexpr int NPAIR = D / 2;
    constexpr int SKIP_PAIR = SKIP < 0 ? -1 : SKIP / 2;   // pair whose first layer takes [gamma, h]

    // layer 0: gamma(x) -> A (nothing pending in front of its first tile); the layer after it opens pair 0
    layer<S::NT, 0, S::KG, X3, false, S::N_H, true>(wk, F, lane, false, SKIP_PAIR == 0, nullptr, nullptr, Ghi, Glo, Ahi, Alo, P0, P1,
                                                    inv_scale, 0.f, 0.f);
    // One pair of trunk layers.  use_g / skip_next are literals at every call site, so the run-time tests on them inside
    // tile_mma (the optional gamma(x) k-steps, the two extra DMA pieces of a skip-layer chunk) fold away per site.
    auto pair_body = [&](bool use_g, bool skip_next, bool last) __attribute__((always_inline)) {
        // first of pair: (gamma +) A -> B, ReLU.  Its first tile finishes the pending last tile of A (ReLU: the
        // producer is layer 0 or a non-final second-of-pair layer).
        layer<S::NT, S::KG, S::KH, X3, true, S::N_H, false>(wk, F, lane, use_g, false, Ghi, Glo, Ahi, Alo, Bhi, Blo, P0, P1, inv_scale,
                                                            0.f, 0.f);
        // second of pair: B -> A; !FOLD: the last pair's second layer is _feature_linear (no ReLU, nerf_model.py:64).
        // After it comes the next pair's first layer (skip: 2 more pieces) or the alpha tile and then the view layer.
        layer<S::NT, 0, S::KH, X3, true, S::N_H, false>(wk, F, lane, false, skip_next, nullptr, nullptr, Bhi, Blo,
                                                        Ahi, Alo, P0, P1, inv_scale, 0.f, (FORM == kFormReference && last) ? -INFINITY : 0.f,
                                                        (FORM == kFormReference && last) ? S::N_V : -1);
    };
    constexpr int PAIRS = FORM == kFormReference ? NPAIR : NPAIR - 1;   // pairs evaluated here (otherwise the last trunk layer stands alone below)
    if constexpr (kPeelSkip && SKIP_PAIR >= 0 && SKIP_PAIR < PAIRS) {
#pragma unroll 1
        for (int pair = 0; pair < SKIP_PAIR; ++pair) pair_body(false, pair + 1 == SKIP_PAIR, false);
        pair_body(true, false, SKIP_PAIR == NPAIR - 1);
#pragma unroll 1
        for (int pair = SKIP_PAIR + 1; pair < PAIRS; ++pair) pair_body(false, false, pair == NPAIR - 1);
    } else {
#pragma unroll 1
        for (int pair = 0; pair < PAIRS; ++pair) {
            const bool last = pair == NPAIR - 1;
            pair_body(pair == SKIP_PAIR, !last && pair + 1 == SKIP_PAIR, last);
        }
    }
    float sig = 0.f;   // FOLD: this lane half's share of _alpha_linear . h
    // both lane halves hold half of the features: the other half's share comes over the 32-lane swap; the row behind the
    // weights holds the bias in element 0
    auto sigma_of = [&]() __attribute__((always_inline)) { return __fadd_rn(__fadd_rn(sig, __shfl_xor(sig, 32, 64)), dot_tab[S::NT * 32]); };
    if constexpr (FOLD) {
        // FOLD: the last trunk layer stands alone (A -> B); behind it comes the view layer at once (its chunks are N_V pieces).
        // _alpha_linear (nerf_model.py:63) is one output row on this layer's activations h: sigma = w . h + b is accumulated
        // in fp32 on the vector ALU with the tiles' epilogues (row rt of dot_tab holds w[32 rt .. 32 rt + 31]) instead of a
        // 32-row MFMA tile of which one row would be used (48 of 3168 MFMAs, 16 KB of the weight stream per evaluation).
        constexpr bool G_LAST = SKIP_PAIR == NPAIR - 1;
        if constexpr (density_only_built<D, SKIP>(FORM)) {
            if (density_only) {
                // Density only (the coarse pass of a lean frame with importance sampling: its colour is never read, only its weights,
                // which depend on sigma alone): the last trunk layer a second time, with nothing streamed behind it - its last two
                // tiles start no DMA of chunks T+1 / T+2 and the last one prefetches no fragments - and the view layer and rgb head
                // (240 of 3120 MFMAs and 160 of 2080 KiB of weight tiles at 8x256) are skipped.  The last trunk tile's epilogue
                // (pending in P1), which view tile 0 runs otherwise, is reduced to what sigma needs: ReLU and row NT-1 of the dot
                // product, in view tile 0's order.  Every FMA into `sig` is the one of the full evaluation in the same order, so
                // sigma has the same bits.
                // End of the evaluation: no DMA is in flight (the last piece, of this layer's last chunk, was waited for at the
                // barrier of tile NT-2), and across the last tile's barrier each wave has at most the two reads of that chunk's TAIL
                // SLOT outstanding, consumed by its own last MFMAs (Walker timeline) - every read of a chunk buffer had completed
                // before any wave passed that barrier.  The next evaluation's first pieces (issued at once, before any barrier) write
                // chunk buffers 0 and 1 only; the first piece that writes a tail slot is issued behind that evaluation's first
                // barriers, which no wave reaches before its last MFMA here.  So nothing lands where a read can still be pending.
                using TrunkA = EpiPlan<X3, S::KH, S::KH, false, DmaPlan<S::N_H, S::N_V, S::KH>::mask()>;   // tile NT-2, full / here
                using TrunkA0 = EpiPlan<X3, S::KH, S::KH, false, DmaPlan<S::N_H, 0, S::KH>::mask()>;
                using TrunkB = EpiPlan<X3, S::KH, S::KH, false, DmaPlan<S::N_V, S::N_V, S::KH>::mask()>;   // tile NT-1, full / here
                using TrunkB0 = EpiPlan<X3, S::KH, S::KH, false, DmaPlan<0, 0, S::KH>::mask()>;
                static_assert(TrunkA::NG == TrunkA0::NG && TrunkB::NG == TrunkB0::NG,
                              "the last trunk tiles must run the epilogues they carry in the full evaluation's order (dot FMAs)");
                static_assert(!G_LAST, "density_only_built: the last trunk layer takes no gamma(x) k-steps here");
                layer<S::NT, 0, S::KH, X3, true, 0, false, true, 0, false>(wk, F, lane, false, false, nullptr, nullptr, Ahi, Alo, Bhi, Blo, P0, P1,
                                                                           inv_scale, 0.f, 0.f, -1, dot_tab, &sig);
                drain_dot<typename ViewDma<W, D, X3>::Plan0, X3>(P1, inv_scale, dot_tab + (S::NT - 1) * 32 + 4 * (lane >> 5), sig);
                o_s = sigma_of();
                o_r = o_g = o_b = 0.f;
                return;
            }
        }
        layer<S::NT, G_LAST ? S::KG : 0, S::KH, X3, true, S::N_V, false, true>(wk, F, lane, G_LAST, false, Ghi, Glo, Ahi, Alo, Bhi, Blo, P0, P1,
                                                                               inv_scale, 0.f, 0.f, -1, dot_tab, &sig);
    }
    constexpr int L = 2 * S::NT - 2;
    constexpr int LV = 2 * S::NTV - 2;
    if constexpr (NOVIEW) {
        // the last trunk layer A -> B: ONE chunk follows it (N_H pieces per wave), so its last tile starts no chunk T+2
        constexpr bool G_LAST = SKIP_PAIR == NPAIR - 1;
        layer<S::NT, G_LAST ? S::KG : 0, S::KH, X3, true, S::N_H, false, false, 0>(wk, F, lane, G_LAST, false, Ghi, Glo, Ahi, Alo, Bhi, Blo, P0, P1,
                                                                                   inv_scale, 0.f, 0.f);
        // _output_linear in P0 while the last trunk tile (P1, NT even) is finished - ReLU - into the last two k-steps of B, which
        // this tile itself reads (FEEDS).  Nothing is streamed behind it: the caller starts the next pass.
        tile_mma<TileCfg<KSteps<0, S::KH>, X3, Chunks<0, 0, false>, kPend | kFeeds>>(wk, F, lane, P0, P1, inv_scale, 0.f, Bhi, Blo, Bhi, Blo, L);
        o_r = pend_value(P0, 0, inv_scale);
        o_g = pend_value(P0, 1, inv_scale);
        o_b = pend_value(P0, 2, inv_scale);
        o_s = pend_value(P0, 3, inv_scale);
        return;
    }
    static_assert((S::NTV * (S::KH + S::KD)) % (PD + 1) == 0, "the view tiles must restore the ring phase");
    // gamma(d) is per-ray, used by the view layer only: it waits in LDS (this lane's 16 bytes of each fragment tile) instead
    // of holding 16 registers through the trunk.  Read behind the trunk's last barrier, long before the view tiles' k-steps
    // KH.. need it; older than the fragment reads the tile barriers leave in flight.
    h8 GDhi[S::KD], GDlo[S::KD];
#pragma unroll
    for (int k = 0; k < S::KD; ++k) {
        GDhi[k] = *reinterpret_cast<const h8*>(gd_lds + (2 * k) * kTileBytes);
        if (X3) GDlo[k] = *reinterpret_cast<const h8*>(gd_lds + (2 * k + 1) * kTileBytes);
    }
    if constexpr (FOLD && CSKIP) {
        static_assert(colour_skip_built<D, SKIP>(FORM), "the hollow path: shapes of colour_skip_built only");
        // The hollow path.  A sample with sigma_raw <= 0 has alpha = 1 - exp(-max(sigma_raw, 0) dist) = 0 and weighs 0, so in
        // r + w c its colour c adds +0 whatever finite value it has (Composite::shade, ::accumulate): nothing the view tiles 1..
        // and the rgb head compute for it reaches an output of a lean frame.  sigma is complete once view tile 0 has run the
        // last trunk tile's epilogue - the same FMAs into `sig` in the same order as ever, so sigma has the same bits - and if
        // NONE of the wave's 32 rays has density there (and the launch allows it: the word), the wave leaves out the rest of the
        // evaluation's arithmetic: NTV - 1 view tiles and the rgb head, 186 of 3120 MFMAs at 8x256, with their fragment reads and
        // epilogues.  The colour it returns is 0 where the full path returns a finite value that is multiplied by a zero weight.
        // -inf and NaN never pass the test: there the weight is NaN and so is every output, on either path.
        // The word is set only where the full path's colour cannot be NaN for a finite sigma by way of its inputs: colour layers
        // finite as packed (Packed::colour_finite) and a finite gamma(d) for every ray of the wave.  What is left is an
        // activation above fp16's range under a finite sigma.
        // The branch is wave-uniform, NOT workgroup-uniform: the other waves may run the full path, and they need this wave's
        // quarter of every chunk and its arrival at every barrier.  tile_pass keeps both, tile for tile, so:
        //   * every buffer release still rests on a barrier plus each wave's own waits in front of it.  A hollow wave only
        //     arrives early at barriers it still takes part in; the pieces it issues behind barrier T are the ones tile_mma
        //     issues there, into the buffer and tail slot that barrier released whatever the timing (Walker timeline).
        //   * on entry the wave may still have the prefetched fragments of view tile 1 in flight (chunk T, which nothing writes
        //     before barrier T + 1); its full wait in front of barrier T retires them.  From there on it has no read outstanding
        //     anywhere, so the tail-slot argument - no write where a read of the old content can be pending - holds for it trivially.
        //   * the end of the evaluation is the state the density-only comment describes: no DMA in flight (the rgb head streams
        //     nothing behind it; the last piece was waited for at the last view tile's barrier), no read of a chunk buffer
        //     pending in any wave behind the rgb head's barrier, the next evaluation's first pieces write buffers 0 and 1 only.
        //   * the pieces of a group stay in order with no other group between them (M0, tools/check_m0.py): tile_pass issues
        //     tile_mma's pieces in tile_mma's order, and the two paths join only at the end of the evaluation.
        const int allow = *skip_word;   // with the gamma(d) fragments: long retired when view tile 0 ends
        view_tiles<0, W, D, X3, false, 1>(wk, F, lane, Bhi, Blo, GDhi, GDlo, Ahi, Alo, P0, P1, inv_scale, dot_tab, &sig);
        const float sigma = sigma_of();
        o_s = sigma;
        if (__all(allow != 0 && sigma <= 0.f && sigma >= -FLT_MAX)) {
            view_pass<1, W, D, X3>(wk);
            tile_pass<TileCfg<KSteps<0, S::KV>, X3, Chunks<0, 0, false>, kNoEpi>>(wk);
            o_r = o_g = o_b = 0.f;
            return;
        }
        view_tiles<1, W, D, X3, false>(wk, F, lane, Bhi, Blo, GDhi, GDlo, Ahi, Alo, P0, P1, inv_scale);
        tile_mma<TileCfg<KSteps<0, S::KV>, X3, Chunks<0, 0, false>, kPend | kFeeds>>(wk, F, lane, P0, P1, inv_scale, 0.f, Ahi, Alo, Ahi, Alo, LV);
        o_r = pend_value(P0, 0, inv_scale);
        o_g = pend_value(P0, 1, inv_scale);
        o_b = pend_value(P0, 2, inv_scale);
        return;
    } else if constexpr (FOLD) {
        // folded view layer: [h (B), gamma(d)] -> A[0..KV), ReLU (nerf_model.py:64-70 with W_v[:, :W] . W_f multiplied out).
        // Its first tile runs the epilogue of the last trunk tile (P1, NT even): ReLU into the last two k-steps of B itself and
        // the last share of the alpha dot product.  Tile RT accumulates in P[RT & 1], so the last one (NTV even) is in P1.
        view_tiles<0, W, D, X3, false>(wk, F, lane, Bhi, Blo, GDhi, GDlo, Ahi, Alo, P0, P1, inv_scale, dot_tab, &sig);
        const float sigma = sigma_of();
        // rgb head (nerf_model.py:74) in P0 while the last view tile (P1) is finished into A; rows 0..2 and their copies 4..6
        // for the upper lane half.  Nothing is streamed behind it: the caller starts the next pass.
        tile_mma<TileCfg<KSteps<0, S::KV>, X3, Chunks<0, 0, false>, kPend | kFeeds>>(wk, F, lane, P0, P1, inv_scale, 0.f, Ahi, Alo, Ahi, Alo, LV);
        o_s = sigma;
        o_r = pend_value(P0, 0, inv_scale);
        o_g = pend_value(P0, 1, inv_scale);
        o_b = pend_value(P0, 2, inv_scale);
        return;
    } else {
        // _alpha_linear on B, the input of _feature_linear (nerf_model.py:63); meanwhile the last feature tile (P1) is
        // finished into A without ReLU.  Rows 0 and 4 of the alpha tile both hold the single output row.
        tile_mma<TileCfg<KSteps<0, S::KH>, X3, Chunks<S::N_V, S::N_V>, kPend>>(wk, F, lane, P0, P1, inv_scale, -INFINITY, Bhi, Blo, Ahi, Alo, L);
        const float sigma = pend_value(P0, 0, inv_scale);
        // view layer: [feature (A), gamma(d)] -> B[0..KV), ReLU (nerf_model.py:66-70)
        view_tiles<0, W, D, X3, true>(wk, F, lane, Ahi, Alo, GDhi, GDlo, Bhi, Blo, P0, P1, inv_scale);
        tile_mma<TileCfg<KSteps<0, S::KV>, X3, Chunks<0, 0, false>, kPend | kFeeds>>(wk, F, lane, P1, P0, inv_scale, 0.f, Bhi, Blo, Bhi, Blo, LV);
        o_s = sigma;
    }
    o_r = pend_value(P1, 0, inv_scale);
    o_g = pend_value(P1, 1, inv_scale);
    o_b = pend_value(P1, 2, inv_scale);
}

}  // namespace nwe
