// The weight stream: LDS-DMA walker over two chunk buffers and three tail slots, and the static plan of which k-step issues
// which piece (see nwe_mfma_kernels.h for the design).
#pragma once
#include "nwe_mfma_config.h"

namespace nwe {

// The weight stream of one network, walked chunk by chunk through two LDS buffers.
//
// LDS-DMA goes through inline asm: hipcc's waitcnt pass treats a builtin global_load_lds as an LDS store that may
// alias every later ds_read of the same array and drains vmcnt(0) in front of the first one, which would serialise
// the prefetch with the compute it is meant to hide behind.  The asm form is invisible to that pass; completion is
// waited for by hand in sync() (s_waitcnt vmcnt(0) + barrier).  Wave w streams the w-th quarter of a chunk (n
// consecutive 1-KiB pieces): source = scalar base + lane*16, so a piece costs scalar instructions only.
//
// M0 carries the wave-uniform LDS destination.  With one wave per SIMD every instruction slot counts (a piece with M0
// saved and restored around it is five), so M0 is OWNED by this kernel: it is written once per group of four pieces and
// left there.  That is sound only while hipcc emits no M0 use of its own in this kernel (it has no reason to on gfx950:
// no movrel, no GDS, no sendmsg) - tests/test_abi.py::test_kernel_owns_m0 greps the generated assembly for exactly that,
// and pieces of a group must be issued in order with no other group in between (tile_mma's static schedule does).
// (An "m0" clobber on the asm statements would say nothing to hipcc: M0 is a reserved register, the clobber is ignored with a
// warning.  tools/check_m0.py is the guard: every M0 write in the disassembly must be the first line of one of these statements,
// and no instruction with an implicit M0 operand may appear in the kernel at all.)
//
// Timeline (tile T consumes chunk T from buffer T&1; PD = fragment prefetch distance in k-steps):
//   * ONE barrier per tile, PD k-steps before the tile's end.  Before it every wave waits for its own LDS reads
//     (all reads of chunk T have been issued by then) and its own DMA pieces (chunk T+1, issued >= 7 k-steps
//     earlier).  After it (a) chunk T+1 is visible, so the A fragments of tile T+1's first PD k-steps are read
//     during the last PD k-steps of tile T and the matrix pipe does not drain at the tile boundary, and (b) buffer
//     T&1 is free, so the DMA of chunk T+2 starts at once: its first PD pieces in tile T, the rest early in T+1.
//   * On the long tiles the pre-barrier wait leaves the two fragment reads issued one k-step earlier in flight
//     (lgkmcnt(2): waiting for them too costs an LDS round trip per tile, 5 % of the frame).  Those two reads fetch the
//     (hi, lo) tiles of the chunk's LAST k-step, and these do not live in the chunk buffer the barrier releases but in
//     one of THREE 2-KiB tail slots, slot = chunk mod 3.  Slot (T+2) mod 3 = (T-1) mod 3 is refilled by DMA pieces that
//     are issued behind the barrier of tile T; its previous content, the tail of chunk T-1, was read one k-step before
//     the barrier of tile T-1 and consumed by every wave's last MFMAs of tile T-1 (a wave waits for a fragment before it
//     multiplies with it), i.e. before that wave ARRIVES at the barrier of tile T.  So no LDS location is ever written
//     while a read of its previous content can be outstanding, whatever the timing: the only reads in flight across a
//     barrier target a slot that no DMA piece issued before the NEXT barrier touches.  (LDS returns a wave's reads in
//     order and nothing else in the tile loop counts on lgkmcnt, so "all but two" is exactly "all but those two".)
template <int CHUNK_BYTES, bool X3>
struct Walker {
    const uint8_t* stream;
    uint32_t next_tile;      // first tile of the next chunk to stream
    uint32_t lds_chunks;     // LDS byte address of chunk buffer 0
    uint32_t lds_tail;       // LDS byte address of tail slot 0 (three slots of two tiles)
    const char* buf0;
    const char* tail0;
    int t3;                  // chunk % 3: tail slot of the chunk being consumed
    uint32_t blk_dst_tail;   // blk_dst for the pieces that go to the tail slot (biased so that piece i lands at base + i KiB)
    int tail_first;          // first piece of this wave's quarter that goes to the tail slot (wave 3 of a long chunk), else huge
    const float* bias_tab;   // LDS bias table of the current network, 32 floats per chunk
    int chunk;               // index of the chunk being consumed
    int b;                   // buffer holding the chunk being consumed
    int wave;
    uint32_t lane_off;       // lane * 16
    const uint8_t* blk_src;  // this wave's quarter of the chunk being streamed (uniform)
    uint32_t blk_dst;
    bool skip_lo = false;    // single-pass mode: the odd pieces of the chunk being streamed are lo tiles
    NWE_STAMP(unsigned long long st_pre = 0, st_wait = 0, st_post = 0, st_t0 = 0;)

    __device__ __forceinline__ void start(const uint8_t* s, const float* bias) {
        stream = s; bias_tab = bias; next_tile = 0; chunk = 0; b = 0; t3 = 0;
    }
    __device__ __forceinline__ const char* cur() const { return buf0 + b * CHUNK_BYTES; }
    __device__ __forceinline__ const char* next() const { return buf0 + (b ^ 1) * CHUNK_BYTES; }
    __device__ __forceinline__ const char* tail() const { return tail0 + t3 * (2 * kTileBytes); }
    // Start streaming a chunk of n_per_wave pieces per wave into `buffer`; ahead = how many chunks it is ahead of the one
    // being consumed (its tail slot is (t3 + ahead) mod 3).
    __device__ __forceinline__ void begin(int n_per_wave, int buffer, int ahead) {
        blk_src = stream + ((size_t)next_tile + (size_t)wave * n_per_wave) * kTileBytes;
        blk_dst = lds_chunks + buffer * CHUNK_BYTES + wave * n_per_wave * kTileBytes;
        next_tile += n_per_wave * kWaves;
        skip_lo = !X3 && (n_per_wave & 1) == 0;
        if (X3) {
            int slot = t3 + ahead;
            slot = slot >= 3 ? slot - 3 : slot;
            const bool lng = n_per_wave >= kLongPieces;
            tail_first = (lng && wave == kWaves - 1) ? n_per_wave - 2 : (1 << 20);
            blk_dst_tail = lds_tail + slot * (2 * kTileBytes) - (n_per_wave - 2) * kTileBytes;
        }
    }
    // Piece i of the chunk being streamed.  Pieces go in groups of four: one scalar base per group, the 1-KiB step inside
    // a group rides on the instruction offset, which advances the global source AND the LDS destination (nwe_selftest
    // report[6]).  i is a compile-time constant at every call site.
    // tail_piece: the piece with which this wave's tail pieces would start if the chunk has exactly the caller's static
    // piece count (NB - 2); it rewrites M0 (a no-op for the waves and chunks whose destination does not change there).
    __device__ __forceinline__ void piece(int i, int tail_piece = -1) {
        if constexpr (kExpNoDma) return;
        // single-pass mode multiplies by the hi tiles only: where a wave's quarter of the chunk starts on an even tile (all
        // chunks but the view layer's, 9 tiles per wave) the lo tile of every (hi, lo) pair = the odd pieces is neither
        // streamed nor read; the LDS layout keeps its holes.  (A run-time test, but only in the single-pass instantiation.)
        if (!X3 && skip_lo && (i & 1)) return;
        const uint8_t* src = blk_src + (size_t)(i >> 2) * (4 * kTileBytes);
        // the last two pieces of a long chunk (wave 3: n-2, n-1) go to the chunk's tail slot: a scalar select, no branch
        // (a long chunk has >= kLongPieces pieces per wave, so only pieces kLongPieces - 2.. can be tail pieces: no select in front
        // of the others)
        const uint32_t base = (X3 && i >= kLongPieces - 2 && i >= tail_first) ? blk_dst_tail : blk_dst;
        const uint32_t dst = base + (i >> 2) * (4 * kTileBytes);
        // M0 is written by the first piece of a group and by the piece the tail would start with (6 of an 8-piece quarter, 7
        // of a 9-piece one; the first tail piece of a 10-piece quarter, 8, opens a group anyway, and so does 8 of 9).
        const bool set_m0 = (i & 3) == 0 || (X3 && i == tail_piece);
#define NWE_GLDS(OFF) asm volatile("global_load_lds_dwordx4 %0, %1 offset:" #OFF NWE_GLDS_POL :: "v"(lane_off), "s"(src) : "memory")
#define NWE_GLDS_M0(OFF) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:" #OFF NWE_GLDS_POL \
                                      :: "v"(lane_off), "s"(src), "s"(dst) : "memory")
#define NWE_GLDS_GROUP(OP) switch (i & 3) { case 0: OP(0); break; case 1: OP(1024); break; case 2: OP(2048); break; default: OP(3072); break; }
        if (set_m0) NWE_GLDS_GROUP(NWE_GLDS_M0)   // point M0 at the group's LDS destination (one wait state before the DMA)
        else NWE_GLDS_GROUP(NWE_GLDS)
#undef NWE_GLDS
#undef NWE_GLDS_M0
#undef NWE_GLDS_GROUP
    }
    template <bool LONG_TILE>
    __device__ __forceinline__ void sync() {
        if constexpr (kExpNoSync) return;
        // Own DMA pieces of chunk T+1 landed and own LDS reads done - on the long tiles EXCEPT the two reads just issued (the
        // fragments of this chunk's last k-step, one k-step ago): waiting for those too costs an LDS round trip per tile
        // (5 % of the frame time).  They read the chunk's tail slot, which this barrier does NOT release (see the
        // timeline above); everything in the chunk buffer it does release has been read.  Short tiles have no tail slot
        // and keep the full wait.
        if (LONG_TILE) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");
    }
    __device__ __forceinline__ void tile_done() { b ^= 1; ++chunk; t3 = t3 == 2 ? 0 : t3 + 1; }
};

// Which k-steps of a tile issue DMA pieces (static; tile_mma and the epilogue plan both read it).  The pieces [PD, NB) of
// chunk T+1 go from k-step 0 on, one per k-step on the long tiles - as early as possible, the barrier at k-step QSYNC =
// NQ - PD waits for them - followed by the two extra pieces of a skip-layer chunk (their slots are reserved whether or not
// the chunk has them); after the barrier come the first min(PD, NA) pieces of chunk T+2.
template <int NB, int NA, int NQ>
struct DmaPlan {
    static constexpr int QSYNC = NQ - PD;
    static constexpr int REST = NB > PD ? NB - PD : 0;
    static constexpr int TOT = REST > 0 ? REST + 2 : 0;                                   // logical slots: pieces, then the two extras
    static constexpr int PPK = TOT == 0 ? 0 : (TOT + (QSYNC > 0 ? QSYNC : 1) - 1) / (QSYNC > 0 ? QSYNC : 1);   // slots per k-step (1 on long tiles)
    static_assert(TOT == 0 || QSYNC > 0, "no k-step in front of the barrier for the DMA pieces");
    // A piece holds the wave's issue for ~30 cycles whatever else the gap carries, and two pieces three MFMAs apart cost more
    // than twice one piece six MFMAs apart (tools/ubench/dma_cost.hip: 20 vs 8.6 cycles each beside 32x32x16 MFMAs), so where
    // the tile is long enough the pieces go out every SECOND k-step: the last one still MARGIN k-steps (~500 cycles, more than
    // an L2-hit LDS-DMA takes to land) in front of the barrier that waits for it; the two extra slots follow back to back.
    static constexpr int MARGIN = 5;
    static constexpr int STRIDE = (kDmaStride == 2 && PPK == 1 && 2 * (REST - 1) <= QSYNC - MARGIN && 2 * (REST - 1) + 2 <= QSYNC - 1) ? 2 : 1;
    static constexpr int kstep_of(int j) { return STRIDE == 1 ? j / (PPK > 0 ? PPK : 1) : (j < REST ? 2 * j : 2 * (REST - 1) + 1 + (j - REST)); }
    static constexpr int lo(int q) {                                                      // slots issued before k-step q
        int n = 0;
        for (int j = 0; j < TOT; ++j) n += kstep_of(j) < q ? 1 : 0;
        return n;
    }
    static_assert(TOT == 0 || lo(QSYNC) == TOT, "every slot must be issued in front of the barrier");
    static constexpr uint32_t mask() {
        uint32_t m = 0;
        for (int q = 0; q < NQ; ++q) {
            const bool pre = q < QSYNC && lo(q + 1) > lo(q);
            const bool post = q >= QSYNC && NA > 0 && q - QSYNC < (NA < PD ? NA : PD);
            if (pre || post) m |= 1u << q;
        }
        return m;
    }
};

}  // namespace nwe
