// The render kernel around mlp_eval - LDS layout, the two work decompositions - and its launcher (see nwe_mfma_kernels.h).
#pragma once
#include "nwe_mfma_eval.h"

namespace nwe {

template <int W, int D, bool SPLIT>
struct Smem {
    using S = Shape<W, D>;
    static constexpr int WBYTES = (SPLIT ? kSplitMaxSamples : kWaves * kPacketMaxSamples) * kRaysPerWave * 4;
    static constexpr int CHUNKS = 2 * S::CHUNK_BYTES;
    static constexpr int BOFF = CHUNKS;                                              // bias tables, coarse then fine
    static constexpr int BIAS_BYTES = ((S::N_CHUNKS * 32 * 4 + 255) / 256) * 256;
    static constexpr int WOFF = BOFF + 2 * BIAS_BYTES;                               // per-wave coarse weights / cdf
    static constexpr int TOFF = WOFF + WBYTES;                                       // t, 1-t, u tables
    static constexpr int XOFF = TOFF + (2 * kMaxSamples + kMaxImportance) * 4;         // sample-split mode: shaded samples, 2 buffers
    static constexpr int LOFF = XOFF + (SPLIT ? 2 * kWaves * kRaysPerWave * 16 : 0);   // three tail slots of two tiles (Walker)
    static constexpr int GOFF = LOFF + 3 * 2 * kTileBytes;                           // gamma(d) fragments, (hi, lo) per k-step and wave
    static constexpr int KOFF = GOFF + kWaves * 2 * S::KD * kTileBytes;                // one word per wave: the hollow path is allowed (colour_skip_built)
    static constexpr int TOTAL = KOFF + kWaves * 4;
    static_assert(XOFF % 16 == 0 && LOFF % 16 == 0 && GOFF % 16 == 0 && KOFF % 16 == 0 && TOTAL % 16 == 0 && TOTAL <= 160 * 1024, "LDS budget");
};

// Two work decompositions, same arithmetic in the same order (results are bit-identical):
//   SPLIT = false: the four waves of a workgroup own four ray packets (128 rays) and walk all their samples;
//   SPLIT = true:  the workgroup owns ONE packet (32 rays); wave w evaluates samples 4i + w, the shaded samples (colour,
//                  opacity) are exchanged through LDS and every wave runs the sequential compositing / importance
//                  sampling for all samples (a few dozen VALU ops per sample, redundantly).  The scheduling unit is a
//                  quarter of the rays and a quarter of the iterations: a 320x240 frame fills the last round of
//                  workgroups 17 % better, a 64x64 frame runs 3x faster; plan_launch() picks per launch.
// What a plain frame does not use: everything but rgb / depth / acc / flags of pinhole views - the coarse-pass and
// diagnostic outputs, raw network outputs, sample depths, coarse weights, the test hooks, the training-mode tables,
// precomputed rays.  A launch without any of them takes the LEAN instantiation, in which they are compile-time null: their
// ~40 pointers otherwise sit in (and spill from) the scalar registers of a kernel that has none to spare - 4.4 GB of
// scratch writes per 800x800 frame before this split (profiles/r02_pmc_summary.txt).
__host__ __device__ inline bool is_lean(const RenderArgs& a) {
    const nwe_outputs& o = a.out;
    return !o.raw_coarse && !o.raw_fine && !o.z_fine && !o.weights_coarse && !o.disp && !o.z_std && !o.rgb_coarse && !o.depth_coarse &&
           !o.acc_coarse && !o.disp_coarse && !o.sample_cond && !o.sample_amp && !o.sample_switch && !o.feat_map && !a.z_fine_in && !a.raw_in_c &&
           !a.raw_in_f && !a.w_in && !a.t_rand && !a.noise_c && !a.noise_f && !a.u_rand && !a.stamps && !a.rays;
}

// The network outputs of one sample: to the raw output (true = a non-finite value, NWE_FLAG_RAW), and - test hook - from the
// caller's table instead of the network; at = ray * samples + sample.
__device__ __forceinline__ bool store_raw(float* raw, float rr, float rg, float rb, float rs) {
    *reinterpret_cast<float4*>(raw) = make_float4(rr, rg, rb, rs);
    return bad(rr) || bad(rg) || bad(rb) || bad(rs);
}
__device__ __forceinline__ void read_raw(const float* raw_in, int64_t at, float& rr, float& rg, float& rb, float& rs) {
    const float4 v = *reinterpret_cast<const float4*>(raw_in + at * 4);
    rr = v.x; rg = v.y; rb = v.z; rs = v.w;
}

// The sample step that the two work decompositions of render_mfma_kernel share.  Macros, not functions: the kernel's register
// allocation does not survive even an inlined call here (a helper for the first fragments alone renumbers scalar registers).
// NWE_PRIME_STREAM: start streaming chunks 0 and 1 (layer 0, tiles 0 and 1), which fly while the sample's depth and gamma(x)
// are computed.  NWE_EVAL_POINT: the network at depth Z on `ray` -> rr, rg, rb, rs: gamma(x), the barrier that publishes chunk 0,
// its first PD fragments, the statements BEHIND_READS, mlp_eval.
#define NWE_PRIME_STREAM()                                                   \
    {                                                                        \
        wk.start(net.stream, bias);                                          \
        wk.begin(S::N_L0, 0, 0);                                             \
        _Pragma("unroll") for (int i = 0; i < S::N_L0; ++i) wk.piece(i);     \
        wk.begin(S::N_L0, 1, 1);                                             \
        _Pragma("unroll") for (int i = 0; i < S::N_L0; ++i) wk.piece(i);     \
    }
#define NWE_EVAL_POINT(Z, BEHIND_READS)                                                                                            \
    {                                                                                                                              \
        float px, py, pz;                                                                                                          \
        point_at(ray, Z, px, py, pz);                                                                                              \
        h8 Ghi[S::KG], Glo[S::KG];                                                                                                 \
        /* handler.py:93: scalar_factor = 10, a true division (embedding.py:48) */                                                 \
        encode<5, S::KG, X3>(__fdiv_rn(px, 10.f), __fdiv_rn(py, 10.f), __fdiv_rn(pz, 10.f), half, Ghi, Glo);                       \
        NWE_STAMP(const unsigned long long t1 = __builtin_amdgcn_s_memtime(); st_enc += t1 - t0;)                                  \
        wk.template sync<false>();                                                                                                 \
        Frags F;                                                                                                                   \
        _Pragma("unroll") for (int k = 0; k < PD; ++k) {                                                                           \
            F.hi[k] = *reinterpret_cast<const h8*>(wk.cur() + lane * 16 + (2 * k) * kTileBytes);                                   \
            if (X3) F.lo[k] = *reinterpret_cast<const h8*>(wk.cur() + lane * 16 + (2 * k + 1) * kTileBytes);                       \
        }                                                                                                                          \
        BEHIND_READS                                                                                                               \
        NWE_STAMP(const unsigned long long t2 = __builtin_amdgcn_s_memtime(); wk.st_t0 = t2; st_sync += t2 - t1;)                  \
        mlp_eval<W, D, SKIP, X3, FORM, CSKIP>(wk, F, lane, net.inv_scale, Ghi, Glo, gd_lds, dot_tab, density_only, rr, rg, rb, rs, \
                                              skip_word);                                                                          \
        NWE_STAMP(st_mlp += __builtin_amdgcn_s_memtime() - t2;)                                                                    \
    }

// TERM: early ray termination (include/nwe.h, nwe_set_early_termination), for the LEAN kernels of the folded and the
// no-view-dirs formulations.  In the pass that produces the outputs (the fine pass, or the only one) a sample whose
// transmittance is below a.min_trans weighs nothing (Composite::accumulate_above) - a per-ray rule, whatever the rays around
// it do - and the workgroup leaves the sample loop once every ray it owns is below: the rest of their samples weigh nothing
// either (T never increases, nwe_device.h), so the exit changes no bit of any output.  The masked state costs no register: it
// is (float)comp.t_run < eps.
// The exit is workgroup-uniform by construction and is taken at the top of a sample iteration only, in front of
// NWE_PRIME_STREAM, where no LDS-DMA piece is in flight (the tile that ends an evaluation streams nothing behind it) and no
// barrier is half passed; it adds no barrier:
//   packets:      at the top of iteration s every wave writes "all my rays are below after sample s - 1" to vote word
//                 [s & 1][wave] and reads the four words [(s - 1) & 1][*], written at the top of iteration s - 1 and published
//                 by that iteration's barriers (the first waits for the writer's LDS counter, Walker::sync<false>), which
//                 every wave has passed.  All four waves read the same four words, so all leave in the same iteration.  Word
//                 [s & 1][w] is next written at the top of iteration s + 2 (s + 1: the other parity), and the writer
//                 gets there only through the barriers of iteration s + 1, which the slowest wave reaches behind its read.
//   sample split: the four waves composite the same 32 rays from the same LDS data, so each wave's own vote is the same
//                 value; no exchange.  The two barriers that close the pass are reached by every wave, with the last drain
//                 between them.
// Lag: ONE iteration in both plans.  With M = the largest stop index of the workgroup's rays (the first sample whose T is below
// eps; samples 0 .. M - 1 count), the packets plan runs min(S, M + 1) iterations of one sample, the sample-split plan
// min(ceil(S / 4), ceil(M / 4) + 1) iterations of four: the votes are taken in front of the compositing that the same
// iteration's first barrier releases.
// The ray evaluations executed go to *a.evals, one atomic per wave: rays of its own x samples its workgroup walked.
constexpr int kVoteBytes = 2 * kWaves * 4;

// SHARE: the coarse pass shared by k x k pixel blocks (include/nwe.h, nwe_set_shared_coarse), for the same LEAN kernels.  One
// instantiation, two launches with a workgroup-uniform role (RenderArgs::share):
//   producer: its rays are the representative pixels of the call's blocks (seed_rep_ray).  Pass 0 only - density-only where
//             that is built - and each sample's weight also goes to the table a.share_w[sample][representative]: the 32 rays
//             of a packet store one 128-byte line per sample.  No per-ray output; the coarse flag bits of its composite go to
//             a.out.flags, which is null unless every ray is its own representative (k = 1 under separate passes).
//   consumer: the call's rays.  Pass 0 is the fill of fs.wc from the table column of the ray's representative (share_rep_of;
//             the path of the a.w_in hook, with an index computed from the pixel and gone again before the sample loop), then
//             build_cdf and the fine pass as in every other kernel.
// The weights the consumer reads are the bits the producer's Composite::accumulate returned, the ones an ordinary frame puts
// into fs.wc for the representative ray itself; near and far are the frame's, so the cdf, and with it z_fine, of a ray is
// its representative's bit for bit.
template <int W, int D, int SKIP, bool X3, bool SPLIT, int FORM, bool LEAN, bool TERM = false, bool SHARE = false>
__global__ void __launch_bounds__(256) render_mfma_kernel(RenderArgs a_in, NetMfma nc, NetMfma nf) {
    static_assert(!TERM || (LEAN && FORM != kFormReference), "early termination: lean kernels of the product formulations only");
    static_assert(!SHARE || (LEAN && !TERM && FORM != kFormReference), "shared coarse pass: lean kernels of the product formulations, not with TERM");
    RenderArgs a = a_in;
    if constexpr (LEAN) {
        a.out.raw_coarse = a.out.raw_fine = a.out.z_fine = a.out.weights_coarse = nullptr;
        a.out.disp = a.out.z_std = a.out.rgb_coarse = a.out.depth_coarse = a.out.acc_coarse = a.out.disp_coarse = nullptr;
        a.out.sample_cond = a.out.sample_amp = a.out.sample_switch = a.out.feat_map = nullptr;
        a.z_fine_in = a.raw_in_c = a.raw_in_f = a.w_in = a.t_rand = a.noise_c = a.noise_f = a.u_rand = nullptr;
        a.stamps = nullptr; a.rays = nullptr;
    }
    using S = Shape<W, D>;
    using SM = Smem<W, D, SPLIT>;
    __shared__ __attribute__((aligned(16))) char smem[SM::TOTAL + (TERM && !SPLIT ? kVoteBytes : 0)];

    // The work item: the workgroup's own index, or - a queued launch (RenderArgs::queue; DESIGN.md section 5, "Dealing") - a
    // ticket, which thread 0 takes as the kernel's first act and publishes through the first word of the chunk buffers: nothing
    // else touches them before the barrier behind the table copies.  A ticket that is not below the launch's items leaves at
    // once, all threads alike.  Nothing waits for another workgroup; the counter is the only state workgroups share.
    static_assert(SM::CHUNKS >= 4 && SM::BOFF >= SM::CHUNKS && SM::WOFF > SM::BOFF && SM::TOFF > SM::BOFF && SM::GOFF > SM::BOFF,
                  "the ticket's word lies in the chunk buffers, below every region the prologue writes in front of its barrier");
    unsigned item = blockIdx.x;
    if constexpr (!TERM && !SHARE) {
        if (a.queue) {
            unsigned* s_item = reinterpret_cast<unsigned*>(smem);
            if (threadIdx.x == 0) *s_item = atomicAdd(a.queue, 1u);
            __syncthreads();
            const unsigned ticket = *s_item;            // tested as the vector value it is read as: with the test behind the
            if (ticket >= a.queue_items) return;        // readfirstlane the full sample-split 8x256 kernel spills 12 bytes
            item = __builtin_amdgcn_readfirstlane(ticket);
        }
    }

    NWE_STAMP(const unsigned stamp_item = item;)
#include "nwe_mfma_render_item.h"
}

// The tail kernel ("Dealing"): the packets launch of a hybrid plan whose surplus workgroups - the
// over-provisioned quarter of a queued grid, placed in time order exactly when the packet tickets have run out, on whichever CU
// has just come free - render the plan's sample-split items instead of leaving at once.  One kernel, two roles (a.share):
//   first launch (kTailOff):   a ticket t below queue_items is packet item t, as in render_mfma_kernel.  Every other workgroup
//                              takes s from the call's third counter (a.tail) and renders split item s if the plan has one.
//   second launch (kTailSecond): the plan's sample-split launch, as queued or not as it was, behind the first on the device:
//                              item t is rendered only if t is not below the final value of the third counter, a plain load;
//                              a workgroup that renders one counts it in the word behind that counter.
// With the launcher's condition (surplus >= split items) the first launch renders them all and the second is empty; it is
// there so that every split item is rendered exactly once whatever the dealing did.  Nothing waits, polls or retries: a
// workgroup takes one number and acts on it.  LEAN, plain (no TERM, no SHARE); a stamped diagnostic build has it not lean.
constexpr int kTailOff = 0, kTailSecond = 3;            // RenderArgs::share of a tail launch (no sharing kernel reads it)
constexpr unsigned kTailSplit = 0x80000000u, kTailNone = ~0u;   // the published ticket: a split item, nothing
template <int W, int D, int SKIP, bool X3, int FORM, bool LEAN>
__global__ void __launch_bounds__(256) render_mfma_tail_kernel(RenderArgs a_in, NetMfma nc, NetMfma nf) {
    RenderArgs a = a_in;
    unsigned* const tail = a.tail;
    const bool second = a.share == kTailSecond;
    a.w_in = nullptr; a.share = kShareOff;
    if constexpr (LEAN) {
        a.out.raw_coarse = a.out.raw_fine = a.out.z_fine = a.out.weights_coarse = nullptr;
        a.out.disp = a.out.z_std = a.out.rgb_coarse = a.out.depth_coarse = a.out.acc_coarse = a.out.disp_coarse = nullptr;
        a.out.sample_cond = a.out.sample_amp = a.out.sample_switch = a.out.feat_map = nullptr;
        a.z_fine_in = a.raw_in_c = a.raw_in_f = a.t_rand = a.noise_c = a.noise_f = a.u_rand = nullptr;
        a.stamps = nullptr; a.rays = nullptr;
    }
    using SP = Smem<W, D, false>;
    using SS = Smem<W, D, true>;
    __shared__ __attribute__((aligned(16))) char smem[SP::TOTAL > SS::TOTAL ? SP::TOTAL : SS::TOTAL];
    static_assert(SS::CHUNKS >= 4 && SS::BOFF >= SS::CHUNKS && SS::WOFF > SS::BOFF && SS::TOFF > SS::BOFF && SS::GOFF > SS::BOFF &&
                  SP::CHUNKS >= 4 && SP::BOFF >= SP::CHUNKS && SP::WOFF > SP::BOFF && SP::TOFF > SP::BOFF && SP::GOFF > SP::BOFF,
                  "the ticket's word lies in the chunk buffers, below every region either prologue writes in front of its barrier");

    // the first ray of the plan's sample-split part, and its items
    const int64_t split_first = second ? a.ray_first : a.ray_first + (int64_t)a.queue_items * (kWaves * kRaysPerWave);
    unsigned* s_item = reinterpret_cast<unsigned*>(smem);
    if (threadIdx.x == 0) {
        unsigned t;
        if (!second) {
            t = atomicAdd(a.queue, 1u);
            if (t >= a.queue_items) {
                const unsigned items1 = (unsigned)((a.n_rays - split_first + kRaysPerWave - 1) / kRaysPerWave);
                const unsigned s = atomicAdd(tail, 1u);
                t = s < items1 ? kTailSplit | s : kTailNone;
            }
        } else {
            t = a.queue ? atomicAdd(a.queue, 1u) : blockIdx.x;
            const unsigned n = a.queue ? a.queue_items : gridDim.x;
            t = t < n && t >= *tail ? kTailSplit | t : kTailNone;
            if (t != kTailNone) atomicAdd(tail + 1, 1u);   // the items this launch rendered (nwe_debug_last_tail_rest): exactly-once, observable
        }
        *s_item = t;
    }
    __syncthreads();
    const unsigned ticket = *s_item;
    if (ticket == kTailNone) return;
    const unsigned t = __builtin_amdgcn_readfirstlane(ticket);
    using S = Shape<W, D>;
    constexpr bool TERM = false, SHARE = false;
    if (t & kTailSplit) {
        constexpr bool SPLIT = true;
        using SM = SS;
        const unsigned item = t & ~kTailSplit;
        // a stolen item's stamp rows are the ones the second launch would have written: behind the first launch's
        NWE_STAMP(const unsigned stamp_item = second ? item : a.queue_items + item;)
        a.ray_first = split_first;
#include "nwe_mfma_render_item.h"
    } else {
        constexpr bool SPLIT = false;
        using SM = SP;
        const unsigned item = t;
        NWE_STAMP(const unsigned stamp_item = item;)
#include "nwe_mfma_render_item.h"
    }
}
// OCC: the occupancy grid (include/nwe.h, nwe_set_occupancy), for the LEAN kernels of the folded and the no-view-dirs
// formulations, in a kernel of its own name: the other kernels keep their symbols and see no new token (NWE_ITEM_OCC).  In BOTH passes a
// sample whose point lies in a cell marked empty has raw = (0, 0, 0, 0) in place of the network's output - a per-ray rule,
// whatever the rays around it do - and a workgroup leaves out the evaluation of an iteration in which every live ray it owns
// is in an empty cell: in the sample-split plan all four samples of the iteration.  In a mixed iteration the network runs and
// the masked lanes' rr, rg, rb, rs are replaced by 0 behind it.  The density-only coarse pass and the hollow colour path are
// the plain lean kernel's.
// The decision is workgroup-uniform by construction and is taken at the top of a sample iteration, in front of
// NWE_PRIME_STREAM.  Unlike early termination the vote concerns THIS iteration, so there is no lag and one barrier more:
//   1. each lane looks up the cell of its ray's point at this iteration's depth (fresh_ray, point_at: the point
//      NWE_EVAL_POINT encodes; one 4-byte load for a lane inside the box) and the wave votes
//      __all(gone || empty) - in the sample-split plan also "my sample 4 it + wave lies behind the pass's last";
//   2. lane 0 writes the vote to word [n & 1][wave] behind the LDS layout, n = the iteration's number (packets: counted over
//      both passes, which no barrier separates; sample split: within the pass, which two barriers close);
//   3. one __syncthreads(), which waits for every wave's LDS write;
//   4. all four waves read the same four words [n & 1][*] and AND them: the same value in every wave.
// Word [n & 1][w] is next written at the top of iteration n + 2 (n + 1: the other parity), and its writer gets there only
// through the vote barrier of iteration n + 1, which the slowest wave reaches behind its read of iteration n.
// The barrier is safe where it stands: the tile that ends the previous evaluation streams nothing behind it, so no LDS-DMA
// piece is in flight and no barrier of the tile walk is half passed (the place where the terminating kernels leave the loop),
// and every wave reaches it in every iteration - the skip is decided behind it, never in front.
// A skipped iteration primes no stream and enters none of the evaluation's barriers, all four waves alike.  The packets plan
// composites shade(0, 0, 0, 0, ..) as ever.  The sample-split plan composites the previous iteration's samples - published by
// the vote barrier, which every wave reaches behind its own write to the exchange buffer - rotates zp and publishes its shaded
// zero sample: the raw_in branch's iteration without a barrier of its own.  Exchange buffer [it & 1] is written at the end of
// iteration it and was last read by drain(it - 2) in iteration it - 1, which every wave has left when one passes the vote
// barrier of iteration it.
// The lane's "empty" flag crosses the evaluation as the wave's ballot in two scalar registers.
// The ray evaluations executed go to *a.evals, one atomic per wave (packets) or workgroup (sample split): its live rays x the
// samples of the iterations its workgroup evaluated, both passes.
template <int W, int D, int SKIP, bool X3, bool SPLIT, int FORM>
__global__ void __launch_bounds__(256) render_mfma_occ_kernel(RenderArgs a_in, NetMfma nc, NetMfma nf) {
    static_assert(FORM != kFormReference, "occupancy grid: lean kernels of the product formulations only");
    constexpr bool LEAN = true, TERM = false, SHARE = false;
    RenderArgs a = a_in;
    const OccGrid* const occ = a_in.occ;
    a.out.raw_coarse = a.out.raw_fine = a.out.z_fine = a.out.weights_coarse = nullptr;
    a.out.disp = a.out.z_std = a.out.rgb_coarse = a.out.depth_coarse = a.out.acc_coarse = a.out.disp_coarse = nullptr;
    a.out.sample_cond = a.out.sample_amp = a.out.sample_switch = a.out.feat_map = nullptr;
    a.z_fine_in = a.raw_in_c = a.raw_in_f = a.w_in = a.t_rand = a.noise_c = a.noise_f = a.u_rand = nullptr;
    a.stamps = nullptr; a.rays = nullptr;
    using S = Shape<W, D>;
    using SM = Smem<W, D, SPLIT>;
    __shared__ __attribute__((aligned(16))) char smem[SM::TOTAL + kVoteBytes];
    const unsigned item = blockIdx.x;   // never queued: the evaluation counter has the queue's slot
    NWE_STAMP(const unsigned stamp_item = item;)
#define NWE_ITEM_OCC
#include "nwe_mfma_render_item.h"
#undef NWE_ITEM_OCC
}
// LIST: a pixel list (include/nwe.h, nwe_render_pixels), for the LEAN kernels of the folded and the no-view-dirs formulations, in a
// kernel of its own name: the other kernels keep their symbols and see no new token (NWE_ITEM_LIST).  The launch is a ray list's -
// n_rays work rows, no packet blocks, no tail path - but ray `row` of it is the ray of pixel list[row] of the pinhole view the
// camera fields describe, which seed_ray makes from three registers: no ray table, so the kernel is lean, with the density-only
// coarse pass and the hollow colour path of the plain lean kernel.  The list comes in the slot of `rays`, which every lean kernel
// nulls: read first, as int32, then nulled like the rest.  ray_cols, the columns of a ray table, is the poses of the camera here:
// the listed value is clamped to 0 .. ray_cols * rows * W - 1, the rays of an nwe_render call with that camera, so that no value
// makes make_ray read outside the pose table.  `row`, the index within the list, stays what every table row, every store and
// live / gone use.  The queue's slot is free: the ticket prologue is render_mfma_kernel's.
template <int W, int D, int SKIP, bool X3, bool SPLIT, int FORM>
__global__ void __launch_bounds__(256) render_mfma_list_kernel(RenderArgs a_in, NetMfma nc, NetMfma nf) {
    static_assert(FORM != kFormReference, "pixel list: lean kernels of the product formulations only");
    constexpr bool LEAN = true, TERM = false, SHARE = false;
    RenderArgs a = a_in;
    const int32_t* const list = reinterpret_cast<const int32_t*>(a_in.rays);
    a.out.raw_coarse = a.out.raw_fine = a.out.z_fine = a.out.weights_coarse = nullptr;
    a.out.disp = a.out.z_std = a.out.rgb_coarse = a.out.depth_coarse = a.out.acc_coarse = a.out.disp_coarse = nullptr;
    a.out.sample_cond = a.out.sample_amp = a.out.sample_switch = a.out.feat_map = nullptr;
    a.z_fine_in = a.raw_in_c = a.raw_in_f = a.w_in = a.t_rand = a.noise_c = a.noise_f = a.u_rand = nullptr;
    a.stamps = nullptr; a.rays = nullptr;
    using S = Shape<W, D>;
    using SM = Smem<W, D, SPLIT>;
    __shared__ __attribute__((aligned(16))) char smem[SM::TOTAL];
    static_assert(SM::CHUNKS >= 4 && SM::BOFF >= SM::CHUNKS && SM::WOFF > SM::BOFF && SM::TOFF > SM::BOFF && SM::GOFF > SM::BOFF,
                  "the ticket's word lies in the chunk buffers, below every region the prologue writes in front of its barrier");
    unsigned item = blockIdx.x;
    if (a.queue) {
        unsigned* s_item = reinterpret_cast<unsigned*>(smem);
        if (threadIdx.x == 0) *s_item = atomicAdd(a.queue, 1u);
        __syncthreads();
        const unsigned ticket = *s_item;            // tested as the vector value it is read as (render_mfma_kernel)
        if (ticket >= a.queue_items) return;
        item = __builtin_amdgcn_readfirstlane(ticket);
    }
    NWE_STAMP(const unsigned stamp_item = item;)
#define NWE_ITEM_LIST
#include "nwe_mfma_render_item.h"
#undef NWE_ITEM_LIST
}
#undef NWE_PRIME_STREAM
#undef NWE_EVAL_POINT

#ifdef NWE_STAMPS   // a stamped launch is not lean (its stamp buffer), and stamps the tail path all the same
constexpr bool kTailLean = false;
#else
constexpr bool kTailLean = true;
#endif

using RenderKernel = void (*)(RenderArgs, NetMfma, NetMfma);
using RenderLauncher = void (*)(RenderArgs, const NetMfma&, const NetMfma&, bool, bool, int64_t, int64_t, hipStream_t);

// One launch of a shape's kernels of one variant for `rays` rays from ray_first on; `split` says which decomposition, and so the
// size of a work item.  Explicitly instantiated per shape and variant (nwe_mfma_shapes.h, nwe_mfma_inst.hip), which instantiates
// the kernels; the plan of a call's launches, and the conditions under which a variant is taken, are nwe_kernel_mfma.hip's (term:
// is_lean(a), a.min_trans > 0, a.evals; share: a.share, a.share_w; occ: a.occ, a.evals; tail: a.tail, a.share).  Nothing for a shape that does not have
// the variant, so that the instantiation exists all the same.
template <int W, int D, int SKIP, int FORM, int VARIANT>
void launch_one(RenderArgs a, const NetMfma& nc, const NetMfma& nf, bool three_pass, bool split, int64_t ray_first, int64_t rays,
                hipStream_t stream) {
    if constexpr (variant_built(VARIANT, FORM)) {
        if (rays <= 0) return;
        a.ray_first = ray_first;
        const unsigned items = mfma_workgroups(rays, split);
        // a queued launch (a.queue: a zeroed counter of this launch's own) deals its work items to a larger grid; the
        // terminating and the sharing kernels take no tickets, so their launches are never queued
        const bool queued = (VARIANT == kVariantPlain || VARIANT == kVariantTail || VARIANT == kVariantList) && a.queue;
        if (queued) a.queue_items = items;
        const unsigned grid = queued ? queue_grid(items) : items;
        RenderKernel kernel;
        if constexpr (VARIANT == kVariantPlain) {
#define NWE_KERNEL(X3_, SPLIT_, LEAN_) render_mfma_kernel<W, D, SKIP, X3_, SPLIT_, FORM, LEAN_>
            const RenderKernel kernels[8] = {   // index: 4 single-pass + 2 packets + 1 not lean
                NWE_KERNEL(true, true, true),  NWE_KERNEL(true, true, false),  NWE_KERNEL(true, false, true),  NWE_KERNEL(true, false, false),
                NWE_KERNEL(false, true, true), NWE_KERNEL(false, true, false), NWE_KERNEL(false, false, true), NWE_KERNEL(false, false, false)};
#undef NWE_KERNEL
            kernel = kernels[(three_pass ? 0 : 4) + (split ? 0 : 2) + (is_lean(a) ? 0 : 1)];
        } else if constexpr (VARIANT == kVariantTail) {
            const RenderKernel kernels[2] = {render_mfma_tail_kernel<W, D, SKIP, true, FORM, kTailLean>,
                                             render_mfma_tail_kernel<W, D, SKIP, false, FORM, kTailLean>};
            kernel = kernels[three_pass ? 0 : 1];
        } else if constexpr (VARIANT == kVariantOcc) {   // lean only: the caller has checked
#define NWE_KERNEL(X3_, SPLIT_) render_mfma_occ_kernel<W, D, SKIP, X3_, SPLIT_, FORM>
            const RenderKernel kernels[4] = {NWE_KERNEL(true, true), NWE_KERNEL(true, false), NWE_KERNEL(false, true), NWE_KERNEL(false, false)};
#undef NWE_KERNEL
            kernel = kernels[(three_pass ? 0 : 2) + (split ? 0 : 1)];
        } else if constexpr (VARIANT == kVariantList) {   // lean only, a.rays = the pixel list: the caller has checked
#define NWE_KERNEL(X3_, SPLIT_) render_mfma_list_kernel<W, D, SKIP, X3_, SPLIT_, FORM>
            const RenderKernel kernels[4] = {NWE_KERNEL(true, true), NWE_KERNEL(true, false), NWE_KERNEL(false, true), NWE_KERNEL(false, false)};
#undef NWE_KERNEL
            kernel = kernels[(three_pass ? 0 : 2) + (split ? 0 : 1)];
        } else {   // lean only: the caller has checked
#define NWE_KERNEL(X3_, SPLIT_) render_mfma_kernel<W, D, SKIP, X3_, SPLIT_, FORM, true, VARIANT == kVariantTerm, VARIANT == kVariantShare>
            const RenderKernel kernels[4] = {NWE_KERNEL(true, true), NWE_KERNEL(true, false), NWE_KERNEL(false, true), NWE_KERNEL(false, false)};
#undef NWE_KERNEL
            kernel = kernels[(three_pass ? 0 : 2) + (split ? 0 : 1)];
        }
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, a, nc, nf);
    }
}

}  // namespace nwe
