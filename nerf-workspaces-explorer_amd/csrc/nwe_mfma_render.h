// The render kernel around mlp_eval - LDS layout, the two work decompositions - and its launcher (see nwe_mfma_kernels.h).
#pragma once
#include "nwe_mfma_eval.h"

namespace nwe {

// Coarse samples the LDS weight / cdf buffer holds: four packets per workgroup keep one buffer per wave (64 samples); the
// sample-split decomposition has ONE packet per workgroup and one shared buffer, which holds the ABI's full 128 samples
// in half the space - so more than 64 coarse samples always take that decomposition (plan_launch, nwe_kernel_mfma.hip).
constexpr int kPacketMaxSamples = 64;
constexpr int kSplitMaxSamples = kMaxSamples;

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
    static constexpr int TOTAL = GOFF + kWaves * 2 * S::KD * kTileBytes;
    static_assert(XOFF % 16 == 0 && LOFF % 16 == 0 && GOFF % 16 == 0 && TOTAL <= 160 * 1024, "LDS budget");
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
        mlp_eval<W, D, SKIP, X3, FORM>(wk, F, lane, net.inv_scale, Ghi, Glo, gd_lds, dot_tab, density_only, rr, rg, rb, rs);       \
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

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5;
    const int ns = a.n_samples, ni = a.n_importance;

    float* s_t = reinterpret_cast<float*>(smem + SM::TOFF);
    float* s_omt = s_t + kMaxSamples;
    float* s_u = s_omt + kMaxSamples;
    for (int i = threadIdx.x; i < ns; i += 256) { s_t[i] = a.t_vals[i]; s_omt[i] = a.omt_vals[i]; }
    for (int i = threadIdx.x; i < ni; i += 256) s_u[i] = a.u_vals[i];
    float* s_bias = reinterpret_cast<float*>(smem + SM::BOFF);
    constexpr int NCH = S::n_chunks(FORM);       // the launcher checks n_chunks of both networks against it
    constexpr int NROWS = S::n_bias_rows(FORM);  // kFormFolded: the alpha layer's weights and bias ride behind the bias rows
    static_assert(NROWS * 32 * 4 <= SM::BIAS_BYTES, "bias table too small for the dot rows");
    for (int i = threadIdx.x; i < NROWS * 32; i += 256) {
        s_bias[i] = nc.bias[i];
        if (ni > 0) s_bias[SM::BIAS_BYTES / 4 + i] = nf.bias[i];
    }

    const int64_t packet = SPLIT ? (int64_t)item : (int64_t)item * kWaves + wave;
    const int64_t ridx64 = a.ray_first + packet * kRaysPerWave + (lane & 31);
    const bool lane_live = ridx64 < a.n_rays && half == 0;    // this lane stores per-sample outputs of its ray
    const bool live = lane_live && (!SPLIT || wave == 0);      // ... and the per-ray results (every wave holds them in SPLIT mode)
    const bool gone = ridx64 >= a.n_rays;                      // TERM: a lane past the call's rays computes along and has no say
    // One 32-bit row index per lane (the ABI keeps n_rays below 2^31): the ray's own index, or the call's last ray for the
    // lanes of a ragged last packet, which compute along and store nothing.  64-bit only where an offset is formed.
    const int row = (int)(ridx64 < a.n_rays ? ridx64 : a.n_rays - 1);
    const int64_t ridx = row, rclamp = row;
    // The ray is kept as its three-register seed and expanded at the top of every sample iteration (bit-identical by
    // construction): nothing of it but |d| stays in registers across an MLP evaluation.  The empty asm hides the seed from
    // loop-invariant code motion, which would otherwise hoist the expansion and spill its results.
    const bool producer = SHARE && share_role(a) == kShareProducer, consumer = SHARE && share_role(a) == kShareConsumer;
    const RaySeed seed = seed_of<SHARE>(a, rclamp);
    auto fresh_ray = [&]() __attribute__((always_inline)) {
        RaySeed sd = seed;
        asm volatile("" : "+v"(sd.pose), "+v"(sd.x), "+v"(sd.y));
        return make_ray<false>(a, sd);
    };

    Walker<S::CHUNK_BYTES, X3> wk;
    wk.buf0 = smem; wk.lds_chunks = (uint32_t)(uintptr_t)(LDS_AS char*)smem;
    wk.tail0 = smem + SM::LOFF; wk.lds_tail = wk.lds_chunks + SM::LOFF; wk.t3 = 0;
    wk.b = 0; wk.wave = wave; wk.lane_off = lane * 16;

    // gamma(d): once per ray (model_utils.py:23-25 re-embeds the same direction for every sample), parked in LDS
    char* gd_lds = smem + SM::GOFF + wave * (2 * S::KD * kTileBytes) + lane * 16;
    if constexpr (FORM != kFormNoViewDirs) {
        const Ray rv = make_ray<true>(a, seed);
        h8 GDhi[S::KD], GDlo[S::KD];
        encode<2, S::KD, X3>(rv.vx, rv.vy, rv.vz, half, GDhi, GDlo);
#pragma unroll
        for (int k = 0; k < S::KD; ++k) {
            *reinterpret_cast<h8*>(gd_lds + (2 * k) * kTileBytes) = GDhi[k];
            *reinterpret_cast<h8*>(gd_lds + (2 * k + 1) * kTileBytes) = GDlo[k];
        }
    }

    FineSampler fs;
    // coarse weights, then the cdf: one buffer per wave (= per packet), or ONE for the workgroup's single packet (SPLIT), which
    // wave 0 alone writes - all four waves compute the same values - and everyone reads behind a workgroup barrier
    fs.wc = reinterpret_cast<float*>(smem + SM::WOFF) + (SPLIT ? 0 : wave * (kPacketMaxSamples * kRaysPerWave)) + (lane & 31);
    const bool wc_writer = !SPLIT || wave == 0;
    fs.stride = kRaysPerWave; fs.u_tab = s_u; fs.ns = ns; fs.ni = ni;
    fs.cd.t_tab = s_t; fs.cd.omt_tab = s_omt; fs.cd.ns = ns;
    fs.cd.jitter = a.t_rand; fs.cd.row = row;                         // training-mode forward: host-drawn random rows
    fs.u_rand = a.u_rand;
    // Up to this barrier nothing may write the chunk buffers (no LDS-DMA piece, no priming): their first word carries a queued
    // launch's ticket until every wave has read it, which this barrier is the first to guarantee.
    __syncthreads();

    Composite comp;
    uint32_t flags = 0;
#ifdef NWE_STAMPS
    unsigned long long st_enc = 0, st_sync = 0, st_mlp = 0, st_comp = 0;
    const unsigned long long st_begin = __builtin_amdgcn_s_memtime();
    const unsigned long long st_real = __builtin_amdgcn_s_memrealtime();   // 100 MHz: the in-kernel clock is d(memtime) / d(memrealtime) x 100 MHz
#endif
    for (int pass = 0; pass < (ni > 0 ? 2 : 1); ++pass) {
        const NetMfma& net = pass == 0 ? nc : nf;
        const float* bias = s_bias + (pass == 0 ? 0 : SM::BIAS_BYTES / 4);
        const float* dot_tab = bias + NCH * 32;
        const int Stot = pass == 0 ? ns : ns + ni;
        // a lean frame with importance sampling reads nothing of the coarse pass but its weights, which depend on sigma alone
        // (mlp_eval: density_only); with ni == 0 the coarse colour is the frame's colour
        const bool density_only = LEAN && density_only_built<D, SKIP>(FORM) && pass == 0 && ni > 0;
        const float* noise = pass == 0 ? a.noise_c : a.noise_f;
        const float* raw_in = pass == 0 ? a.raw_in_c : a.raw_in_f;   // test hook: network outputs from the caller (uniform)
        if (pass == 0 && a.w_in) {                                   // test hook: coarse weights from the caller, no coarse pass
            if (wc_writer) for (int s = 0; s < ns; ++s) fs.wc[s * kRaysPerWave] = a.w_in[rclamp * ns + s];
            continue;
        }
        if constexpr (SHARE) {
            if (pass == 0 && consumer) {                             // the representative's coarse weights instead of a coarse pass
                const float* col = a.share_w + share_rep_of(a, rclamp);
                const int n_rep = share_n_rep(a, share_grid(a));
                if (wc_writer) for (int s = 0; s < ns; ++s) fs.wc[s * kRaysPerWave] = col[(int64_t)s * n_rep];
                continue;
            }
        }
        comp.reset();
        const bool stops = TERM && (pass == 1 || ni == 0);          // the pass that produces the outputs
        const float eps = stops ? a.min_trans : 0.f;                // 0: nothing is ever below
        if constexpr (SPLIT) {
            // depths are produced strictly in order: zq[0..3] = this iteration's four samples, zq[4] = the first of the next
            int produced = 0;
            auto gen = [&](const Ray& ray) -> float {
                const int i = produced++;
                if (i >= Stot) return 0.f;
                if (pass == 0) return fs.cd.z(ray, i);
                return a.z_fine_in ? a.z_fine_in[rclamp * Stot + i] : fs.next(ray);
            };
            float zq[5], zp[4];
            {
                const Ray ray = fresh_ray();
                if (pass == 1) {
                    if (wc_writer) fs.build_cdf();     // in place: one wave, then everyone reads
                    __syncthreads();
                    fs.start(ray);
                    if (wants_survey(a.out)) {
                        const SampleSurvey sv = fs.survey(ray);
                        if (live) flags |= store_survey(a.out, ridx, sv);
                    }
                }
#pragma unroll
                for (int k = 0; k < 5; ++k) zq[k] = gen(ray);
            }
            float4* xch = reinterpret_cast<float4*>(smem + SM::XOFF);
            const int n_it = (Stot + 3) / 4;
            // composite the (up to four) samples of iteration `it`, shaded by the four waves, in sample order
            auto drain = [&](int it) {
                const float4* x = xch + (it & 1) * (kWaves * kRaysPerWave) + (lane & 31);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int si = 4 * it + k;
                    if (si < Stot) {
                        const float w = TERM ? comp.accumulate_above(x[k * kRaysPerWave], zp[k], eps) : comp.accumulate(x[k * kRaysPerWave], zp[k]);
                        if (pass == 0) {
                            if (wc_writer) fs.wc[si * kRaysPerWave] = w;
                            if constexpr (SHARE) { if (producer && live) a.share_w[si * a.n_rays + row] = w; }   // n_rays = n_rep
                            if (live && a.out.weights_coarse) a.out.weights_coarse[ridx * ns + si] = w;
                        }
                    }
                }
            };
            [[maybe_unused]] int it_end = n_it;   // TERM: the iterations that ran
            for (int it = 0; it < n_it; ++it) {
                if constexpr (TERM) {
                    // comp holds the samples of iterations 0 .. it - 2: iteration it - 1 is composited behind this one's barrier
                    if (stops && it > 0 && __all(gone || comp.below(eps))) { it_end = it; break; }
                }
                NWE_STAMP(const unsigned long long t0 = __builtin_amdgcn_s_memtime();)
                if (!raw_in) NWE_PRIME_STREAM();
                const Ray ray = fresh_ray();
                const int s_own = 4 * it + wave;
                const bool own_valid = s_own < Stot;
                float z_own = zq[0], z_nxt = zq[1];
                if (wave == 1) { z_own = zq[1]; z_nxt = zq[2]; }
                if (wave == 2) { z_own = zq[2]; z_nxt = zq[3]; }
                if (wave == 3) { z_own = zq[3]; z_nxt = zq[4]; }
                float nz[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) nz[k] = gen(ray);
                float rr, rg, rb, rs;
                if (raw_in) {
                    __syncthreads();             // publishes the previous iteration's shaded samples
                    if (it > 0) drain(it - 1);
#pragma unroll
                    for (int k = 0; k < 4; ++k) zp[k] = zq[k];
                    read_raw(raw_in, rclamp * Stot + (own_valid ? s_own : Stot - 1), rr, rg, rb, rs);
                } else {
                    // its barrier also publishes the previous iteration's shaded samples; they are composited behind the fragment
                    // reads, whose latency that covers
                    NWE_EVAL_POINT(z_own, if (it > 0) drain(it - 1); _Pragma("unroll") for (int k = 0; k < 4; ++k) zp[k] = zq[k];);
                }
                NWE_STAMP(const unsigned long long t3 = __builtin_amdgcn_s_memtime();)
                if (own_valid) {
                    xch[(it & 1) * (kWaves * kRaysPerWave) + wave * kRaysPerWave + (lane & 31)] =
                        Composite::shade(rr, rg, rb, rs, z_own, z_nxt, s_own + 1 == Stot, ray.dnorm, noise ? noise[rclamp * Stot + s_own] : 0.f);
                    if (lane_live) {
                        float* raw = pass == 0 ? a.out.raw_coarse : a.out.raw_fine;
                        if (raw && store_raw(raw + (ridx * Stot + s_own) * 4, rr, rg, rb, rs)) flags |= NWE_FLAG_RAW;
                        if (pass == 1 && a.out.z_fine) a.out.z_fine[ridx * Stot + s_own] = z_own;
                    }
                }
                zq[0] = zq[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) zq[k + 1] = nz[k];
                NWE_STAMP(st_comp += __builtin_amdgcn_s_memtime() - t3;)
            }
            __syncthreads();
            drain(TERM ? it_end - 1 : n_it - 1);   // TERM: the last iteration that ran (it_end >= 1)
            __syncthreads();   // the exchange buffers are free again for the next pass
            if constexpr (TERM) {
                if (stops) {
                    const unsigned long long mine = __popcll(__ballot(lane_live));
                    const int walked = (ni > 0 ? ns : 0) + (4 * it_end < Stot ? 4 * it_end : Stot);
                    if (wave == 0 && lane == 0) atomicAdd(a.evals, mine * (unsigned long long)walked);
                }
            }
        } else {
            float z_cur, z_next = 0.f;
            {
                const Ray ray = fresh_ray();
                if (pass == 0) z_cur = fs.cd.z(ray, 0);
                else {
                    fs.prepare(ray);
                    if (wants_survey(a.out)) {
                        const SampleSurvey sv = fs.survey(ray);
                        if (live) flags |= store_survey(a.out, ridx, sv);
                    }
                    z_cur = a.z_fine_in ? a.z_fine_in[rclamp * Stot] : fs.next(ray);
                }
            }
            [[maybe_unused]] int s_end = Stot;   // TERM: the iterations that ran
            for (int s = 0; s < Stot; ++s) {
                if constexpr (TERM) {
                    if (stops) {
                        int* vote = reinterpret_cast<int*>(smem + SM::TOTAL);
                        const int mine = __all(gone || comp.below(eps));
                        if (lane == 0) vote[(s & 1) * kWaves + wave] = mine;
                        if (s > 0) {
                            const int* v = vote + ((s - 1) & 1) * kWaves;
                            if (__builtin_amdgcn_readfirstlane(v[0] & v[1] & v[2] & v[3])) { s_end = s; break; }
                        }
                    }
                }
                NWE_STAMP(const unsigned long long t0 = __builtin_amdgcn_s_memtime();)
                if (!raw_in) NWE_PRIME_STREAM();
                const Ray ray = fresh_ray();
                if (s + 1 < Stot) {
                    if (pass == 0) z_next = fs.cd.z(ray, s + 1);
                    else z_next = a.z_fine_in ? a.z_fine_in[rclamp * Stot + s + 1] : fs.next(ray);
                }
                float rr, rg, rb, rs;
                if (raw_in) {
                    read_raw(raw_in, rclamp * Stot + s, rr, rg, rb, rs);
                } else {
                    NWE_EVAL_POINT(z_cur, );
                }
                NWE_STAMP(const unsigned long long t3 = __builtin_amdgcn_s_memtime();)
                const float4 shaded = Composite::shade(rr, rg, rb, rs, z_cur, z_next, s + 1 == Stot, ray.dnorm, noise ? noise[rclamp * Stot + s] : 0.f);
                const float w = TERM ? comp.accumulate_above(shaded, z_cur, eps) : comp.accumulate(shaded, z_cur);
                if (pass == 0) fs.wc[s * kRaysPerWave] = w;
                if constexpr (SHARE) { if (producer && lane_live) a.share_w[s * a.n_rays + row] = w; }   // n_rays = n_rep
                if (lane_live) {
                    if (pass == 0 && a.out.weights_coarse) a.out.weights_coarse[ridx * ns + s] = w;
                    float* raw = pass == 0 ? a.out.raw_coarse : a.out.raw_fine;
                    if (raw && store_raw(raw + (ridx * Stot + s) * 4, rr, rg, rb, rs)) flags |= NWE_FLAG_RAW;
                    if (pass == 1 && a.out.z_fine) a.out.z_fine[ridx * Stot + s] = z_cur;
                }
                z_cur = z_next;
                NWE_STAMP(st_comp += __builtin_amdgcn_s_memtime() - t3;)
            }
            if constexpr (TERM) {
                if (stops) {
                    const unsigned long long mine = __popcll(__ballot(lane_live));
                    if (lane == 0 && mine) atomicAdd(a.evals, mine * (unsigned long long)((ni > 0 ? ns : 0) + s_end));
                }
            }
        }
        if (live) {
            // density-only coarse pass: there is no coarse colour whose flag could be raised (include/nwe.h)
            flags |= store_ray(a.out, ridx, comp, pass == 1, a.white_bkgd != 0) & (density_only ? ~(uint32_t)NWE_FLAG_RGB_COARSE : ~0u);
            if (ni == 0) flags |= store_ray(a.out, ridx, comp, true, a.white_bkgd != 0);
        }
        // the table is the producer's only result; its coarse flag bits reach a flag word only where the launcher gave it one
        // (separate passes at k = 1, where every ray runs its own coarse pass: nwe_abi.hip)
        if (producer) break;
    }
    if (flags && a.out.flags) atomicOr(a.out.flags, flags);
#ifdef NWE_STAMPS
    if (a.stamps && lane == 0) {   // diagnostic build only: a buffer no other code reads
        unsigned long long* o = a.stamps + ((size_t)item * kWaves + wave) * kStampWords;   // by work item: however it was dealt
        o[0] = st_enc; o[1] = st_sync; o[2] = st_mlp; o[3] = st_comp; o[4] = __builtin_amdgcn_s_memtime() - st_begin;
        o[5] = wk.st_pre; o[6] = wk.st_wait; o[7] = wk.st_post;
        const unsigned long long st_real_end = __builtin_amdgcn_s_memrealtime();
        o[8] = st_real_end - st_real; o[9] = st_begin;
        // where and when the wave ran: HW_REG_XCC_ID (register 20; the XCD is its low four bits) with HW_REG_HW_ID (register 4:
        // wave, SIMD, CU, shader array and engine) above it, the work item, and the wave's span on the 100 MHz clock
        o[10] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) | (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 32;
        o[11] = item; o[12] = st_real; o[13] = st_real_end;
    }
#endif
}
#undef NWE_PRIME_STREAM
#undef NWE_EVAL_POINT

// One launch of a shape's kernel for `rays` rays from ray_first on.  Explicitly instantiated per shape (nwe_mfma_shapes.h), which
// instantiates the shape's eight kernels; the plan of a call's launches is nwe_kernel_mfma.hip's.
template <int W, int D, int SKIP, int FORM>
void launch_one(RenderArgs a, const NetMfma& nc, const NetMfma& nf, bool three_pass, bool split, int64_t ray_first, int64_t rays,
                hipStream_t stream) {
    if (rays <= 0) return;
    a.ray_first = ray_first;
    const int64_t per_wg = split ? kRaysPerWave : kWaves * kRaysPerWave;
    const unsigned blocks = (unsigned)((rays + per_wg - 1) / per_wg);
    // a queued launch (a.queue: a zeroed counter of this launch's own) deals its `blocks` work items to a larger grid
    if (a.queue) a.queue_items = blocks;
    const unsigned grid = a.queue ? queue_grid(blocks) : blocks;
#define NWE_KERNEL(X3_, SPLIT_, LEAN_) render_mfma_kernel<W, D, SKIP, X3_, SPLIT_, FORM, LEAN_>
    void (*const kernels[8])(RenderArgs, NetMfma, NetMfma) = {   // index: 4 single-pass + 2 packets + 1 not lean
        NWE_KERNEL(true, true, true),  NWE_KERNEL(true, true, false),  NWE_KERNEL(true, false, true),  NWE_KERNEL(true, false, false),
        NWE_KERNEL(false, true, true), NWE_KERNEL(false, true, false), NWE_KERNEL(false, false, true), NWE_KERNEL(false, false, false)};
#undef NWE_KERNEL
    hipLaunchKernelGGL(kernels[(three_pass ? 0 : 4) + (split ? 0 : 2) + (is_lean(a) ? 0 : 1)], dim3(grid), dim3(256), 0, stream, a, nc, nf);
}

// Whether a shape has the terminating kernels (TERM): the product formulations do, kFormReference is a comparison path.
constexpr bool term_built(int form) { return form != kFormReference; }

// The same launch with early termination: the shape's four terminating kernels (three-pass / single-pass, packets / sample
// split; lean only - the caller has checked is_lean(a), a.min_trans > 0 and a.evals).  Instantiated per shape in files of their
// own (nwe_mfma_inst_term_*.hip); nothing for a shape that is not term_built.
template <int W, int D, int SKIP, int FORM>
void launch_one_term(RenderArgs a, const NetMfma& nc, const NetMfma& nf, bool three_pass, bool split, int64_t ray_first, int64_t rays,
                     hipStream_t stream) {
    if constexpr (term_built(FORM)) {
        if (rays <= 0) return;
        a.ray_first = ray_first;
        const int64_t per_wg = split ? kRaysPerWave : kWaves * kRaysPerWave;
        const unsigned blocks = (unsigned)((rays + per_wg - 1) / per_wg);
#define NWE_KERNEL(X3_, SPLIT_) render_mfma_kernel<W, D, SKIP, X3_, SPLIT_, FORM, true, true>
        void (*const kernels[4])(RenderArgs, NetMfma, NetMfma) = {NWE_KERNEL(true, true), NWE_KERNEL(true, false), NWE_KERNEL(false, true),
                                                                  NWE_KERNEL(false, false)};
#undef NWE_KERNEL
        hipLaunchKernelGGL(kernels[(three_pass ? 0 : 2) + (split ? 0 : 1)], dim3(blocks), dim3(256), 0, stream, a, nc, nf);
    }
}

// Whether a shape has the sharing kernels (SHARE): as the terminating ones.
constexpr bool share_built(int form) { return form != kFormReference; }

// The same launch for the shared coarse pass (a.share: producer or consumer): the shape's four sharing kernels, lean only.
// Instantiated per shape in files of their own (nwe_mfma_inst_share_*.hip); nothing for a shape that is not share_built.
template <int W, int D, int SKIP, int FORM>
void launch_one_share(RenderArgs a, const NetMfma& nc, const NetMfma& nf, bool three_pass, bool split, int64_t ray_first, int64_t rays,
                      hipStream_t stream) {
    if constexpr (share_built(FORM)) {
        if (rays <= 0) return;
        a.ray_first = ray_first;
        const int64_t per_wg = split ? kRaysPerWave : kWaves * kRaysPerWave;
        const unsigned blocks = (unsigned)((rays + per_wg - 1) / per_wg);
#define NWE_KERNEL(X3_, SPLIT_) render_mfma_kernel<W, D, SKIP, X3_, SPLIT_, FORM, true, false, true>
        void (*const kernels[4])(RenderArgs, NetMfma, NetMfma) = {NWE_KERNEL(true, true), NWE_KERNEL(true, false), NWE_KERNEL(false, true),
                                                                  NWE_KERNEL(false, false)};
#undef NWE_KERNEL
        hipLaunchKernelGGL(kernels[(three_pass ? 0 : 2) + (split ? 0 : 1)], dim3(blocks), dim3(256), 0, stream, a, nc, nf);
    }
}

}  // namespace nwe
