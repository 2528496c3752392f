// Launch planning and dispatch of the MFMA render kernel (templates: nwe_mfma_kernels.h).  This file compiles no kernel: the
// instantiations are translation units of their own (nwe_mfma_inst.hip, once per group of nwe_mfma_shapes.h and kernel variant)
// so that they build in parallel, and are reached through the table below.
#include "nwe_mfma_kernels.h"
#include "nwe_mfma_query.h"

namespace nwe {

#define NWE_DECLARE_SHAPE(W_, D_, SKIP_, FORM_)                                                                                   \
    NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantPlain) NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantTerm)   \
    NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantShare) NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantTail)   \
    NWE_EXTERN_SHAPE_QUERY_LAUNCHER(W_, D_, SKIP_, FORM_)
NWE_SHAPES(NWE_DECLARE_SHAPE)
#undef NWE_DECLARE_SHAPE

// What this library links of a shape in the table.  The product: every variant the shape has, and its query kernels.  A
// diagnostic build (-DNWE_ONLY_HEADLINE: the headline shape alone) links the plain kernels and - `make stamps`,
// -DNWE_DIAG_TAIL - the tail kernel; what is not linked is not named, so its table entry is null.
constexpr bool linked(int variant) {
#if !defined(NWE_ONLY_HEADLINE)
    return true;
#elif defined(NWE_DIAG_TAIL)
    return variant == kVariantPlain || variant == kVariantTail;
#else
    return variant == kVariantPlain;
#endif
}
#ifdef NWE_ONLY_HEADLINE
constexpr bool kQueryLinked = false;
#else
constexpr bool kQueryLinked = true;
#endif

using QueryLauncher = void (*)(QueryArgs, const NetMfma&, bool, unsigned, hipStream_t);

template <int W, int D, int SKIP, int FORM, int VARIANT>
constexpr RenderLauncher render_launcher() {
    if constexpr (linked(VARIANT) && variant_built(VARIANT, FORM)) return launch_one<W, D, SKIP, FORM, VARIANT>;
    else return nullptr;
}
template <int W, int D, int SKIP, int FORM>
constexpr QueryLauncher query_launcher() {
    if constexpr (kQueryLinked) return launch_one_query<W, D, SKIP, FORM>;
    else return nullptr;
}

// One row per built shape: what identifies it, the chunks of its weight stream (the kernel copies that many bias rows), its
// render launcher per variant and its query launcher.  A null launcher: not built.
struct ShapeRow {
    int W, D, skip, form, n_chunks;
    RenderLauncher render[kVariants];
    QueryLauncher query;
};
#define NWE_SHAPE_ROW(W_, D_, SKIP_, FORM_)                                                                                  \
    {W_, D_, SKIP_, FORM_, Shape<W_, D_>::n_chunks(FORM_),                                                                   \
     {render_launcher<W_, D_, SKIP_, FORM_, kVariantPlain>(), render_launcher<W_, D_, SKIP_, FORM_, kVariantTerm>(),         \
      render_launcher<W_, D_, SKIP_, FORM_, kVariantShare>(), render_launcher<W_, D_, SKIP_, FORM_, kVariantTail>()},        \
     query_launcher<W_, D_, SKIP_, FORM_>()},
static const ShapeRow kShapes[] = {NWE_SHAPES(NWE_SHAPE_ROW)};
#undef NWE_SHAPE_ROW

static const ShapeRow* find_shape(int D, int W, int skip, int form) {
    for (const ShapeRow& r : kShapes)
        if (r.W == W && r.D == D && r.skip == skip && r.form == form) return &r;
    return nullptr;
}

bool mfma_supported(int D, int W, int in_xyz, int in_dir, int skip, int form) {
    if (in_xyz != 63 || in_dir != (form == kFormNoViewDirs ? 0 : 27)) return false;
    return find_shape(D, W, skip, form) != nullptr;
}

bool mfma_term_supported(int D, int W, int skip, int form) {
    const ShapeRow* shape = find_shape(D, W, skip, form);
    return shape && shape->render[kVariantTerm];
}

bool mfma_share_supported(int D, int W, int skip, int form) {
    const ShapeRow* shape = find_shape(D, W, skip, form);
    return shape && shape->render[kVariantShare];
}

bool mfma_is_lean(const RenderArgs& a) { return is_lean(a); }

int mfma_max_samples() { return kSplitMaxSamples; }

static int device_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus > 0 ? cus : 256;
}

// The plan of a call: 0 = all packets, 1 = all sample-split, 2 = hybrid; *full = the rays of the hybrid plan's first launch.
static int plan_launch(const RenderArgs& a, int decomposition, int cus, int64_t* full_out) {
    // One workgroup per CU at a time, so a launch costs (rounds of workgroups) x (sample iterations per workgroup).  Three
    // plans, same arithmetic: all packets; all sample-split (finer units, ~6 % overhead: redundant sequential part and
    // exchange); or the full rounds as packets and the ragged last round sample-split in a second launch behind it.
    const int64_t rays_wg = kWaves * kRaysPerWave;
    // the sample iterations this launch runs: both passes, or - shared coarse pass - the producer's coarse pass alone, the
    // consumer's fine pass alone
    const int s_coarse = share_role(a) == kShareConsumer ? 0 : a.n_samples;
    const int s_fine = share_role(a) == kShareProducer || a.n_importance <= 0 ? 0 : a.n_samples + a.n_importance;
    const double its = (double)(s_coarse + s_fine);
    const double its_split = 1.06 * (double)((s_coarse + 3) / 4 + (s_fine + 3) / 4);
    const auto rounds = [&](int64_t rays, int64_t per_wg) { return (double)(((rays + per_wg - 1) / per_wg + cus - 1) / cus); };
    const int64_t full = (a.n_rays / rays_wg / cus) * cus * rays_wg;            // rays in complete rounds of packet workgroups
    const double t_packet = rounds(a.n_rays, rays_wg) * its;
    const double t_split = rounds(a.n_rays, kRaysPerWave) * its_split;
    const double t_hybrid = full > 0 && full < a.n_rays ? (double)(full / rays_wg / cus) * its + rounds(a.n_rays - full, kRaysPerWave) * its_split : 1e300;
    // two launches when the model promises at least 0.8 %: the 800x800 frame (19 full rounds + 136 workgroups) is 1.0 % by the
    // model and measures -0.4 % (368.4 vs 370.0 ms, alternating, tools/plan_ab.py); a second launch costs a few microseconds
    const double t_single = t_packet <= t_split ? t_packet : t_split;
    int plan = t_hybrid < 0.992 * t_single ? 2 : (t_packet <= t_split ? 0 : 1);
    if (decomposition >= 0) plan = decomposition;   // nwe_debug_set_decomposition: tests force one
    if (a.n_samples > kPacketMaxSamples) plan = 1;  // only the single-packet workgroup has LDS for that many coarse weights
    *full_out = full;
    return plan;
}

bool mfma_queues(const RenderArgs& a, int decomposition, int queue_mode) {
    if (queue_mode == 0) return false;
    int64_t full = 0;
    const int cus = device_cus();
    const int plan = plan_launch(a, decomposition, cus, &full);
    const auto queued = [&](int64_t rays, bool split) { return rays > 0 && (queue_mode == 1 || mfma_workgroups(rays, split) > (unsigned)cus); };
    return plan == 2 ? queued(full, false) || queued(a.n_rays - full, true) : queued(a.n_rays, plan == 1);
}

bool launch_render_mfma(const RenderArgs& a, const NetMfma& nc, const NetMfma& nf, bool three_pass, int decomposition, hipStream_t stream,
                        LaunchInfo* info) {
    if (a.n_importance > 0 && (nf.D != nc.D || nf.W != nc.W || nf.skip != nc.skip || nf.form != nc.form)) return false;
    if (a.n_samples > kSplitMaxSamples) return false;
    const int D = nc.D, W = nc.W, skip = nc.skip, form = nc.form;
    // early termination (a.min_trans > 0): the shape's terminating kernels, which exist for lean calls only (nwe_abi.hip refuses
    // the rest by name before it gets here)
    const bool term = a.min_trans > 0.f;
    if (term && (!is_lean(a) || !a.evals || !mfma_term_supported(D, W, skip, form))) return false;
    // shared coarse pass (a.share) of a lean call: the shape's sharing kernels, under the same conditions.  A call that is
    // not lean carries a role only under separate passes (nwe_abi.hip): its two launches are full kernels, which do not read
    // it - the coarse one renders a single pass, the fine one takes the coarse weights from a.w_in - and plan_launch costs each
    // by its role
    const bool share = a.share != kShareOff && is_lean(a);
    if (a.share != kShareOff && !share && (term || (share_role(a) == kShareProducer ? a.n_importance != 0 : !a.w_in))) return false;
    if (share && (term || !a.share_w || a.n_importance <= 0 || !mfma_share_supported(D, W, skip, form))) return false;
    const ShapeRow* shape = find_shape(D, W, skip, form);
    if (!shape) return false;
    const RenderLauncher launch = shape->render[term ? kVariantTerm : share ? kVariantShare : kVariantPlain];
    const RenderLauncher launch_tail = shape->render[kVariantTail];
    if (!launch) return false;
    if (nc.n_chunks != shape->n_chunks || (a.n_importance > 0 && nf.n_chunks != shape->n_chunks)) return false;   // the kernel copies n_chunks bias rows
    int64_t full = 0;
    const int cus = device_cus();
    const int plan = plan_launch(a, decomposition, cus, &full);
    if (info) { info->plan = plan; info->rays_first = plan == 2 ? full : a.n_rays; info->mid_recorded = false; }
    // Dealing: the hardware hands workgroup b of a launch to XCD (b + c) mod 8, an eighth of the launch each
    // whatever pace an XCD runs at.  A queued launch deals tickets instead (render_mfma_kernel), from a counter of its own.
    // i = the launch of the plan; returns the arguments that launch takes.
    const bool may_queue = info && info->queue && !term && !share;
    const auto dealt = [&](int i, int64_t rays, bool split) {
        RenderArgs q = a;
        const unsigned wgs = mfma_workgroups(rays, split);
        if (may_queue && rays > 0 && (info->queue_mode == 1 || wgs > (unsigned)cus)) {
            q.queue = info->queue + i;
            info->items[i] = wgs; info->grid[i] = queue_grid(wgs);
        }
        return q;
    };
    if (plan == 2) {
        RenderArgs first = dealt(0, full, false);
        RenderArgs second = dealt(1, a.n_rays - full, true);
#ifdef NWE_STAMPS   // the second launch's stamp rows lie behind the first's: rows are indexed by work item within a launch
        if (second.stamps) second.stamps += (size_t)mfma_workgroups(full, false) * kWaves * kStampWords;
#endif
        const bool backfill = info && info->side && info->fork && info->join;
        // The tail path: the surplus workgroups of the queued packets launch render the split items, one ticket each from the
        // call's third counter, and the second launch - the same kernel, behind the first on the device - renders what they
        // left, which is nothing when the surplus covers every item; only then is the path taken.  Otherwise nothing changes.
#ifdef NWE_STAMPS
        RenderArgs plain = a; plain.stamps = nullptr;
        const bool lean = is_lean(plain);
#else
        const bool lean = is_lean(a);
#endif
        const unsigned items1 = mfma_workgroups(a.n_rays - full, true);
        if (first.queue && backfill && info->tail && lean && !term && !share && launch_tail && a.n_rays > full &&
            info->grid[0] - info->items[0] >= items1) {
            first.tail = second.tail = info->queue + 2;
            second.share = kTailSecond;
            launch_tail(first, nc, nf, three_pass, false, 0, full, stream);
            if (info->mid) info->mid_recorded = hipEventRecord(info->mid, stream) == hipSuccess;
            info->tail_items = items1;
            // the side stream starts behind the first launch here: the second reads the third counter's final value
            hipStream_t second_stream = stream;
            if (hipEventRecord(info->fork, stream) == hipSuccess && hipStreamWaitEvent(info->side, info->fork, 0) == hipSuccess)
                second_stream = info->side;
            launch_tail(second, nc, nf, three_pass, true, full, a.n_rays - full, second_stream);
            if (second_stream != stream) {
                info->side_used = true;
                if (hipEventRecord(info->join, second_stream) != hipSuccess || hipStreamWaitEvent(stream, info->join, 0) != hipSuccess) return false;
            }
            return true;
        }
        // With queues on, the second launch backfills the first: it goes to the side stream, which forks from the caller's
        // stream in front of the first launch, so that its quarter-size work items are there for a CU the moment the packet
        // items run out; the side stream's low priority keeps them behind the packets until then.
        hipStream_t second_stream = stream;
        if (backfill && (first.queue || second.queue) &&
            hipEventRecord(info->fork, stream) == hipSuccess && hipStreamWaitEvent(info->side, info->fork, 0) == hipSuccess)
            second_stream = info->side;
        launch(first, nc, nf, three_pass, false, 0, full, stream);
        if (info && info->mid) info->mid_recorded = hipEventRecord(info->mid, stream) == hipSuccess;   // the two launches timed apart
        launch(second, nc, nf, three_pass, true, full, a.n_rays - full, second_stream);
        if (second_stream != stream) {
            info->side_used = true;
            // the caller's stream goes on when the side launch has finished; if that cannot be queued the caller is told
            if (hipEventRecord(info->join, second_stream) != hipSuccess || hipStreamWaitEvent(stream, info->join, 0) != hipSuccess) return false;
        }
    } else {
        launch(dealt(0, a.n_rays, plan == 1), nc, nf, three_pass, plan == 1, 0, a.n_rays, stream);
    }
    return true;
}

// ---- point query (nwe_query_points) ----

int query_steps(int64_t packets, int forced) {
    if (forced > 0) return forced < kQueryMaxSteps ? forced : kQueryMaxSteps;
    const int64_t steps = packets / (8 * (int64_t)device_cus());   // the rule: nwe_host.h
    return (int)(steps < 1 ? 1 : (steps > kQueryMaxSteps ? kQueryMaxSteps : steps));
}

bool launch_query_mfma(const QueryArgs& a_in, const NetMfma& net, bool three_pass, int forced_steps, hipStream_t stream) {
    const ShapeRow* shape = find_shape(net.D, net.W, net.skip, net.form);
    if (!shape || !shape->query || net.n_chunks != shape->n_chunks) return false;   // the kernel copies n_chunks bias rows
    if (a_in.n_points <= 0) return true;
    QueryArgs a = a_in;
    const int64_t packets = ((int64_t)a.n_points + kQueryPacket - 1) / kQueryPacket;
    a.steps = query_steps(packets, forced_steps);
    shape->query(a, net, three_pass, (unsigned)((packets + a.steps - 1) / a.steps), stream);
    return true;
}

}  // namespace nwe
