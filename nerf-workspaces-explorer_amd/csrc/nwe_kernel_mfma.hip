// Dispatch of the MFMA render kernel (templates: nwe_mfma_kernels.h; the plan of a call: nwe_plan.cpp).  This file compiles no kernel: the
// instantiations are translation units of their own (nwe_mfma_inst.hip, once per group of nwe_mfma_shapes.h and kernel variant)
// so that they build in parallel, and are reached through the table below.
#include "nwe_mfma_kernels.h"
#include "nwe_mfma_query.h"

namespace nwe {

#define NWE_DECLARE_SHAPE(W_, D_, SKIP_, FORM_)                                                                                   \
    NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantPlain) NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantTerm)   \
    NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantShare) NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantOcc)    \
    NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantTail) NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, kVariantList)    \
    NWE_EXTERN_SHAPE_QUERY_LAUNCHER(W_, D_, SKIP_, FORM_) NWE_EXTERN_SHAPE_QUERY_COUNTED_LAUNCHER(W_, D_, SKIP_, FORM_)
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
using QueryCountedLauncher = void (*)(QueryArgs, const NetMfma&, const uint32_t*, bool, unsigned, hipStream_t);

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
template <int W, int D, int SKIP, int FORM>
constexpr QueryCountedLauncher query_counted_launcher() {
    if constexpr (kQueryLinked) return launch_one_query_counted<W, D, SKIP, FORM>;
    else return nullptr;
}

// One row per built shape: what identifies it, the chunks of its weight stream (the kernel copies that many bias rows), its
// render launcher per variant and its two query launchers.  A null launcher: not built.
struct ShapeRow {
    int W, D, skip, form, n_chunks;
    RenderLauncher render[kVariants];
    QueryLauncher query;
    QueryCountedLauncher query_counted;
};
#define NWE_SHAPE_ROW(W_, D_, SKIP_, FORM_)                                                                                  \
    {W_, D_, SKIP_, FORM_, Shape<W_, D_>::n_chunks(FORM_),                                                                   \
     {render_launcher<W_, D_, SKIP_, FORM_, kVariantPlain>(), render_launcher<W_, D_, SKIP_, FORM_, kVariantTerm>(),         \
      render_launcher<W_, D_, SKIP_, FORM_, kVariantShare>(), render_launcher<W_, D_, SKIP_, FORM_, kVariantOcc>(),          \
      render_launcher<W_, D_, SKIP_, FORM_, kVariantTail>(), render_launcher<W_, D_, SKIP_, FORM_, kVariantList>()},         \
     query_launcher<W_, D_, SKIP_, FORM_>(), query_counted_launcher<W_, D_, SKIP_, FORM_>()},
static_assert(kVariantPlain == 0 && kVariantTerm == 1 && kVariantShare == 2 && kVariantOcc == 3 && kVariantTail == 4 && kVariantList == 5 &&
              kVariants == 6,
              "a row lists its launchers in the order of Variant");
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

bool mfma_variant_built(int D, int W, int skip, int form, int variant) {
    const ShapeRow* shape = find_shape(D, W, skip, form);
    return shape && variant >= 0 && variant < kVariants && shape->render[variant];
}

bool mfma_is_lean(const RenderArgs& a) { return is_lean(a); }

bool launch_render_mfma(const RenderArgs& a, const NetMfma& nc, const NetMfma& nf, bool three_pass, const PassPlan& p,
                        const LaunchResources& res, hipStream_t stream, LaunchReport* out) {
    if (!p.ok) return false;
    if (a.n_importance > 0 && (nf.D != nc.D || nf.W != nc.W || nf.skip != nc.skip || nf.form != nc.form)) return false;
    if (a.n_samples > kSplitMaxSamples) return false;
    const ShapeRow* shape = find_shape(nc.D, nc.W, nc.skip, nc.form);
    if (!shape) return false;
    // the tail path runs both launches through the tail kernel
    const RenderLauncher launch = shape->render[p.tail ? kVariantTail : p.variant];
    if (!launch) return false;
    if (nc.n_chunks != shape->n_chunks || (a.n_importance > 0 && nf.n_chunks != shape->n_chunks)) return false;   // the kernel copies n_chunks bias rows
    // the arguments launch i of the plan takes: a queued launch deals tickets from the call's counter i
    const auto dealt = [&](int i) {
        RenderArgs q = a;
        if (p.launch[i].grid) q.queue = res.counters + i;
        return q;
    };
    const auto issue = [&](const RenderArgs& q, int i, hipStream_t s) {
        launch(q, nc, nf, three_pass, p.launch[i].split, p.launch[i].ray_first, p.launch[i].rays, s);
    };
    if (p.n_launches == 1) {
        issue(dealt(0), 0, stream);
        return true;
    }
    RenderArgs first = dealt(0), second = dealt(1);
#ifdef NWE_STAMPS   // the second launch's stamp rows lie behind the first's: rows are indexed by work item within a launch
    if (second.stamps) second.stamps += (size_t)p.launch[0].items * kWaves * kStampWords;
#endif
    if (p.tail) {
        first.tail = second.tail = res.counters + 2;
        second.share = kTailSecond;
    }
    // the side stream takes the second launch only if it can be made to start behind the fork
    hipStream_t second_stream = stream;
    const auto fork = [&] {
        if (res.side && hipEventRecord(res.fork, stream) == hipSuccess && hipStreamWaitEvent(res.side, res.fork, 0) == hipSuccess)
            second_stream = res.side;
    };
    if (p.fork == kForkFront) fork();
    issue(first, 0, stream);
    if (res.mid) out->mid_recorded = hipEventRecord(res.mid, stream) == hipSuccess;   // the two launches timed apart
    if (p.fork == kForkBehind) fork();
    issue(second, 1, second_stream);
    if (second_stream != stream) {
        out->side_used = true;
        // the caller's stream goes on when the side launch has finished; if that cannot be queued the caller is told
        if (hipEventRecord(res.join, second_stream) != hipSuccess || hipStreamWaitEvent(stream, res.join, 0) != hipSuccess) return false;
    }
    return true;
}

// ---- point query (nwe_query_points) ----

bool launch_query_mfma(const QueryArgs& a_in, const NetMfma& net, bool three_pass, int forced_steps, int cus, hipStream_t stream) {
    const ShapeRow* shape = find_shape(net.D, net.W, net.skip, net.form);
    if (!shape || !shape->query || net.n_chunks != shape->n_chunks) return false;   // the kernel copies n_chunks bias rows
    if (a_in.n_points <= 0) return true;
    QueryArgs a = a_in;
    const int64_t packets = ((int64_t)a.n_points + kQueryPacket - 1) / kQueryPacket;
    a.steps = query_steps(packets, forced_steps, cus);
    shape->query(a, net, three_pass, (unsigned)((packets + a.steps - 1) / a.steps), stream);
    return true;
}

bool launch_query_mfma_counted(const QueryArgs& a_in, const uint32_t* count, const NetMfma& net, bool three_pass, int forced_steps, int cus,
                               hipStream_t stream) {
    const ShapeRow* shape = find_shape(net.D, net.W, net.skip, net.form);
    if (!shape || !shape->query_counted || net.n_chunks != shape->n_chunks) return false;   // the kernel copies n_chunks bias rows
    if (a_in.n_points <= 0) return true;
    QueryArgs a = a_in;
    a.steps = 0;   // not read: the walk is strided over the grid
    shape->query_counted(a, net, count, three_pass, query_counted_grid(a.n_points, kQueryPacket, forced_steps, cus), stream);
    return true;
}

}  // namespace nwe
