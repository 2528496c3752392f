// C ABI of libnwe_hip.so (include/nwe.h): the context and what the units of the ABI share (nwe_ctx.h), networks and sampling, the
// render, tiled, ray and query calls, their reports, the debug switches.  The grids: nwe_abi_grids.hip; the sparse frames:
// nwe_abi_sparse.hip; the adaptive frame: nwe_abi_adaptive.hip; the pixel list: nwe_abi_pixels.hip.  Weight packing: nwe_pack.cpp; planning: nwe_plan.cpp; the refusals: nwe_check.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "nwe_ctx.h"
#include "nwe_pack.h"

namespace {
thread_local std::string g_create_error;
}

namespace nwe {

int fail(nwe_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// The context as plain data, read here and nowhere else: what a call is checked against (nwe_check.h) and planned from (describe_call).
ContextDesc describe_context(const nwe_ctx* c) {
    ContextDesc d;
    for (int i = 0; i < 2; ++i) d.net[i] = c->net[i];
    d.ns = c->ns; d.ni = c->ni; d.host_only = c->host_only;
    d.min_trans = c->min_trans; d.share_k = c->share_k; d.separate = c->separate != 0;
    d.occ.set = c->occ.set; d.cgrid.set = c->cgrid.set; d.rgrid.set = c->rgrid.set;
    for (int i = 0; i < 3; ++i) { d.occ.res[i] = c->occ.box.res[i]; d.cgrid.res[i] = c->cgrid.box.res[i]; d.rgrid.res[i] = c->rgrid.box.res[i]; }
    d.stamps = c->stamps != nullptr;
    d.decomposition = c->decomposition; d.queue_mode = c->work_queue;
    d.backfill = c->backfill; d.tail = c->tail; d.packet_blocks = c->packet_blocks;
    return d;
}

// Makes a slot ready for a new launch: waits for the launch that used it last (for a render slot that was kSlots launches
// ago, normally long finished).  From here on the slot's events describe no launch until a new one has been recorded.
int prepare_slot(nwe_ctx* c, Slot& s) {
    if (!s.ev0)
        for (Event* e : {&s.ev0, &s.ev1}) HIPCHK(c, hipEventCreate(&e->h));
    if (s.used) HIPCHK(c, hipEventSynchronize(s.ev1));
    s.used = false;
    for (bool& read : s.time_read) read = false;
    return NWE_OK;
}
int prepare_slot(nwe_ctx* c, RenderSlot& s) {
    if (!s.ev_mid)
        for (Event* e : {&s.ev_mid, &s.ev_share}) HIPCHK(c, hipEventCreate(&e->h));
    s.has_mid = s.has_share = false;
    return prepare_slot(c, static_cast<Slot&>(s));
}

// The sparse calls in flight, on whatever streams they are: a synchronous one has been waited for unless it failed half way, an
// asynchronous one ends in its slot's ev1.  *waits counts the slots that had not finished yet.
int wait_for_sparse(nwe_ctx* c, int* waits) {
    for (SparseSlot& s : c->sparse.slots) {
        if (!s.used) continue;
        if (waits && hipEventQuery(s.ev1) != hipSuccess) { ++*waits; (void)hipGetLastError(); }
        HIPCHK(c, hipEventSynchronize(s.ev1));
    }
    return NWE_OK;
}

// nwe_set_sampling and nwe_set_network change device memory that a queued launch reads (the sampling tables are copied
// into LDS by every workgroup as it starts, the weights are streamed throughout): wait for this context's own launches,
// on whatever streams they are.  Costs nothing when nothing is in flight.
int wait_for_launches(nwe_ctx* c) {
    for (RenderSlot& s : c->render.slots)
        if (s.used) HIPCHK(c, hipEventSynchronize(s.ev1));
    if (c->rays_slot.used) HIPCHK(c, hipEventSynchronize(c->rays_slot.ev1));
    if (c->adaptive_slot.used) HIPCHK(c, hipEventSynchronize(c->adaptive_slot.ev1));   // synchronous: long passed
    if (c->adaptive_levels_slot.used) HIPCHK(c, hipEventSynchronize(c->adaptive_levels_slot.ev1));
    for (Slot& s : c->query.slots)  // a query streams the weights of its network throughout
        if (s.used) HIPCHK(c, hipEventSynchronize(s.ev1));
    for (Slot& s : c->grid.slots)    // a grid frame reads the sampling tables and the radiance grid
        if (s.used) HIPCHK(c, hipEventSynchronize(s.ev1));
    return wait_for_sparse(c, nullptr);   // a sparse frame reads all of it
}

// Poses into the slot's own table (its last reader finished: prepare_slot).  hipMemcpyAsync from pageable host memory is
// staged by the runtime before it returns, so the caller's array is free on return; from pinned memory the copy is truly
// asynchronous and include/nwe.h asks the caller to keep the array alive until the stream has passed it.
int upload_poses(nwe_ctx* c, Slot& s, const float* c2w, int n_poses, hipStream_t stream) {
    HIPCHK(c, s.poses.reserve((size_t)std::max(n_poses, 64) * 16));
    HIPCHK(c, hipMemcpyAsync(s.poses.get(), c2w, (size_t)n_poses * 16 * sizeof(float), hipMemcpyHostToDevice, stream));
    return NWE_OK;
}

// The camera part of RenderArgs: rays are generated in the kernel from the pose table `poses_dev`.
RenderArgs camera_args(const Camera& m, const float* poses_dev) {
    RenderArgs a = {};
    a.poses = poses_dev;
    a.H = m.H; a.W = m.W; a.row_begin = m.row_begin; a.rows = m.row_end - m.row_begin;
    a.n_rays = (int64_t)m.n_poses * a.rows * m.W;
    a.fx = m.fx; a.fy = m.fy; a.cx = m.cx; a.cy = m.cy; a.near = m.near; a.far = m.far;
    return a;
}

// What the context holds for every render call: background, sampling tables and counts, the modes' kernel arguments.
void context_args(const nwe_ctx* ctx, RenderArgs& a) {
    a.white_bkgd = ctx->white_bkgd;
    a.t_vals = ctx->d_t.get();   // null on a host-only context, which plans and never launches
    if (a.t_vals) { a.omt_vals = a.t_vals + kMaxSamples; a.u_vals = a.omt_vals + kMaxSamples; }
    a.n_samples = ctx->ns; a.n_importance = ctx->ni;
    a.stamps = ctx->stamps;   // only read by -DNWE_STAMPS builds of the kernel (nwe_debug_set_stamps)
    a.min_trans = ctx->min_trans;
}

RenderArgs frame_args(const nwe_ctx* c, const Camera& m, const float* poses_dev, float* rgb, float* depth, float* acc, uint32_t* flags) {
    RenderArgs a = camera_args(m, poses_dev);
    a.white_bkgd = c->white_bkgd;   // nothing else of the context: the sampling tables and counts, no mode
    a.t_vals = c->d_t.get(); a.omt_vals = a.t_vals + kMaxSamples; a.u_vals = a.omt_vals + kMaxSamples;
    a.n_samples = c->ns; a.n_importance = c->ni;
    a.out.struct_bytes = sizeof(nwe_outputs);
    a.out.rgb = rgb; a.out.depth = depth; a.out.acc = acc; a.out.flags = flags;
    return a;
}

// The time between two events of the launch that slot `s` describes (both have passed): read once, then the same value.
hipError_t kept_time(const Slot& s, int which, hipEvent_t from, hipEvent_t to, float* ms) {
    if (!s.time_read[which]) {
        const hipError_t e = hipEventElapsedTime(&s.time_ms[which], from, to);
        if (e != hipSuccess) return e;
        s.time_read[which] = true;
    }
    *ms = s.time_ms[which];
    return hipSuccess;
}

// nwe_last_kernel_ms and its like: the time between the events of a recorded launch (a ring's last()); -1 where there is none, or -1
// and the context's error
float elapsed_ms(nwe_ctx* c, const Slot* last, const char* who) {
    if (!last) return -1.f;
    const Slot& s = *last;
    DeviceGuard guard;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipEventSynchronize(s.ev1);
    float ms = -1.f;
    if (e == hipSuccess) e = kept_time(s, Slot::kWhole, s.ev0, s.ev1, &ms);
    if (e != hipSuccess) { c->err = std::string(who) + ": " + hipGetErrorString(e); (void)hipGetLastError(); return -1.f; }
    return ms;
}

int run_query(nwe_ctx* c, const NetState& net, const QueryArgs& q, int precision, hipStream_t stream, const uint32_t* count) {
    const bool f32 = precision == NWE_PREC_F32, three_pass = precision == NWE_PREC_F16X3;
    bool ok = true;
    if (f32 && count) launch_query_f32_counted(q, count, net.f32, c->query_steps, c->cus, stream);
    else if (f32) launch_query_f32(q, net.f32, c->query_steps, c->cus, stream);
    else if (count) ok = launch_query_mfma_counted(q, count, net.mf, three_pass, c->query_steps, c->cus, stream);
    else ok = launch_query_mfma(q, net.mf, three_pass, c->query_steps, c->cus, stream);
    return ok ? NWE_OK : fail(c, NWE_ERR_UNSUPPORTED, "no MFMA query kernel in this build for this network shape; use NWE_PREC_F32");
}

}  // namespace nwe

namespace {

__global__ void to8b_kernel(const float* __restrict__ x, uint8_t* __restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {   // model_utils.py:9: (255 * clip(x, 0, 1)).astype(uint8) -- truncation
        const float v = 255.f * fminf(fmaxf(x[i], 0.f), 1.f);
        y[i] = (uint8_t)(int)v;
    }
}

__global__ void or_flags_kernel(const uint32_t* __restrict__ parts, int n, uint32_t* __restrict__ out) {
    uint32_t f = 0;
    for (int i = 0; i < n; ++i) f |= parts[i];
    if (f) atomicOr(out, f);
}

// Separate passes: the coarse launch of a full kernel is a single-pass render, which also reports its composite under the
// main outputs' bits; only the bits in `mask` (the coarse outputs' and NWE_FLAG_RAW) reach the caller's word.
__global__ void or_masked_flags_kernel(const uint32_t* __restrict__ word, uint32_t mask, uint32_t* __restrict__ out) {
    const uint32_t f = *word & mask;
    if (f) atomicOr(out, f);
}

__global__ void create_rays_kernel(RenderArgs a, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_rays) return;
    const Ray r = load_ray(a, i);
    float* o = out + i * 11;
    o[0] = r.ox; o[1] = r.oy; o[2] = r.oz; o[3] = r.dx; o[4] = r.dy; o[5] = r.dz;
    o[6] = r.near; o[7] = r.far; o[8] = r.vx; o[9] = r.vy; o[10] = r.vz;
}

// The one-shot hooks of nwe_render_rays (nwe_debug_set_fine_depths / _raw / _coarse_weights, nwe_set_train_tables) are
// consumed by the call whatever becomes of it: a refused call must not leave them armed for a later one.
struct HookReset {
    nwe_ctx* c;
    ~HookReset() {
        if (!c) return;
        c->dbg_z_fine = c->dbg_raw_c = c->dbg_raw_f = c->dbg_w = nullptr;
        c->trn_t = c->trn_nc = c->trn_nf = c->trn_u = nullptr;
    }
};

#ifdef NWE_STAMPS
constexpr bool kStampedBuild = true;
#else
constexpr bool kStampedBuild = false;
#endif

// The call as the planner sees it (nwe_plan.h): `a` as the entry point and context_args() filled it, the context's modes.
CallDesc describe_call(const ContextDesc& ctx, const RenderArgs& a, int precision, bool list = false) {
    CallDesc d;
    d.n_rays = a.n_rays;
    RenderArgs consumer = a;
    consumer.share = kShareConsumer | ctx.share_k << 8;
    d.n_rep = share_n_rep(consumer, share_grid(consumer));   // at most n_rays
    d.n_samples = a.n_samples; d.n_importance = a.n_importance;
    d.mfma = precision != NWE_PREC_F32;
    d.term = a.min_trans > 0.f;
    d.occ = ctx.occ.set;
    d.share_k = ctx.share_k; d.separate = ctx.separate;
    d.baked = ctx.cgrid.set;   // check_ready has let nothing but lean pinhole calls through
    RenderArgs unstamped = a;
    unstamped.stamps = nullptr;
    d.list = list;
    if (list) unstamped.rays = nullptr;   // the pixel list, no ray table: the list kernels make the rays themselves
    d.lean = mfma_is_lean(unstamped); d.stamps = a.stamps != nullptr; d.stamped_build = kStampedBuild;
    d.w_in = a.w_in != nullptr;
    d.want_weights_coarse = a.out.weights_coarse != nullptr; d.want_flags = a.out.flags != nullptr;
    for (int i = 0; i < 2; ++i)
        for (int v = 0; v < kVariants; ++v) d.built[i][v] = ctx.net[i].set && ctx.net[i].mfma_ok && ctx.net[i].built[v];
    d.decomposition = ctx.decomposition; d.queue_mode = ctx.queue_mode;
    d.backfill = ctx.backfill; d.tail = ctx.tail;
    if (!a.rays) { d.rows = a.rows; d.width = a.W; }
    d.packet_blocks = ctx.packet_blocks;
    return d;
}

// What the plan asks of the slot, reserved and - on the caller's stream - zeroed (the last reader of each has finished: prepare_slot).
int provide(nwe_ctx* ctx, RenderSlot& slot, const CallPlan& p, hipStream_t stream) {
    if (p.need_evals) {   // the launch's waves add their ray evaluations to the slot's own word
        HIPCHK(ctx, slot.evals.reserve(1));
        HIPCHK(ctx, hipMemsetAsync(slot.evals.get(), 0, sizeof(unsigned long long), stream));
    }
    HIPCHK(ctx, slot.share_w.reserve((size_t)p.table_elems));
    if (p.coarse_flags) {
        HIPCHK(ctx, slot.coarse_flags.reserve(1));
        HIPCHK(ctx, hipMemsetAsync(slot.coarse_flags.get(), 0, sizeof(uint32_t), stream));
    }
    if (p.may_queue) HIPCHK(ctx, slot.queue.reserve(4));   // LaunchResources::counters, zeroed in front of the main stage
    // every slot's stream with the first call that queues a launch, not one with each of the ring's first four: creating a stream takes
    // milliseconds, which belong to a context's first frame and to no later one.  The lowest priority there is, so that the
    // quarter-size work items wait behind the packets until those run out.
    for (RenderSlot& s : ctx->render.slots) {
        if (!p.need_side || s.side) continue;
        int least = 0, greatest = 0;
        HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(ctx, hipStreamCreateWithPriority(&s.side.h, hipStreamNonBlocking, least));
        for (Event* e : {&s.ev_fork, &s.ev_join}) HIPCHK(ctx, hipEventCreateWithFlags(&e->h, hipEventDisableTiming));
    }
    return NWE_OK;
}

// The stages' kernel arguments from the call's: `a` becomes the main stage's; returns the coarse stage's (unused without one).
RenderArgs stage_args(const CallPlan& p, const RenderSlot& slot, RenderArgs& a) {
    RenderArgs prod = {};
    if (p.need_evals) a.evals = slot.evals.get();
    if (p.main.role != kShareOff) a.share = p.main.role | p.share_k << 8;   // the full kernels do not read it: it costs the launch by its role
    if (p.share) a.share_w = slot.share_w.get();
    if (p.coarse.active) {
        prod = a;
        prod.share = p.coarse.role | p.share_k << 8; prod.n_rays = p.coarse.n_rays; prod.n_importance = p.coarse.n_importance;
        prod.out = {};
        if (p.share) {
            // k = 1 (separate passes): every ray runs its own coarse pass, whose flag bits are the fused kernel's; a representative's
            // coarse pass (k > 1) describes no ray of the call
            if (p.share_k == 1) prod.out.flags = a.out.flags;
        } else {   // the single-pass render of the full kernels, whose weights_coarse output is the table: the caller's own if it asked for one
            float* table = a.out.weights_coarse ? a.out.weights_coarse : slot.share_w.get();
            prod.z_fine_in = prod.raw_in_f = prod.noise_f = prod.u_rand = nullptr;
            prod.out.struct_bytes = a.out.struct_bytes;
            prod.out.raw_coarse = a.out.raw_coarse; prod.out.weights_coarse = table;
            prod.out.rgb_coarse = a.out.rgb_coarse; prod.out.depth_coarse = a.out.depth_coarse;
            prod.out.acc_coarse = a.out.acc_coarse; prod.out.disp_coarse = a.out.disp_coarse;
            if (p.coarse_flags) prod.out.flags = slot.coarse_flags.get();
            a.w_in = table;   // read through the coarse-weights hook, which takes the place of pass 0
        }
    }
    if (p.full) {
        a.raw_in_c = a.noise_c = nullptr;   // the coarse launch's
        a.out.raw_coarse = a.out.weights_coarse = a.out.rgb_coarse = a.out.depth_coarse = a.out.acc_coarse = a.out.disp_coarse = nullptr;
    }
    return prod;
}

// A render launch on the ring slot prepare_slot() made ready (ctx->render.next()): describe the call, plan it, carry
// the plan out.  The ring moves on here, once the launch has been recorded.
int launch(nwe_ctx* ctx, const ContextDesc& desc, RenderSlot& slot, RenderArgs& a, int precision, hipStream_t stream, bool list = false,
           uint32_t flags_mask = 0) {
    context_args(ctx, a);
    if (a.n_rays <= 0) return NWE_OK;
    const CallPlan p = plan_call(describe_call(desc, a, precision, list), ctx->cus);
    // a pixel-list call: the launch's flag bits go through a word of the slot's, the masked bits from there to the caller's
    uint32_t* const masked_flags = flags_mask ? a.out.flags : nullptr;
    if (masked_flags) {
        HIPCHK(ctx, slot.pixel_flags.reserve(1));
        HIPCHK(ctx, hipMemsetAsync(slot.pixel_flags.get(), 0, sizeof(uint32_t), stream));
        a.out.flags = slot.pixel_flags.get();
    }
    const bool mfma = precision != NWE_PREC_F32, three_pass = precision == NWE_PREC_F16X3;
    TRY(provide(ctx, slot, p, stream));
    const RenderArgs prod = stage_args(p, slot, a);
    if (p.occ) a.occ = ctx->d_occ.get();   // the slot of `stamps`, which such a call does not have (check_ready)
    if (p.blocks) a.ray_cols |= kPacketBlocksBit;   // a pinhole call: nothing else reads the word (nwe_packet_blocks.h)
    ctx->last_packet_blocks = p.blocks ? 1 : 0;
    const NetState &nc = ctx->net[0], &nf = ctx->net[ctx->ni > 0 ? 1 : 0];
    // the launch's own descriptors: whether its lean kernels may take the hollow path with this network (nwe_debug_set_colour_skip)
    const auto with_skip = [&](const NetState& n) {
        NetMfma m = n.mf;
        m.colour_skip = ctx->colour_skip == 2 || (ctx->colour_skip == 1 && n.p.colour_finite) ? 1 : 0;
        return m;
    };
    const NetMfma mf[2] = {with_skip(nc), with_skip(nf)};
    // one stage: (coarse, fine) in the descriptor slots of one fused kernel, the stage's own network twice under separate passes
    const auto run = [&](const StagePlan& s, const RenderArgs& args, const LaunchResources& res, LaunchReport* report) {
        if (!mfma) {
            if (p.occ) launch_render_f32_occ(args, nc.f32, nf.f32, stream); else launch_render_f32(args, nc.f32, nf.f32, stream);
            return true;
        }
        return launch_render_mfma(args, mf[s.net < 0 ? 0 : s.net], mf[s.net < 0 ? 1 : s.net], three_pass, s.pass, res, stream, report);
    };
    const int rc = record_launch(ctx, slot, stream, [&]() -> int {
        const PassPlan& pass = p.main.pass;
        slot.has_mid = false; slot.rays_total = a.n_rays;
        slot.rays_first = mfma ? pass.launch[0].rays : a.n_rays;
        for (int i = 0; i < 2; ++i) { slot.q_grid[i] = pass.launch[i].grid; slot.q_items[i] = pass.launch[i].grid ? pass.launch[i].items : 0; }
        slot.side_used = false; slot.tail_items = pass.tail_items;
        slot.term = p.need_evals;
        slot.evals_full = p.evals_full; slot.evals_run = p.evals_run; slot.share_rays = p.share_rays;
        const char* shapes_differ = "coarse and fine networks must have the same shape for the MFMA kernel";
        LaunchReport report;
        if (p.baked) {   // the coarse stage is the grid producer: the table from the context's grid, on the caller's stream
            launch_coarse_grid_weights(a, coarse_grid_args(ctx), slot.share_w.get(), nullptr, nullptr, stream);
            HIPCHK(ctx, hipEventRecord(slot.ev_share, stream));
            slot.has_share = true;
        } else if (p.coarse.active) {
            if (!run(p.coarse, prod, LaunchResources{}, &report)) return fail(ctx, NWE_ERR_UNSUPPORTED, shapes_differ);
            if (p.full && prod.out.flags)
                hipLaunchKernelGGL(or_masked_flags_kernel, dim3(1), dim3(1), 0, stream, prod.out.flags,
                                   ~(uint32_t)(NWE_FLAG_RGB | NWE_FLAG_DEPTH | NWE_FLAG_ACC | NWE_FLAG_DISP), a.out.flags);
            HIPCHK(ctx, hipEventRecord(slot.ev_share, stream));
            slot.has_share = true;
        }
        LaunchResources res;
        res.mid = slot.ev_mid;
        if (p.may_queue) {
            HIPCHK(ctx, hipMemsetAsync(slot.queue.get(), 0, 4 * sizeof(unsigned), stream));
            res.counters = slot.queue.get();
            res.side = slot.side; res.fork = slot.ev_fork; res.join = slot.ev_join;
        }
        report = {};
        if (!run(p.main, a, res, &report)) {
            if (!report.side_used) return fail(ctx, NWE_ERR_UNSUPPORTED, shapes_differ);
            // the side launch is queued and the caller's stream could not be made to wait for it: nothing of this call may
            // still run when the call returns its error
            (void)hipStreamSynchronize(slot.side);
            return fail(ctx, NWE_ERR_HIP, std::string("work queue: joining the side stream: ") + hipGetErrorString(hipGetLastError()));
        }
        if (masked_flags) hipLaunchKernelGGL(or_masked_flags_kernel, dim3(1), dim3(1), 0, stream, a.out.flags, flags_mask, masked_flags);
        if (mfma) ctx->last_plan = pass.plan;
        slot.side_used = report.side_used; slot.has_mid = report.mid_recorded;
        return NWE_OK;
    });
    if (rc) return rc;
    ctx->render.commit(slot);
    return NWE_OK;
}

// nwe_render, and one tile of nwe_render_tiled.  Refuses in this order: check_ready, camera, device.
int render_rows(nwe_ctx* c, const Camera& m, int precision, const nwe_outputs* out, hipStream_t stream) {
    const MaybeContext desc(c);
    CHECK(c, check_ready(desc.p, out, precision, true));
    CHECK(c, check_camera(m));
    ON_DEVICE(c);
    RenderSlot& slot = c->render.next();
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, m.c2w, m.n_poses, stream));
    RenderArgs a = camera_args(m, slot.poses.get());
    CHECK(c, check_ray_count(a.n_rays, false));
    a.out = *out;
    return launch(c, desc.d, slot, a, precision, stream);
}

}  // namespace

namespace nwe {

int render_ray_list(nwe_ctx* c, const ContextDesc& desc, const float* rays_dev, int64_t n_rays, int precision, const nwe_outputs& out, bool hooks,
                    hipStream_t stream, uint32_t flags_mask) {
    RenderSlot& slot = c->render.next();
    TRY(prepare_slot(c, slot));
    RenderArgs a = {};
    a.rays = rays_dev; a.n_rays = n_rays; a.W = 1; a.rows = 1;
    a.ray_cols = c->net[0].in_dir == 0 ? 8 : 11;                       // rays.py:22-30: no view-direction columns without view dirs
    if (hooks) {
        a.z_fine_in = c->dbg_z_fine; a.raw_in_c = c->dbg_raw_c; a.raw_in_f = c->dbg_raw_f; a.w_in = c->dbg_w;
        a.t_rand = c->trn_t; a.noise_c = c->trn_nc; a.noise_f = c->trn_nf; a.u_rand = c->trn_u;
    }
    a.out = out;
    return launch(c, desc, slot, a, precision, stream, false, flags_mask);
}

int render_pixel_list(nwe_ctx* c, const ContextDesc& desc, const RenderArgs& cam, int n_poses, const int32_t* list_dev, int64_t n, int precision,
                      const nwe_outputs& out, hipStream_t stream, uint32_t flags_mask) {
    RenderSlot& slot = c->render.next();
    TRY(prepare_slot(c, slot));
    RenderArgs a = cam;
    a.rays = reinterpret_cast<const float*>(list_dev);   // the list kernels read the slot as int32 (render_mfma_list_kernel)
    a.ray_cols = n_poses;                                // ... and clamp a listed pixel to the rays of the camera's own frame
    a.n_rays = n;
    a.out = out;
    return launch(c, desc, slot, a, precision, stream, true, flags_mask);
}

}  // namespace nwe

namespace {

// 1 / 0: device `from` can / cannot read and write `to`'s memory directly; -1: the query failed (*err says how)
int can_access_peer(int from, int to, hipError_t* err = nullptr) {
    int can = 0;
    const hipError_t e = hipDeviceCanAccessPeer(&can, from, to);
    if (err) *err = e;
    if (e != hipSuccess) { (void)hipGetLastError(); return -1; }
    return can ? 1 : 0;
}

// ---- nwe_render_tiled, step by step; c = the context of tile i, c0 = contexts[0], whose device holds the frame ----

// What a tile needs on its device, created on first use: its stream, its event, its flag word, and room for `floats` of results.
int tile_resources(nwe_ctx* c, size_t floats) {
    if (!c->tile_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->tile_stream.h, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->tile_done.h, hipEventDisableTiming));
        HIPCHK(c, c->tile_flags.reserve(1));
    }
    if (c->tile_buf.cap < floats) HIPCHK(c, hipStreamSynchronize(c->tile_stream));   // the copies of earlier frames read the old buffer
    HIPCHK(c, c->tile_buf.reserve(floats));
    return NWE_OK;
}

// Asked once per context: direct xGMI copies into the frame; without peer access the runtime stages the copy through the host.
// Neither outcome fails the call, but the caller can read it (nwe_debug_peer_access, nwe_last_warning).
void probe_peer_access(nwe_ctx* c, nwe_ctx* c0, int i) {
    if (c->peer_access != -2) return;
    c->peer_access = 1;
    if (c->device == c0->device) return;
    hipError_t e = hipSuccess;
    const int can = can_access_peer(c->device, c0->device, &e);
    if (can == 1) {
        e = hipDeviceEnablePeerAccess(c0->device, 0);
        if (e == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); e = hipSuccess; }
    }
    const std::string tile = "tile " + std::to_string(i) + ": ", from = std::to_string(c->device), to = std::to_string(c0->device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c->peer_access = -1;
        c0->warn += tile + "peer access device " + from + " -> " + to + " not enabled (" + hipGetErrorString(e) + "), copies are staged; ";
    } else if (can == 0) {
        c->peer_access = 0;
        c0->warn += tile + "device " + from + " cannot access device " + to + " directly, copies are staged; ";
    }
}

// The caller's frame on c0's device, row-major [n_poses, H, W, C]; a null plane was not asked for.
struct Frame { float *rgb, *depth, *acc; };

// Whatever happens in a tile's step, stream0 must wait for everything this call has queued on the tile stream: the event is
// recorded on EVERY exit of the step once the stream exists (a failing copy after earlier copies were queued would
// otherwise leave stream0 waiting on the previous frame's already-completed event).
struct RecordOnExit {
    nwe_ctx* c;
    ~RecordOnExit() { if (c->tile_done && c->tile_stream && hipEventRecord(c->tile_done, c->tile_stream) != hipSuccess) (void)hipGetLastError(); }
};

// The step of tile i = the rows of `m`, on c's device and stream: wait until the frame is free, render into the tile
// buffer, copy the tile's planes into the frame and its flag word into c0's flag_parts[i].
int queue_tile(nwe_ctx* c, nwe_ctx* c0, int i, const Camera& m, int precision, const Frame& f) {
    HIPCHK(c, hipSetDevice(c->device));
    RecordOnExit record_on_exit{c};
    const size_t px = (size_t)(m.row_end - m.row_begin) * m.W;   // pixels of one pose's tile
    TRY(tile_resources(c, (size_t)m.n_poses * px * 5));
    probe_peer_access(c, c0, i);
    HIPCHK(c, hipStreamWaitEvent(c->tile_stream, c0->frame_ready, 0));
    if (px == 0) return NWE_OK;
    HIPCHK(c, hipMemsetAsync(c->tile_flags.get(), 0, sizeof(uint32_t), c->tile_stream));
    float* t_rgb = c->tile_buf.get();
    float* t_depth = t_rgb + (size_t)m.n_poses * px * 3;
    float* t_acc = t_depth + (size_t)m.n_poses * px;
    nwe_outputs o = {};
    o.struct_bytes = sizeof(nwe_outputs);
    o.rgb = f.rgb ? t_rgb : nullptr; o.depth = f.depth ? t_depth : nullptr; o.acc = f.acc ? t_acc : nullptr;
    o.flags = c->tile_flags.get();
    TRY(render_rows(c, m, precision, &o, c->tile_stream));
    auto copy = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyPeerAsync(dst, c0->device, src, c->device, bytes, c->tile_stream); };
    // tile -> frame: pose p's rows [row_begin, row_end) are contiguous in the row-major [n_poses, H, W, C] frame
    for (int p = 0; p < m.n_poses; ++p) {
        const size_t dst_px = ((size_t)p * m.H + m.row_begin) * m.W, src_px = (size_t)p * px;
        if (f.rgb) HIPCHK(c, copy(f.rgb + dst_px * 3, t_rgb + src_px * 3, px * 3 * sizeof(float)));
        if (f.depth) HIPCHK(c, copy(f.depth + dst_px, t_depth + src_px, px * sizeof(float)));
        if (f.acc) HIPCHK(c, copy(f.acc + dst_px, t_acc + src_px, px * sizeof(float)));
    }
    HIPCHK(c, copy(c0->flag_parts.get() + i, c->tile_flags.get(), sizeof(uint32_t)));
    return NWE_OK;   // record_on_exit records tile_done
}

template <class T>
int upload(nwe_ctx* c, DevBuf<T>& dst, const std::vector<T>& src) {
    HIPCHK(c, dst.reserve(src.size()));
    HIPCHK(c, hipMemcpy(dst.get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return NWE_OK;
}

int set_network(nwe_ctx* c, int which, const NetShape& shape, const float* const* w, const float* const* b) {
    NetState& n = c->net[which];
    n.set = false;   // stays false if anything below fails
    static_cast<NetShape&>(n) = shape;
    if (n.skip < -1 || n.skip >= n.D - 1) n.skip = -1;   // a skip after the last trunk layer never feeds a layer
    n.flops = algo_flops(n);
    pack_f32(n.p, n, w, b);
    n.f32 = n.p.f32;
    n.form = n.in_dir == 0 ? kFormNoViewDirs : (c->fold != 0 ? kFormFolded : kFormReference);
    n.mfma_ok = mfma_supported(n.D, n.W, n.in_xyz, n.in_dir, n.skip, n.form);
    for (int v = 0; v < kVariants; ++v) n.built[v] = mfma_variant_built(n.D, n.W, n.skip, n.form, v);
    if (n.mfma_ok) pack_mfma(n.p, n, n.form, w, b); else { n.p.stream.clear(); n.p.bias_tab.clear(); n.p.n_chunks = 0; }
    n.mf = {};
    n.mf.D = n.D; n.mf.W = n.W; n.mf.skip = n.skip; n.mf.form = n.form;
    n.mf.n_tiles = (int)(n.p.stream.size() / kTileBytes);
    n.mf.n_chunks = n.mfma_ok ? n.p.n_chunks : 0;
    n.mf.inv_scale = 1.f / n.p.w_scale;
    if (!c->host_only) {
        ON_DEVICE(c);
        TRY(wait_for_launches(c));   // a queued launch still streams the old weights
        TRY(upload(c, n.d_blob, n.p.blob));
        if (n.mfma_ok) {
            TRY(upload(c, n.d_stream, n.p.stream));
            TRY(upload(c, n.d_bias, n.p.bias_tab));
        }
        n.f32.blob = n.d_blob.get();
        n.mf.stream = n.mfma_ok ? n.d_stream.get() : nullptr;
        n.mf.bias = n.mfma_ok ? n.d_bias.get() : nullptr;
    }
    n.set = true;
    c->occ.set = false;   // a grid describes the networks it was made for (include/nwe.h); the wait above covers its readers
    if (which == NWE_NET_COARSE) c->cgrid = CoarseGridState{};   // the coarse density grid describes the coarse network
    c->rgrid = RadianceGridState{};   // the radiance grid was baked from a network of this context: either upload clears it
    return NWE_OK;
}

// The accessors' guard: the network `which` of c if it has been set, else null.
const NetState* set_net(const nwe_ctx* c, int which) { return c && which >= 0 && which <= 1 && c->net[which].set ? &c->net[which] : nullptr; }

// The least nwe_last_launch_parts reports for a part, in ms: the 10 ns step of the event timer
constexpr float kMinPartMs = 1e-5f;

// The most recent recorded render launch (nwe_last_kernel_ms, nwe_last_launch_parts), or null
const RenderSlot* last_render(const nwe_ctx* c) { return c->host_only ? nullptr : c->render.last(); }

// A switch of the environment that a new context starts from (A/B timing on one library): 0 or 1, or -1 for anything else
int env_switch(const char* name) {
    const char* e = std::getenv(name);
    return e && (e[0] == '0' || e[0] == '1') && !e[1] ? e[0] - '0' : -1;
}

}  // namespace

extern "C" {

int nwe_create(nwe_ctx** out, int device) {
    if (!out) return fail(nullptr, NWE_ERR_INVALID, "out is null");
    nwe_ctx* c = new nwe_ctx();
    c->device = device;
    c->host_only = device < 0;
    // the defaults of a new context: the queue, its backfill (which only 0 changes), its tail path, the hollow path, the 8x4 packets
    if (const int v = env_switch("NWE_WORK_QUEUE"); v >= 0) c->work_queue = v;
    if (env_switch("NWE_WORK_QUEUE_BACKFILL") == 0) c->backfill = false;
    if (const int v = env_switch("NWE_WORK_QUEUE_TAIL"); v >= 0) c->tail = v == 1;
    if (const int v = env_switch("NWE_COLOUR_SKIP"); v >= 0) c->colour_skip = v;
    if (const int v = env_switch("NWE_PACKET_BLOCKS"); v >= 0) c->packet_blocks = v == 1;
    if (!c->host_only) {
        const hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { delete c; return fail(nullptr, NWE_ERR_HIP, std::string("nwe_create: ") + hipGetErrorString(e)); }
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->cus = cus;
        else (void)hipGetLastError();
    }
    *out = c;
    return NWE_OK;
}

void nwe_destroy(nwe_ctx* c) {
    if (!c) return;
    if (c->host_only) { delete c; return; }   // holds nothing on a device: no HIP call
    DeviceGuard guard;
    (void)hipSetDevice(c->device);
    // nothing of this context may still be running when its buffers go; then the owners release what they hold
    (void)wait_for_launches(c);
    if (c->tile_stream) (void)hipStreamSynchronize(c->tile_stream);
    delete c;
}

const char* nwe_last_error(const nwe_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int nwe_set_network(nwe_ctx* c, int which, int depth, int width, int in_xyz, int in_dir, int skip_layer,
                    const float* const* w, const float* const* b) {
    CHECK(c, check_network(!c || !w || !b, which, depth, width, in_xyz, in_dir, 0, true, w, b));
    return set_network(c, which, NetShape{depth, width, in_xyz, in_dir, skip_layer, 0}, w, b);
}

int nwe_set_network_no_view_dirs(nwe_ctx* c, int which, int depth, int width, int in_xyz, int skip_layer, int output_ch,
                                 const float* const* w, const float* const* b) {
    CHECK(c, check_network(!c || !w || !b, which, depth, width, in_xyz, 0, output_ch, false, w, b));
    return set_network(c, which, NetShape{depth, width, in_xyz, 0, skip_layer, output_ch}, w, b);
}

int nwe_set_sampling(nwe_ctx* c, const float* t_vals, const float* one_minus_t, int n_samples, const float* u,
                     int n_importance) {
    CHECK(c, check_sampling(!c, t_vals, one_minus_t, n_samples, u, n_importance));
    c->ns = n_samples; c->ni = n_importance;
    if (c->host_only) return NWE_OK;
    ON_DEVICE(c);
    HIPCHK(c, c->d_t.reserve(2 * kMaxSamples + kMaxImportance));
    TRY(wait_for_launches(c));   // later workgroups of a queued launch still read the old tables
    float* d_t = c->d_t.get();
    HIPCHK(c, hipMemcpy(d_t, t_vals, n_samples * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_t + kMaxSamples, one_minus_t, n_samples * sizeof(float), hipMemcpyHostToDevice));
    if (n_importance > 0) HIPCHK(c, hipMemcpy(d_t + 2 * kMaxSamples, u, n_importance * sizeof(float), hipMemcpyHostToDevice));
    return NWE_OK;
}

int nwe_render(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
               float far, int row_begin, int row_end, int precision, const nwe_outputs* out, void* stream) {
    return render_rows(c, Camera{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end}, precision, out, (hipStream_t)stream);
}

int nwe_render_tiled(nwe_ctx* const* ctxs, int n_ctx, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx,
                     float cy, float near, float far, int precision, float* rgb_dev, float* depth_dev, float* acc_dev,
                     uint32_t* flags_dev, void* stream_) {
    if (!ctxs || n_ctx < 1 || !ctxs[0]) return fail(nullptr, NWE_ERR_INVALID, "nwe_render_tiled: no contexts");
    nwe_ctx* c0 = ctxs[0];
    for (int i = 0; i < n_ctx; ++i)
        if (!ctxs[i] || ctxs[i]->host_only) return fail(c0, NWE_ERR_INVALID, "nwe_render_tiled: null or host-only context");
    Camera m{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, 0, H};
    CHECK(c0, check_camera(m, kCameraOfTiled));
    m.row_end = 0;   // from here on the rows of one tile
    hipStream_t stream0 = (hipStream_t)stream_;
    DeviceGuard guard;
    c0->warn.clear();
    // the caller's buffers may still be in use by earlier work on its stream: every tile stream starts behind this point
    HIPCHK(c0, hipSetDevice(c0->device));
    if (!c0->frame_ready) HIPCHK(c0, hipEventCreateWithFlags(&c0->frame_ready.h, hipEventDisableTiming));
    HIPCHK(c0, c0->flag_parts.reserve(n_ctx));
    HIPCHK(c0, hipMemsetAsync(c0->flag_parts.get(), 0, (size_t)n_ctx * sizeof(uint32_t), stream0));
    HIPCHK(c0, hipEventRecord(c0->frame_ready, stream0));
    const int base = H / n_ctx, extra = H % n_ctx;      // dist.shard_rows: the first H % n tiles get one more row
    int rc_all = NWE_OK;
    for (int i = 0; i < n_ctx && rc_all == NWE_OK; ++i) {
        m.row_begin = m.row_end;
        m.row_end += base + (i < extra ? 1 : 0);
        rc_all = queue_tile(ctxs[i], c0, i, m, precision, Frame{rgb_dev, depth_dev, acc_dev});
        if (rc_all != NWE_OK && ctxs[i] != c0) c0->err = "tile " + std::to_string(i) + ": " + ctxs[i]->err;
    }
    // the caller's stream continues when every tile has landed (also on the error path: nothing may still be writing;
    // every tile that queued anything has re-recorded its event, see RecordOnExit)
    (void)hipSetDevice(c0->device);
    for (int i = 0; i < n_ctx; ++i)
        if (ctxs[i]->tile_done) (void)hipStreamWaitEvent(stream0, ctxs[i]->tile_done, 0);
    if (rc_all != NWE_OK) return rc_all;
    if (flags_dev) {
        hipLaunchKernelGGL(or_flags_kernel, dim3(1), dim3(1), 0, stream0, c0->flag_parts.get(), n_ctx, flags_dev);
        HIPCHK(c0, hipGetLastError());
    }
    return NWE_OK;
}

int nwe_create_rays(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
                    float far, int row_begin, int row_end, float* rays_out_dev, void* stream_) {
    CHECK(c, check_on_device(c && !c->host_only));
    const Camera m{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end};
    if (!rays_out_dev) return fail(c, NWE_ERR_INVALID, "bad pose / image / row range");   // no output: the refusal of no poses
    CHECK(c, check_camera(m, kCameraOfCreateRays));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    Slot& slot = c->rays_slot;   // not a slot of the ring: nwe_last_kernel_ms / _launch_parts keep describing the last render
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, c2w, n_poses, stream));
    const RenderArgs a = camera_args(m, slot.poses.get());
    if (a.n_rays == 0) return NWE_OK;
    return record_launch(c, slot, stream, [&]() -> int {
        hipLaunchKernelGGL(create_rays_kernel, dim3((unsigned)((a.n_rays + 255) / 256)), dim3(256), 0, stream, a, rays_out_dev);
        return NWE_OK;
    });
}

int nwe_query_points(nwe_ctx* c, int which, const float* points_dev, int64_t n_points, const float* dirs_dev, int64_t points_per_dir,
                     int precision, const nwe_point_outputs* out, void* stream_) {
    CHECK(c, check_query(MaybeContext(c).p, which, points_dev, n_points, dirs_dev, points_per_dir, precision, out));
    const NetState& net = c->net[which];
    if (n_points == 0) return NWE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    Slot& slot = c->query.next();   // not a slot of the render ring (see nwe_create_rays)
    TRY(prepare_slot(c, slot));
    QueryArgs a = {};
    a.points = points_dev; a.dirs = dirs_dev; a.raw = out->raw; a.sigma = out->sigma; a.flags = out->flags;
    a.n_points = (int)n_points;
    a.points_per_dir = (int)std::min(points_per_dir, n_points);   // one direction for all of them from there on
    a.density_only = out->raw ? 0 : 1;
    TRY(record_launch(c, slot, stream, [&]() -> int { return run_query(c, net, a, precision, stream); }));
    c->query.commit(slot);
    return NWE_OK;
}

float nwe_last_query_ms(nwe_ctx* c) { return elapsed_ms(c, c ? c->query.last() : nullptr, "nwe_last_query_ms"); }

int nwe_debug_set_query_steps(nwe_ctx* c, int steps) { return set_on(steps < 0 || steps > kQueryMaxSteps ? nullptr : c, [&] { c->query_steps = steps; }); }

int nwe_render_rays(nwe_ctx* c, const float* rays_dev, int64_t n_rays, int precision, const nwe_outputs* out, void* stream) {
    HookReset hooks{c};   // every return below, refusals included, consumes the one-shot hooks
    const MaybeContext desc(c);
    CHECK(c, check_ready(desc.p, out, precision, false));
    CHECK(c, check_ray_count(n_rays, true, !rays_dev));
    if (n_rays == 0) return NWE_OK;
    ON_DEVICE(c);
    return render_ray_list(c, desc.d, rays_dev, n_rays, precision, *out, true, (hipStream_t)stream);
}

int nwe_to8b(nwe_ctx* c, const float* rgb_dev, uint8_t* out_dev, int64_t n, void* stream) {
    if (!c || c->host_only || !rgb_dev || !out_dev || n < 0) return fail(c, NWE_ERR_INVALID, "bad argument");
    if (n == 0) return NWE_OK;
    ON_DEVICE(c);
    hipLaunchKernelGGL(to8b_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rgb_dev, out_dev, n);
    HIPCHK(c, hipGetLastError());
    return NWE_OK;
}

float nwe_last_kernel_ms(nwe_ctx* c) { return elapsed_ms(c, c ? last_render(c) : nullptr, "nwe_last_kernel_ms"); }

int nwe_last_launch_parts(nwe_ctx* c, float* ms2, int64_t* rays2) {
    if (!c || !ms2 || !rays2) return NWE_ERR_INVALID;
    ms2[0] = ms2[1] = -1.f; rays2[0] = rays2[1] = 0;
    const RenderSlot* s = last_render(c);
    if (!s) return fail(c, NWE_ERR_STATE, "nothing has been launched");
    ON_DEVICE(c);
    HIPCHK(c, hipEventSynchronize(s->ev1));
    rays2[0] = s->rays_first; rays2[1] = s->rays_total - s->rays_first;
    const hipEvent_t begin = s->has_share ? s->ev_share : s->ev0;   // behind the producer of a shared coarse pass
    if (s->has_mid) {
        HIPCHK(c, kept_time(*s, Slot::kPart0, begin, s->ev_mid, &ms2[0]));
        HIPCHK(c, kept_time(*s, Slot::kPart1, s->ev_mid, s->ev1, &ms2[1]));
        // begin, ev_mid and ev1 lie on the caller's stream in this order, also when the second launch runs on the side stream
        // (ev1 behind the join), so no part is negative; one that is below the timer's step is reported as that step, never as 0
        // (the sum then exceeds nwe_last_kernel_ms by less than that step)
        for (int i = 0; i < 2; ++i) ms2[i] = std::max(ms2[i], kMinPartMs);
    } else {
        HIPCHK(c, kept_time(*s, Slot::kPart0, begin, s->ev1, &ms2[0]));
    }
    return NWE_OK;
}

int nwe_last_coarse_launch(nwe_ctx* c, float* ms, int64_t* rays) {
    if (!c || !ms || !rays) return NWE_ERR_INVALID;
    *ms = -1.f; *rays = 0;
    const RenderSlot* s = last_render(c);
    if (!s) return fail(c, NWE_ERR_STATE, "nothing has been launched");
    if (!s->has_share) return NWE_OK;
    ON_DEVICE(c);
    HIPCHK(c, hipEventSynchronize(s->ev1));
    HIPCHK(c, kept_time(*s, Slot::kCoarse, s->ev0, s->ev_share, ms));
    *rays = s->share_rays;
    return NWE_OK;
}

int nwe_last_ray_evaluations(nwe_ctx* c, int64_t* out2) {
    if (!c || !out2) return NWE_ERR_INVALID;
    out2[0] = out2[1] = 0;
    const RenderSlot* s = last_render(c);
    if (!s) return fail(c, NWE_ERR_STATE, "nothing has been launched");
    ON_DEVICE(c);
    HIPCHK(c, hipEventSynchronize(s->ev1));
    out2[0] = s->evals_run; out2[1] = s->evals_full;
    if (s->term) {
        unsigned long long ran = 0;
        HIPCHK(c, hipMemcpy(&ran, s->evals.get(), sizeof(ran), hipMemcpyDeviceToHost));
        out2[0] = (int64_t)ran;
    }
    return NWE_OK;
}

int64_t nwe_flops_per_eval(const nwe_ctx* c, int which) { const NetState* n = set_net(c, which); return n ? n->flops : 0; }
int64_t nwe_packed_bytes(const nwe_ctx* c, int which) { const NetState* n = set_net(c, which); return n ? (int64_t)n->p.stream.size() : 0; }
int64_t nwe_packed_bias_count(const nwe_ctx* c, int which) { const NetState* n = set_net(c, which); return n ? (int64_t)n->p.bias_tab.size() : 0; }
float nwe_packed_scale(const nwe_ctx* c, int which) { const NetState* n = set_net(c, which); return n ? n->p.w_scale : 0.f; }
int nwe_packed_colour_finite(const nwe_ctx* c, int which) { const NetState* n = set_net(c, which); return n ? (n->p.colour_finite ? 1 : 0) : -1; }

int nwe_packed_copy(const nwe_ctx* c, int which, void* host_dst, int64_t bytes) { const NetState* n = set_net(c, which); return copy_out(n ? &n->p.stream : nullptr, host_dst, bytes); }
int nwe_packed_bias_copy(const nwe_ctx* c, int which, float* host_dst, int64_t count) { const NetState* n = set_net(c, which); return copy_out(n ? &n->p.bias_tab : nullptr, host_dst, count); }

int nwe_debug_set_fine_depths(nwe_ctx* c, const float* z_dev) { return set_on(c, [&] { c->dbg_z_fine = z_dev; }); }
int nwe_debug_set_raw(nwe_ctx* c, const float* raw_coarse_dev, const float* raw_fine_dev) { return set_on(c, [&] { c->dbg_raw_c = raw_coarse_dev; c->dbg_raw_f = raw_fine_dev; }); }
int nwe_debug_set_coarse_weights(nwe_ctx* c, const float* weights_dev) { return set_on(c, [&] { c->dbg_w = weights_dev; }); }
int nwe_debug_set_fold(nwe_ctx* c, int on) { return set_on(c, [&] { c->fold = on ? 1 : 0; }); }
int nwe_debug_set_decomposition(nwe_ctx* c, int mode) { return set_on(mode < -1 || mode > 2 ? nullptr : c, [&] { c->decomposition = mode; }); }
int nwe_debug_set_work_queue(nwe_ctx* c, int mode) { return set_on(mode < -1 || mode > 1 ? nullptr : c, [&] { c->work_queue = mode; }); }
int nwe_debug_get_work_queue(const nwe_ctx* c) { return c ? c->work_queue : -2; }
int nwe_debug_set_colour_skip(nwe_ctx* c, int mode) { return set_on(mode < 0 || mode > 2 ? nullptr : c, [&] { c->colour_skip = mode; }); }
int nwe_debug_get_colour_skip(const nwe_ctx* c) { return c ? c->colour_skip : -1; }
int nwe_debug_set_packet_blocks(nwe_ctx* c, int on) { return set_on(on < 0 || on > 1 ? nullptr : c, [&] { c->packet_blocks = on != 0; }); }
int nwe_debug_last_packet_blocks(const nwe_ctx* c) { return c ? c->last_packet_blocks : -1; }
int nwe_debug_packet_pixels(int64_t first, int64_t n, int W, int32_t* pixels) {
    if (first < 0 || n < 0 || first + n > INT32_MAX || W < 1 || W > (INT32_MAX / kBlockH) || (n > 0 && !pixels)) return NWE_ERR_INVALID;
    for (int64_t i = 0; i < n; ++i) pixels[i] = packet_block_pixel((int)(first + i), W);
    return NWE_OK;
}
int nwe_debug_get_work_queue_backfill(const nwe_ctx* c) { return c ? (c->backfill ? 1 : 0) : -1; }
unsigned nwe_debug_queue_grid(unsigned items) { return queue_grid(items); }
// The plan of a call without the call: check_ready's refusals, the entry point's own, then plan_call at the given CU count.
int nwe_debug_plan(nwe_ctx* c, int n_poses, int H, int W, int row_begin, int row_end, int64_t n_rays, const nwe_outputs* out,
                   unsigned hooks, int precision, int cus, nwe_plan_report* report) {
    const bool pinhole = n_rays < 0;
    const MaybeContext desc(c);
    CHECK(c, check_ready(desc.p, out, precision, pinhole, true));
    if (!report || report->struct_bytes != sizeof(nwe_plan_report))
        return fail(c, NWE_ERR_INVALID, "nwe_plan_report.struct_bytes != sizeof(nwe_plan_report): the caller was built against another version of include/nwe.h");
    if (cus < 1) return fail(c, NWE_ERR_INVALID, "cus must be at least 1");
    *report = {};
    report->struct_bytes = sizeof(nwe_plan_report);
    static const float somewhere = 0.f;   // an armed hook, a pose table: only null / non-null is read
    RenderArgs a = {};
    if (pinhole) {
        const Camera m{&somewhere, n_poses, H, W, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f, row_begin, row_end};
        CHECK(c, check_camera(m));
        a = camera_args(m, &somewhere);
    } else {
        a.rays = &somewhere; a.n_rays = n_rays; a.W = 1; a.rows = 1;
        if (hooks & NWE_PLAN_HOOK_COARSE_WEIGHTS) a.w_in = &somewhere;
        if (hooks & NWE_PLAN_HOOK_OTHER) a.z_fine_in = &somewhere;
    }
    CHECK(c, check_ray_count(a.n_rays, !pinhole));
    a.out = *out;
    context_args(c, a);
    if (a.n_rays <= 0) return NWE_OK;   // the call launches nothing
    const CallPlan p = plan_call(describe_call(desc.d, a, precision), cus);
    c->last_packet_blocks = p.blocks ? 1 : 0;
    report->separate = p.separate; report->share = p.share; report->full = p.full; report->coarse_launch = p.coarse_launch;
    report->may_queue = p.may_queue; report->need_side = p.need_side; report->need_evals = p.need_evals;
    report->coarse_flags = p.coarse_flags; report->share_k = p.share_k;
    report->table_elems = p.table_elems; report->evals_full = p.evals_full; report->evals_run = p.evals_run; report->share_rays = p.share_rays;
    const StagePlan* stages[2] = {&p.coarse, &p.main};
    for (int i = 0; i < 2; ++i) {
        const StagePlan& s = *stages[i];
        nwe_plan_stage& r = i == 0 ? report->coarse : report->main;
        if (!s.active) continue;
        r.active = 1; r.role = s.role; r.n_rays = s.n_rays; r.n_importance = s.n_importance; r.net = s.net;
        if (p.baked && i == 0) {   // the grid producer: one launch that is no MFMA launch group, so it has no variant and no plan
            r.variant = r.plan = -1; r.n_launches = 1;
            continue;
        }
        if (precision == NWE_PREC_F32) continue;   // the fp32 launcher has no plan
        // what launch_render_mfma refuses: no kernel for the stage, or one fused kernel over two networks of different shapes
        const NetState &nc = c->net[0], &nf = c->net[1];
        if (!s.pass.ok || (s.net < 0 && s.n_importance > 0 && (nf.D != nc.D || nf.W != nc.W || nf.skip != nc.skip || nf.form != nc.form)))
            return fail(c, NWE_ERR_UNSUPPORTED, "coarse and fine networks must have the same shape for the MFMA kernel");
        r.variant = s.pass.variant; r.plan = s.pass.plan; r.n_launches = s.pass.n_launches;
        for (int l = 0; l < 2; ++l) {
            const LaunchPlan& q = s.pass.launch[l];
            r.ray_first[l] = q.ray_first; r.rays[l] = q.rays; r.split[l] = q.split; r.items[l] = q.items; r.grid[l] = q.grid;
        }
        r.fork = s.pass.fork; r.tail = s.pass.tail; r.tail_items = s.pass.tail_items;
    }
    return NWE_OK;
}
int nwe_debug_last_queue(nwe_ctx* c, unsigned* items2, unsigned* grid2, unsigned* taken2, int* side_stream) {
    if (!c || !items2 || !grid2 || !taken2) return NWE_ERR_INVALID;
    for (int i = 0; i < 2; ++i) items2[i] = grid2[i] = taken2[i] = 0;
    if (side_stream) *side_stream = 0;
    const RenderSlot* s = last_render(c);
    if (!s) return fail(c, NWE_ERR_STATE, "nothing has been launched");
    ON_DEVICE(c);
    HIPCHK(c, hipEventSynchronize(s->ev1));
    unsigned taken[2] = {0, 0};
    if (s->q_grid[0] || s->q_grid[1]) HIPCHK(c, hipMemcpy(taken, s->queue.get(), sizeof(taken), hipMemcpyDeviceToHost));
    for (int i = 0; i < 2; ++i) { items2[i] = s->q_items[i]; grid2[i] = s->q_grid[i]; taken2[i] = s->q_grid[i] ? taken[i] : 0; }
    if (side_stream) *side_stream = s->side_used ? 1 : 0;
    return NWE_OK;
}
int nwe_debug_get_work_queue_tail(const nwe_ctx* c) { return c ? (c->tail ? 1 : 0) : -1; }
// which = 0: the split items the first launch rendered; 1: the ones the second launch rendered
static int last_tail(nwe_ctx* c, unsigned* out, int which) {
    if (!c || !out) return NWE_ERR_INVALID;
    *out = 0;
    const RenderSlot* s = last_render(c);
    if (!s) return fail(c, NWE_ERR_STATE, "nothing has been launched");
    if (!s->tail_items) return NWE_OK;
    ON_DEVICE(c);
    HIPCHK(c, hipEventSynchronize(s->ev1));
    unsigned word = 0;   // every surplus workgroup of the first launch took a number: the items it rendered are the numbers below tail_items
    HIPCHK(c, hipMemcpy(&word, s->queue.get() + 2 + which, sizeof(word), hipMemcpyDeviceToHost));
    *out = which == 0 ? std::min(word, s->tail_items) : word;
    return NWE_OK;
}
int nwe_debug_last_tail(nwe_ctx* c, unsigned* stolen) { return last_tail(c, stolen, 0); }
int nwe_debug_last_tail_rest(nwe_ctx* c, unsigned* rendered) { return last_tail(c, rendered, 1); }
int nwe_debug_set_stamps(nwe_ctx* c, unsigned long long* per_wave_dev) { return set_on(c, [&] { c->stamps = per_wave_dev; }); }
int nwe_set_white_background(nwe_ctx* c, int on) { return set_on(c, [&] { c->white_bkgd = on ? 1 : 0; }); }
int nwe_set_early_termination(nwe_ctx* c, float min_transmittance) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_early_termination(min_transmittance));
    c->min_trans = min_transmittance > 0.f ? min_transmittance : 0.f;
    return NWE_OK;
}
float nwe_get_early_termination(const nwe_ctx* c) { return c ? c->min_trans : -1.f; }
int nwe_set_shared_coarse(nwe_ctx* c, int k) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_shared_coarse(k));
    c->share_k = k;
    return NWE_OK;
}
int nwe_get_shared_coarse(const nwe_ctx* c) { return c ? c->share_k : -1; }
int nwe_set_separate_passes(nwe_ctx* c, int on) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_separate_passes(on));
    c->separate = on;
    return NWE_OK;
}
int nwe_get_separate_passes(const nwe_ctx* c) { return c ? c->separate : -1; }

int nwe_set_train_tables(nwe_ctx* c, const float* t_rand_dev, const float* noise_coarse_dev, const float* noise_fine_dev, const float* u_sorted_dev) {
    return set_on(c, [&] { c->trn_t = t_rand_dev; c->trn_nc = noise_coarse_dev; c->trn_nf = noise_fine_dev; c->trn_u = u_sorted_dev; });
}

int nwe_debug_last_plan(const nwe_ctx* c) { return c ? c->last_plan : -1; }
const char* nwe_last_warning(const nwe_ctx* c) { return c ? c->warn.c_str() : ""; }

int nwe_debug_peer_access(const nwe_ctx* first, const nwe_ctx* tile) {
    if (!first || !tile || first->host_only || tile->host_only) return -1;
    if (tile->peer_access != -2) return tile->peer_access;
    return tile->device == first->device ? 1 : can_access_peer(tile->device, first->device);
}

int nwe_selftest(nwe_ctx* c, int32_t* report8) {
    if (!c || c->host_only || !report8) return fail(c, NWE_ERR_INVALID, "bad argument");
    ON_DEVICE(c);
    const int rc = run_selftest(report8, nullptr);
    if (rc == -1) return fail(c, NWE_ERR_HIP, "selftest: HIP failure");
    if (rc != 0) return fail(c, NWE_ERR_STATE, "selftest: a hardware layout assumption does not hold (see report)");
    return NWE_OK;
}

}  // extern "C"
