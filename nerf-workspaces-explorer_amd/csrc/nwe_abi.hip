// C ABI of libnwe_hip.so (include/nwe.h): context, device resources, table upload, kernel launches.  Weight packing: nwe_pack.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nwe_check.h"
#include "nwe_host.h"
#include "nwe_pack.h"

using namespace nwe;

namespace {

// Move-only owners of what the context holds on its device.  One that holds nothing calls nothing, so a host-only context
// makes no HIP call in creation, use or destruction; what they hold is released with the context (nwe_destroy).
template <class H, hipError_t (*Release)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    ~Owned() { reset(); }
    void reset() { if (h) (void)Release(h); h = nullptr; }
    operator H() const { return h; }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

template <class T>
struct DevBuf {
    Owned<void*, hipFree> mem;
    size_t cap = 0;   // elements
    T* get() const { return static_cast<T*>(mem.h); }
    // Grow-only; growing drops the old contents, so the caller has made sure that nothing queued still reads them.
    hipError_t reserve(size_t count) {
        if (count <= cap) return hipSuccess;
        mem.reset(); cap = 0;
        const hipError_t e = hipMalloc(&mem.h, count * sizeof(T));
        if (e == hipSuccess) cap = count; else mem.h = nullptr;
        return e;
    }
};

struct NetState : NetDesc {       // shape, set, form, mfma_ok, built: what the checks and the planner read (nwe_check.h)
    int64_t flops = 0;
    Packed p;                      // host side: blob + offsets, stream, bias table, scale (nwe_pack.h)
    NetF32 f32 = {};               // fp32 kernel: p.f32 with the blob on the device
    NetMfma mf = {};
    DevBuf<float> d_blob, d_bias;  // device side: copies of p.blob, p.bias_tab
    DevBuf<uint8_t> d_stream;      //              and of p.stream
};

// One slot per launch in flight: the pose table a kernel reads and the events around it.  A slot is reused only
// after its own launch has finished (its `done` event), so launches of one context queued on different streams never
// share a pose buffer.  This much every launch has: nwe_create_rays and the query ring take it as it is.
struct Slot {
    DevBuf<float> poses;
    Event ev0, ev1;
    bool used = false;
    // A time of the launch is read from its pair of events ONCE and kept (kept_time): the runtime converts the device's ticks anew
    // at every hipEventElapsedTime, and two readings of one launch were seen to differ in the last digit - a report must not
    // change while it describes the same launch.  kWhole: ev0 .. ev1; the others are the render ring's (nwe_last_launch_parts,
    // nwe_last_coarse_launch).  Forgotten when the slot is prepared for a new launch.
    enum { kWhole, kPart0, kPart1, kCoarse, kTimes };
    mutable float time_ms[kTimes] = {};
    mutable bool time_read[kTimes] = {};
};

// A slot of the sparse ring.  An asynchronous call (nwe_render_sparse_async) leaves its selected samples in `tally` on the device -
// one add per chunk - and, behind its last chunk, in the pinned `word`, which nwe_last_sparse_samples reads once ev1 has passed.
struct SparseSlot : Slot {
    DevBuf<unsigned long long> tally;
    Owned<void*, hipHostFree> word;
};

// A slot of the render ring: what its launch reports and the device resources its plan asks for (CallPlan, nwe_plan.h).
struct RenderSlot : Slot {
    Event ev_mid;   // between the two launches of the hybrid plan
    bool has_mid = false;
    int64_t rays_first = 0, rays_total = 0;
    // nwe_last_ray_evaluations: the full count of the launch and, if it terminated rays early, the word its waves added to
    DevBuf<unsigned long long> evals;
    bool term = false;
    int64_t evals_full = 0;
    // shared coarse pass (nwe_set_shared_coarse): the launch's own weight table [n_samples][n_rep], which the producer launch
    // fills and the consumer launch behind it reads (last reader: prepare_slot), the event between the two
    // (nwe_last_coarse_launch), the representatives and the evaluations the two launches ran
    // separate passes (nwe_set_separate_passes): the same table between the coarse and the fine launch, [n_rays][n_samples] when
    // the two are full kernels, and the word the coarse launch's flags go through (or_masked_flags_kernel)
    DevBuf<float> share_w;
    DevBuf<uint32_t> coarse_flags;
    Event ev_share;
    bool has_share = false;
    int64_t share_rays = 0, evals_run = 0;
    // work queue (nwe_debug_set_work_queue): the ticket counters of the call (LaunchResources::counters), zeroed on the
    // caller's stream in front of the launches (last reader: prepare_slot); the low-priority stream the second launch of the
    // hybrid plan backfills the first from, and the events of its fork and join; what nwe_debug_last_queue reports
    DevBuf<unsigned> queue;
    Stream side;
    Event ev_fork, ev_join;
    unsigned q_items[2] = {0, 0}, q_grid[2] = {0, 0};
    bool side_used = false;
    // the tail path (nwe_debug_last_tail): the split items of a launch that took it, whose third counter lies behind the two
    unsigned tail_items = 0;
};

// The box of either grid of a context, as its checks let it through (check_grid_box).
struct GridBox {
    float lo[3] = {}, hi[3] = {}, inv[3] = {};
    int res[3] = {};
    int64_t cells = 0;
    GridBox() = default;
    GridBox(const float* lo_, const float* hi_, const int* res_) : cells((int64_t)res_[0] * res_[1] * res_[2]) {
        for (int i = 0; i < 3; ++i) {
            lo[i] = lo_[i]; hi[i] = hi_[i]; res[i] = res_[i];
            inv[i] = (float)res[i] / (hi[i] - lo[i]);   // fp32, once: what the kernels multiply by (nwe_get_occupancy / _coarse_grid report it)
        }
    }
    // nwe_get_occupancy, nwe_get_coarse_grid, nwe_get_radiance_grid: every pointer may be null
    void read(float* lo_, float* hi_, int* res_, float* inv_) const {
        for (int i = 0; i < 3; ++i) {
            if (lo_) lo_[i] = lo[i];
            if (hi_) hi_[i] = hi[i];
            if (res_) res_[i] = res[i];
            if (inv_) inv_[i] = inv[i];
        }
    }
};

// The occupancy grid of a context (nwe_set_occupancy, nwe_build_occupancy).  The words on the host are the truth of
// nwe_get_occupancy / nwe_occupancy_copy and all there is on a host-only context; a device context also holds them, and the
// descriptor the occupancy kernels read, in buffers of its own.
struct Occupancy {
    bool set = false;
    GridBox box;
    int64_t occupied = 0;
    std::vector<uint32_t> bits;
};

// The coarse density grid of a context (nwe_set_coarse_grid, nwe_bake_coarse_grid).  A device context keeps the values on its
// device only (d_cgrid: up to 512^3 floats), a host-only context in `host`.
struct CoarseGridState {
    bool set = false;
    GridBox box;
    std::vector<float> host;
};

// The radiance grid of a context (nwe_set_radiance_grid, nwe_bake_radiance_grid): four values per cell, kept like the coarse
// grid's - on a device context in d_rgrid only (up to 512^3 rows, 2 GiB), on a host-only context in `host`.
using RadianceGridState = CoarseGridState;

thread_local std::string g_create_error;

}  // namespace

struct nwe_ctx {
    int device = -1;
    bool host_only = false;
    int cus = 256;            // the device's compute units, asked once by nwe_create: what the launch plans and the query's steps count rounds in
    NetState net[2];
    DevBuf<float> d_t;        // t_vals | one_minus_t | u, at 0, kMaxSamples and 2 kMaxSamples
    int ns = 0, ni = 0;
    static constexpr int kSlots = 4;
    RenderSlot slots[kSlots];
    Slot rays_slot;                      // nwe_create_rays: a pose table and events of its own, outside the timing ring
    // next_slot: the slot the next render takes.  last_slot: the most recent render launch that was RECORDED
    // (nwe_last_kernel_ms); both move only when launch() has succeeded, so a refused launch leaves the timing calls alone.
    int next_slot = 0, last_slot = -1;
    // nwe_query_points: a ring of its own, outside the render ring like rays_slot, so that a query moves none of the render
    // launches' reports; last_query: the most recent query launch that was recorded (nwe_last_query_ms)
    Slot query_slots[kSlots];
    int next_query = 0, last_query = -1;
    int query_steps = 0;      // nwe_debug_set_query_steps: 0 = automatic
    // nwe_render_grid: a ring of its own as well, so that a grid frame moves none of the render launches' or the query's reports;
    // last_grid: the most recent grid launch that was recorded (nwe_last_grid_ms)
    Slot grid_slots[kSlots];
    int next_grid = 0, last_grid = -1;
    // nwe_render_sparse: one more ring of its own; last_sparse: the most recent sparse call that ran (nwe_last_sparse_ms), what it
    // selected of how many samples (nwe_last_sparse_samples); the chunks' scratch, grow-only, the device word the scan leaves a
    // chunk's total in (behind the scratch's tables) and the pinned word it is read back through
    // nwe_render_sparse_async shares the ring, the scratch and the reports: sparse_async says which kind the last call was (its
    // selected samples are then in the slot's pinned word), sparse_host_waits how often it made the host wait
    // (nwe_debug_last_sparse_host_waits)
    SparseSlot sparse_slots[kSlots];
    int next_sparse = 0, last_sparse = -1;
    int64_t sparse_selected = 0, sparse_total = 0;
    bool sparse_async = false;
    int sparse_host_waits = -1;
    int sparse_chunk = 0;     // nwe_debug_set_sparse_chunk: 0 = the default
    DevBuf<uint8_t> d_sparse_scratch;
    Owned<void*, hipHostFree> sparse_word;
    const float* dbg_z_fine = nullptr;
    const float *dbg_raw_c = nullptr, *dbg_raw_f = nullptr, *dbg_w = nullptr;   // nwe_debug_set_raw / _coarse_weights, one call
    int fold = 1;             // nwe_debug_set_fold: read by nwe_set_network
    // nwe_render_tiled: this context's row tile (rgb | depth | acc slabs + its flag word), its own stream, and the event
    // that says "tile rendered and copied into the frame"
    DevBuf<float> tile_buf;
    DevBuf<uint32_t> tile_flags;
    Stream tile_stream;
    Event tile_done;
    Event frame_ready;                  // contexts[0] only: recorded on the caller's stream when the call starts
    DevBuf<uint32_t> flag_parts;        // contexts[0] only: one flag word per tile, on its device
    int peer_access = -2;               // this context's device -> contexts[0]'s device: 1 direct, 0 staged, -1 query/enable failed, -2 not asked yet
    std::string warn;                   // nwe_last_warning: what did not fail the call but the caller should know
    int white_bkgd = 0;
    float min_trans = 0.f;    // nwe_set_early_termination: 0 = off
    int share_k = 1;          // nwe_set_shared_coarse: 1 = off
    int separate = 0;         // nwe_set_separate_passes: 0 = off
    Occupancy occ;            // nwe_set_occupancy / nwe_build_occupancy: occ.set = a grid is set
    DevBuf<uint32_t> d_occ_bits, d_occ_tmp;   // the grid's words on the device; nwe_build_occupancy's second buffer for the dilation
    DevBuf<OccGrid> d_occ;                    // the descriptor RenderArgs::occ points to
    DevBuf<float> d_occ_scratch;              // nwe_build_occupancy: probe points and their sigma, one chunk
    CoarseGridState cgrid;    // nwe_set_coarse_grid / nwe_bake_coarse_grid: cgrid.set = a grid is set
    DevBuf<float> d_cgrid;                    // its values on the device; nwe_bake_coarse_grid's cell centres go through d_occ_scratch
    RadianceGridState rgrid;  // nwe_set_radiance_grid / nwe_bake_radiance_grid: rgrid.set = a grid is set
    DevBuf<float> d_rgrid;                    // its rows on the device; nwe_bake_radiance_grid's cell centres go through d_occ_scratch
    int decomposition = -1;   // nwe_debug_set_decomposition
    int work_queue = -1;      // nwe_debug_set_work_queue; a new context takes NWE_WORK_QUEUE=0|1 from the environment
    bool backfill = true;     // the hybrid plan's second launch on the slot's own stream; NWE_WORK_QUEUE_BACKFILL=0: behind the first
    bool tail = true;         // the hybrid plan's split items in the packets launch's tail; NWE_WORK_QUEUE_TAIL=0: as without it
    int colour_skip = 1;      // nwe_debug_set_colour_skip; NWE_COLOUR_SKIP=0: a new context starts with 0
    int last_plan = -1;       // nwe_debug_last_plan
    bool packet_blocks = true;       // nwe_debug_set_packet_blocks; NWE_PACKET_BLOCKS=0: a new context starts without
    int last_packet_blocks = 0;      // nwe_debug_last_packet_blocks: the last call planned (rendered, or nwe_debug_plan) was blocked
    unsigned long long* stamps = nullptr;   // nwe_debug_set_stamps
    const float *trn_t = nullptr, *trn_nc = nullptr, *trn_nf = nullptr, *trn_u = nullptr;   // nwe_set_train_tables, one call
    std::string err;
};

namespace {

int fail(nwe_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// Every entry point that switches the calling thread's HIP device puts it back on return: a GUI or bench thread that
// queries a tile of another device must not find its later torch calls on that device.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#define HIPCHK(ctx, expr)                                                                                       \
    do {                                                                                                        \
        const hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail(ctx, NWE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define ON_DEVICE(c) DeviceGuard guard; HIPCHK(c, hipSetDevice(c->device))   // the rest of the entry point runs on c's device
#define TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)
// A check of nwe_check.h: its refusal, if any, becomes the context's error and the entry point's return value.
#define CHECK(c, check) do { const Refusal r_ = (check); if (r_) return fail(c, r_.code, r_.text); } while (0)

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
// ... of a context that may be null: what the checks that refuse a null context take
struct MaybeContext {
    ContextDesc d;
    const ContextDesc* p = nullptr;
    explicit MaybeContext(const nwe_ctx* c) { if (c) { d = describe_context(c); p = &d; } }
};

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

// ev0, what `queue` launches, ev1: from then on the slot describes this launch.  `queue` returns NWE_OK or refuses (then
// nothing was launched and the slot stays unused).
template <class Queue>
int record_launch(nwe_ctx* c, Slot& s, hipStream_t stream, Queue&& queue) {
    HIPCHK(c, hipEventRecord(s.ev0, stream));
    TRY(queue());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(s.ev1, stream));
    s.used = true;
    return NWE_OK;
}

// The sparse calls in flight, on whatever streams they are: a synchronous one has been waited for unless it failed half way, an
// asynchronous one ends in its slot's ev1.  *waits counts the slots that had not finished yet.
int wait_for_sparse(nwe_ctx* c, int* waits) {
    for (SparseSlot& s : c->sparse_slots) {
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
    for (RenderSlot& s : c->slots)
        if (s.used) HIPCHK(c, hipEventSynchronize(s.ev1));
    if (c->rays_slot.used) HIPCHK(c, hipEventSynchronize(c->rays_slot.ev1));
    for (Slot& s : c->query_slots)   // a query streams the weights of its network throughout
        if (s.used) HIPCHK(c, hipEventSynchronize(s.ev1));
    for (Slot& s : c->grid_slots)    // a grid frame reads the sampling tables and the radiance grid
        if (s.used) HIPCHK(c, hipEventSynchronize(s.ev1));
    return wait_for_sparse(c, nullptr);   // a sparse frame reads all of it
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

#ifdef NWE_STAMPS
constexpr bool kStampedBuild = true;
#else
constexpr bool kStampedBuild = false;
#endif

// What the context holds for every render call: background, sampling tables and counts, the modes' kernel arguments.
void context_args(const nwe_ctx* ctx, RenderArgs& a) {
    a.white_bkgd = ctx->white_bkgd;
    a.t_vals = ctx->d_t.get();   // null on a host-only context, which plans and never launches
    if (a.t_vals) { a.omt_vals = a.t_vals + kMaxSamples; a.u_vals = a.omt_vals + kMaxSamples; }
    a.n_samples = ctx->ns; a.n_importance = ctx->ni;
    a.stamps = ctx->stamps;   // only read by -DNWE_STAMPS builds of the kernel (nwe_debug_set_stamps)
    a.min_trans = ctx->min_trans;
}

// The call as the planner sees it (nwe_plan.h): `a` as the entry point and context_args() filled it, the context's modes.
CallDesc describe_call(const ContextDesc& ctx, const RenderArgs& a, int precision) {
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
    for (RenderSlot& s : ctx->slots) {
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

// The context's coarse density grid as the producer kernel takes it.
CoarseGrid coarse_grid_args(const nwe_ctx* ctx) {
    CoarseGrid g = {};
    const GridBox& box = ctx->cgrid.box;
    for (int i = 0; i < 3; ++i) { g.lo[i] = box.lo[i]; g.inv[i] = box.inv[i]; g.res[i] = box.res[i]; }
    g.sigma = ctx->d_cgrid.get();
    return g;
}

// A render launch on the ring slot prepare_slot() made ready (ctx->slots[ctx->next_slot]): describe the call, plan it, carry
// the plan out.  The ring moves on here, once the launch has been recorded.
int launch(nwe_ctx* ctx, const ContextDesc& desc, RenderSlot& slot, RenderArgs& a, int precision, hipStream_t stream) {
    context_args(ctx, a);
    if (a.n_rays <= 0) return NWE_OK;
    const CallPlan p = plan_call(describe_call(desc, a, precision), ctx->cus);
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
        if (mfma) ctx->last_plan = pass.plan;
        slot.side_used = report.side_used; slot.has_mid = report.mid_recorded;
        return NWE_OK;
    });
    if (rc) return rc;
    ctx->last_slot = (int)(&slot - ctx->slots);
    ctx->next_slot = (ctx->last_slot + 1) % nwe_ctx::kSlots;
    return NWE_OK;
}

// nwe_render, and one tile of nwe_render_tiled.  Refuses in this order: check_ready, camera, device.
int render_rows(nwe_ctx* c, const Camera& m, int precision, const nwe_outputs* out, hipStream_t stream) {
    const MaybeContext desc(c);
    CHECK(c, check_ready(desc.p, out, precision, true));
    CHECK(c, check_camera(m));
    ON_DEVICE(c);
    RenderSlot& slot = c->slots[c->next_slot];
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, m.c2w, m.n_poses, stream));
    RenderArgs a = camera_args(m, slot.poses.get());
    CHECK(c, check_ray_count(a.n_rays, false));
    a.out = *out;
    return launch(c, desc.d, slot, a, precision, stream);
}

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

template <class T>
int copy_out(const std::vector<T>* v, void* host_dst, int64_t count) {
    if (!v || !host_dst || count != (int64_t)v->size()) return NWE_ERR_INVALID;
    std::memcpy(host_dst, v->data(), (size_t)count * sizeof(T));
    return NWE_OK;
}

// The setters' guard: they refuse a null context and say nothing else (no error text).
template <class Set>
int set_on(nwe_ctx* c, Set&& set) { if (!c) return NWE_ERR_INVALID; set(); return NWE_OK; }

// The least nwe_last_launch_parts reports for a part, in ms: the 10 ns step of the event timer
constexpr float kMinPartMs = 1e-5f;

// The most recent recorded render launch (nwe_last_kernel_ms, nwe_last_launch_parts), or null
const RenderSlot* last_render(const nwe_ctx* c) { return c->host_only || c->last_slot < 0 || !c->slots[c->last_slot].used ? nullptr : &c->slots[c->last_slot]; }

// ---- occupancy grid (nwe_set_occupancy, nwe_build_occupancy) ----

int64_t occ_words(int64_t cells) { return (cells + 31) / 32; }

// Makes `words` (host, occ_words(cells) of them) the context's grid.  The bits behind the last cell are cleared; on a device
// context the words and the descriptor go to the context's own buffers, which no launch reads any more (the caller has waited).
int install_occupancy(nwe_ctx* c, const GridBox& box, std::vector<uint32_t>&& words) {
    Occupancy g;
    g.box = box;
    if (box.cells & 31) words.back() &= (1u << (box.cells & 31)) - 1u;
    for (const uint32_t w : words) g.occupied += __builtin_popcount(w);
    g.bits = std::move(words);
    if (!c->host_only) {
        c->occ.set = false;   // a failing upload leaves no grid rather than the old one's descriptor over new words
        HIPCHK(c, c->d_occ_bits.reserve(g.bits.size()));
        HIPCHK(c, c->d_occ.reserve(1));
        HIPCHK(c, hipMemcpy(c->d_occ_bits.get(), g.bits.data(), g.bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        OccGrid d = {};
        for (int i = 0; i < 3; ++i) { d.lo[i] = box.lo[i]; d.inv[i] = box.inv[i]; d.res[i] = box.res[i]; }
        d.bits = c->d_occ_bits.get();
        HIPCHK(c, hipMemcpy(c->d_occ.get(), &d, sizeof(d), hipMemcpyHostToDevice));
    }
    g.set = true;
    c->occ = std::move(g);
    return NWE_OK;
}

// ---- coarse density grid (nwe_set_coarse_grid, nwe_bake_coarse_grid) ----

// The box, the resolution and inv of a new grid of values - the coarse density grid or the radiance grid; the values are in place
// (the grid's device buffer or g.host) when this is called.
void install_grid(CoarseGridState& slot, const GridBox& box, std::vector<float>&& host) {
    CoarseGridState g;
    g.box = box;
    g.host = std::move(host);
    g.set = true;
    slot = std::move(g);
}
void install_coarse_grid(nwe_ctx* c, const GridBox& box, std::vector<float>&& host) { install_grid(c->cgrid, box, std::move(host)); }

// nwe_set_* of a grid of values, `per_cell` floats a cell, behind its checks: the one path of both such grids.
int set_values_grid(nwe_ctx* c, CoarseGridState& slot, DevBuf<float>& dev, const GridBox& box, int per_cell, const float* values, bool on_device) {
    const size_t count = (size_t)box.cells * per_cell;
    if (c->host_only) {
        install_grid(slot, box, std::vector<float>(values, values + count));
        return NWE_OK;
    }
    ON_DEVICE(c);
    TRY(wait_for_launches(c));   // a queued launch still reads the old grid
    slot = CoarseGridState{};    // a failing allocation or upload leaves no grid rather than the old box over new values
    HIPCHK(c, dev.reserve(count));
    HIPCHK(c, hipMemcpy(dev.get(), values, count * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    install_grid(slot, box, {});
    return NWE_OK;
}
int clear_values_grid(nwe_ctx* c, CoarseGridState& slot) {
    if (!c->host_only && slot.set) {
        ON_DEVICE(c);
        TRY(wait_for_launches(c));
    }
    slot = CoarseGridState{};
    return NWE_OK;
}
int copy_values_grid(nwe_ctx* c, const CoarseGridState& slot, const DevBuf<float>& dev, float* host_values, int64_t n_values) {
    if (c->host_only) return copy_out(&slot.host, host_values, n_values);
    ON_DEVICE(c);
    HIPCHK(c, hipMemcpy(host_values, dev.get(), (size_t)n_values * sizeof(float), hipMemcpyDeviceToHost));
    return NWE_OK;
}

// The context's radiance grid as its kernel takes it.
RadianceGrid radiance_grid_args(const nwe_ctx* ctx) {
    RadianceGrid g = {};
    const GridBox& box = ctx->rgrid.box;
    for (int i = 0; i < 3; ++i) { g.lo[i] = box.lo[i]; g.inv[i] = box.inv[i]; g.res[i] = box.res[i]; }
    g.rows = reinterpret_cast<const float4*>(ctx->d_rgrid.get());
    return g;
}

// ---- the probe lattice of a box: what nwe_build_occupancy asks the networks at, and - probes = 1, the cells' centres - what
// nwe_bake_coarse_grid does ----

struct Lattice {
    OccBuild b;
    int per_cell;       // probes^3
    int chunk_cells;    // the cells whose probes go through the scratch buffer at a time: 2^20 points at the most
};

Lattice probe_lattice(const GridBox& box, int probes) {
    Lattice l = {};
    for (int i = 0; i < 3; ++i) {
        l.b.lo[i] = box.lo[i]; l.b.res[i] = box.res[i];
        l.b.step[i] = (float)(((double)box.hi[i] - (double)box.lo[i]) / (double)box.res[i]);
    }
    l.b.probes = probes;
    l.per_cell = probes * probes * probes;
    l.chunk_cells = (int)std::min<int64_t>(box.cells, std::max(1, (1 << 20) / l.per_cell));
    return l;
}

// Chunk by chunk on `stream`: the probe points of the chunk's cells into `points`, network n's sigma at them - the sigma-only
// query of nwe_query_points: no directions, the density trunk alone where it is built - to where sigma_of(first cell) says, then
// done(sigma, first cell, cells), which queues what the caller makes of them.
template <class SigmaOf, class Done>
int query_lattice(nwe_ctx* c, const NetState& n, const Lattice& l, int64_t cells, float* points, int precision, hipStream_t stream,
                  SigmaOf&& sigma_of, Done&& done) {
    for (int64_t first = 0; first < cells; first += l.chunk_cells) {
        const int count = (int)std::min<int64_t>(l.chunk_cells, cells - first);
        launch_occ_probe_points(l.b, first, count, points, stream);
        QueryArgs q = {};
        q.points = points; q.sigma = sigma_of(first); q.n_points = count * l.per_cell; q.points_per_dir = 1; q.density_only = 1;
        if (precision == NWE_PREC_F32) launch_query_f32(q, n.f32, c->query_steps, c->cus, stream);
        else if (!launch_query_mfma(q, n.mf, precision == NWE_PREC_F16X3, c->query_steps, c->cus, stream))
            return fail(c, NWE_ERR_UNSUPPORTED, "no MFMA query kernel in this build for this network shape; use NWE_PREC_F32");
        done(q.sigma, first, count);
    }
    return NWE_OK;
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

// nwe_last_kernel_ms, nwe_last_query_ms: the time between the events of a recorded launch, or -1 and the context's error
float elapsed_ms(nwe_ctx* c, const Slot& s, const char* who) {
    DeviceGuard guard;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipEventSynchronize(s.ev1);
    float ms = -1.f;
    if (e == hipSuccess) e = kept_time(s, Slot::kWhole, s.ev0, s.ev1, &ms);
    if (e != hipSuccess) { c->err = std::string(who) + ": " + hipGetErrorString(e); (void)hipGetLastError(); return -1.f; }
    return ms;
}

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
    Slot& slot = c->query_slots[c->next_query];   // not a slot of the render ring (see nwe_create_rays)
    TRY(prepare_slot(c, slot));
    QueryArgs a = {};
    a.points = points_dev; a.dirs = dirs_dev; a.raw = out->raw; a.sigma = out->sigma; a.flags = out->flags;
    a.n_points = (int)n_points;
    a.points_per_dir = (int)std::min(points_per_dir, n_points);   // one direction for all of them from there on
    a.density_only = out->raw ? 0 : 1;
    TRY(record_launch(c, slot, stream, [&]() -> int {
        if (precision == NWE_PREC_F32) launch_query_f32(a, net.f32, c->query_steps, c->cus, stream);
        else if (!launch_query_mfma(a, net.mf, precision == NWE_PREC_F16X3, c->query_steps, c->cus, stream))
            return fail(c, NWE_ERR_UNSUPPORTED, "no MFMA query kernel in this build for this network shape; use NWE_PREC_F32");
        return NWE_OK;
    }));
    c->last_query = (int)(&slot - c->query_slots);
    c->next_query = (c->last_query + 1) % nwe_ctx::kSlots;
    return NWE_OK;
}

float nwe_last_query_ms(nwe_ctx* c) {
    if (!c || c->host_only || c->last_query < 0 || !c->query_slots[c->last_query].used) return -1.f;
    return elapsed_ms(c, c->query_slots[c->last_query], "nwe_last_query_ms");
}

int nwe_debug_set_query_steps(nwe_ctx* c, int steps) { return set_on(steps < 0 || steps > kQueryMaxSteps ? nullptr : c, [&] { c->query_steps = steps; }); }

int nwe_render_rays(nwe_ctx* c, const float* rays_dev, int64_t n_rays, int precision, const nwe_outputs* out, void* stream) {
    HookReset hooks{c};   // every return below, refusals included, consumes the one-shot hooks
    const MaybeContext desc(c);
    CHECK(c, check_ready(desc.p, out, precision, false));
    CHECK(c, check_ray_count(n_rays, true, !rays_dev));
    if (n_rays == 0) return NWE_OK;
    ON_DEVICE(c);
    RenderSlot& slot = c->slots[c->next_slot];
    TRY(prepare_slot(c, slot));
    RenderArgs a = {};
    a.rays = rays_dev; a.n_rays = n_rays; a.W = 1; a.rows = 1;
    a.ray_cols = c->net[0].in_dir == 0 ? 8 : 11;                       // rays.py:22-30: no view-direction columns without view dirs
    a.z_fine_in = c->dbg_z_fine; a.raw_in_c = c->dbg_raw_c; a.raw_in_f = c->dbg_raw_f; a.w_in = c->dbg_w;
    a.t_rand = c->trn_t; a.noise_c = c->trn_nc; a.noise_f = c->trn_nf; a.u_rand = c->trn_u;
    a.out = *out;
    return launch(c, desc.d, slot, a, precision, (hipStream_t)stream);
}

int nwe_to8b(nwe_ctx* c, const float* rgb_dev, uint8_t* out_dev, int64_t n, void* stream) {
    if (!c || c->host_only || !rgb_dev || !out_dev || n < 0) return fail(c, NWE_ERR_INVALID, "bad argument");
    if (n == 0) return NWE_OK;
    ON_DEVICE(c);
    hipLaunchKernelGGL(to8b_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rgb_dev, out_dev, n);
    HIPCHK(c, hipGetLastError());
    return NWE_OK;
}

float nwe_last_kernel_ms(nwe_ctx* c) {
    const RenderSlot* s = c ? last_render(c) : nullptr;
    return s ? elapsed_ms(c, *s, "nwe_last_kernel_ms") : -1.f;
}

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
int nwe_set_occupancy(nwe_ctx* c, const float* lo, const float* hi, const int* res, const uint32_t* bits, int bits_on_device) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_set_grid(kOccupancyGrid, lo, hi, res, bits, bits_on_device != 0, c->host_only));
    const GridBox box(lo, hi, res);
    std::vector<uint32_t> words((size_t)occ_words(box.cells));
    if (c->host_only) {
        std::memcpy(words.data(), bits, words.size() * sizeof(uint32_t));
        return install_occupancy(c, box, std::move(words));
    }
    ON_DEVICE(c);
    TRY(wait_for_launches(c));   // a queued launch still reads the old grid
    if (bits_on_device) HIPCHK(c, hipMemcpy(words.data(), bits, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    else std::memcpy(words.data(), bits, words.size() * sizeof(uint32_t));
    return install_occupancy(c, box, std::move(words));
}

int nwe_clear_occupancy(nwe_ctx* c) {
    if (!c) return NWE_ERR_INVALID;
    if (!c->host_only && c->occ.set) {
        ON_DEVICE(c);
        TRY(wait_for_launches(c));
    }
    c->occ = Occupancy{};
    return NWE_OK;
}

int nwe_get_occupancy(const nwe_ctx* c, float* lo, float* hi, int* res, float* inv, int64_t* occupied_cells) {
    if (!c) return NWE_ERR_INVALID;
    if (!c->occ.set) return NWE_ERR_STATE;   // no grid is set: the outputs stay untouched (and so does the error text of a const context)
    c->occ.box.read(lo, hi, res, inv);
    if (occupied_cells) *occupied_cells = c->occ.occupied;
    return NWE_OK;
}

int nwe_occupancy_copy(const nwe_ctx* c, uint32_t* host_words, int64_t n_words) {
    if (!c) return NWE_ERR_INVALID;
    if (!c->occ.set) return NWE_ERR_STATE;
    return copy_out(&c->occ.bits, host_words, n_words);
}

int nwe_build_occupancy(nwe_ctx* c, const float* lo, const float* hi, const int* res, int probes, float threshold, int dilate,
                        int precision, void* stream_) {
    CHECK(c, check_build_occupancy(MaybeContext(c).p, lo, hi, res, probes, threshold, dilate, precision));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    TRY(wait_for_launches(c));   // the build ends in a new grid: a queued launch still reads the old one
    const GridBox box(lo, hi, res);
    const Lattice l = probe_lattice(box, probes);
    const int64_t words = occ_words(box.cells);
    // the probes of a chunk of cells and their sigma in a scratch buffer the context keeps: 2^20 points (16 MB) at the most
    HIPCHK(c, c->d_occ_scratch.reserve((size_t)l.chunk_cells * l.per_cell * 4));
    HIPCHK(c, c->d_occ_tmp.reserve((size_t)words * 2));
    float* points = c->d_occ_scratch.get();
    float* sigma = points + (size_t)l.chunk_cells * l.per_cell * 3;
    uint32_t* buf[2] = {c->d_occ_tmp.get(), c->d_occ_tmp.get() + words};
    HIPCHK(c, hipMemsetAsync(buf[0], 0, (size_t)words * sizeof(uint32_t), stream));
    for (const NetState& n : c->net)   // a cell is occupied where either network says so
        if (n.set)
            TRY(query_lattice(c, n, l, box.cells, points, precision, stream, [&](int64_t) { return sigma; }, [&](const float* s, int64_t first, int count) {
                launch_occ_reduce_bits(s, first, count, l.per_cell, threshold, buf[0], stream);
            }));
    int cur = 0;
    for (int d = 0; d < dilate; ++d, cur ^= 1)
        launch_occ_dilate(buf[cur], buf[cur ^ 1], res, stream);
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> host((size_t)words);
    HIPCHK(c, hipMemcpyAsync(host.data(), buf[cur], (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    return install_occupancy(c, box, std::move(host));
}

int nwe_set_coarse_grid(nwe_ctx* c, const float* lo, const float* hi, const int* res, const float* sigma, int on_device) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_set_grid(kCoarseGrid, lo, hi, res, sigma, on_device != 0, c->host_only));
    return set_values_grid(c, c->cgrid, c->d_cgrid, GridBox(lo, hi, res), 1, sigma, on_device != 0);
}

int nwe_clear_coarse_grid(nwe_ctx* c) {
    if (!c) return NWE_ERR_INVALID;
    return clear_values_grid(c, c->cgrid);
}

int nwe_get_coarse_grid(const nwe_ctx* c, float* lo, float* hi, int* res, float* inv) {
    if (!c) return NWE_ERR_INVALID;
    if (!c->cgrid.set) return NWE_ERR_STATE;   // no grid is set: the outputs stay untouched (and so does the error text of a const context)
    c->cgrid.box.read(lo, hi, res, inv);
    return NWE_OK;
}

int nwe_coarse_grid_copy(nwe_ctx* c, float* host_values, int64_t n_values) {
    if (!c) return NWE_ERR_INVALID;
    if (!c->cgrid.set) return NWE_ERR_STATE;
    if (!host_values || n_values != c->cgrid.box.cells) return fail(c, NWE_ERR_INVALID, "coarse grid: the copy needs rx * ry * rz values");
    return copy_values_grid(c, c->cgrid, c->d_cgrid, host_values, n_values);
}

int nwe_bake_coarse_grid(nwe_ctx* c, const float* lo, const float* hi, const int* res, int precision, void* stream_) {
    CHECK(c, check_bake_coarse_grid(MaybeContext(c).p, lo, hi, res, precision));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    TRY(wait_for_launches(c));   // the bake ends in a new grid: a queued launch still reads the old one
    c->cgrid = CoarseGridState{};   // a failing bake leaves no grid
    const GridBox box(lo, hi, res);
    const Lattice l = probe_lattice(box, 1);   // the cells' centres, a chunk of them in the scratch buffer: 12 MB at the most
    HIPCHK(c, c->d_occ_scratch.reserve((size_t)l.chunk_cells * 3));
    HIPCHK(c, c->d_cgrid.reserve((size_t)box.cells));
    float* grid = c->d_cgrid.get();   // the sigma of a chunk goes straight into the grid
    TRY(query_lattice(c, c->net[NWE_NET_COARSE], l, box.cells, c->d_occ_scratch.get(), precision, stream,
                      [&](int64_t first) { return grid + first; }, [](const float*, int64_t, int) {}));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(stream));
    install_coarse_grid(c, box, {});
    return NWE_OK;
}

int nwe_coarse_grid_weights(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
                            float far, int row_begin, int row_end, float* sigma_out_dev, float* weights_out_dev, void* stream_) {
    CHECK(c, check_on_device(c && !c->host_only));
    if (!c->cgrid.set) return fail(c, NWE_ERR_STATE, "coarse grid: no grid is set (nwe_set_coarse_grid, nwe_bake_coarse_grid)");
    if (c->ns <= 0) return fail(c, NWE_ERR_STATE, "nwe_set_sampling has not been called");
    const Camera m{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end};
    CHECK(c, check_camera(m));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    Slot& slot = c->rays_slot;   // not a slot of the ring, like nwe_create_rays: the timing calls keep describing the last render
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, c2w, n_poses, stream));
    RenderArgs a = camera_args(m, slot.poses.get());
    CHECK(c, check_ray_count(a.n_rays, false));
    context_args(c, a);
    if (a.n_rays == 0 || (!sigma_out_dev && !weights_out_dev)) return NWE_OK;
    return record_launch(c, slot, stream, [&]() -> int {
        launch_coarse_grid_weights(a, coarse_grid_args(c), nullptr, sigma_out_dev, weights_out_dev, stream);
        return NWE_OK;
    });
}

int nwe_set_radiance_grid(nwe_ctx* c, const float* lo, const float* hi, const int* res, const float* raw, int on_device) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_set_grid(kRadianceGrid, lo, hi, res, raw, on_device != 0, c->host_only));
    return set_values_grid(c, c->rgrid, c->d_rgrid, GridBox(lo, hi, res), 4, raw, on_device != 0);
}

int nwe_clear_radiance_grid(nwe_ctx* c) {
    if (!c) return NWE_ERR_INVALID;
    return clear_values_grid(c, c->rgrid);
}

int nwe_get_radiance_grid(const nwe_ctx* c, float* lo, float* hi, int* res, float* inv) {
    if (!c) return NWE_ERR_INVALID;
    if (!c->rgrid.set) return NWE_ERR_STATE;   // no grid is set: the outputs stay untouched (and so does the error text of a const context)
    c->rgrid.box.read(lo, hi, res, inv);
    return NWE_OK;
}

int nwe_radiance_grid_copy(nwe_ctx* c, float* host_values, int64_t n_values) {
    if (!c) return NWE_ERR_INVALID;
    if (!c->rgrid.set) return NWE_ERR_STATE;
    if (!host_values || n_values != 4 * c->rgrid.box.cells) return fail(c, NWE_ERR_INVALID, "radiance grid: the copy needs 4 * rx * ry * rz values");
    return copy_values_grid(c, c->rgrid, c->d_rgrid, host_values, n_values);
}

int nwe_bake_radiance_grid(nwe_ctx* c, const float* lo, const float* hi, const int* res, int which, const float* dir3_host, int precision,
                           void* stream_) {
    CHECK(c, check_bake_radiance_grid(MaybeContext(c).p, lo, hi, res, which, dir3_host, precision));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    TRY(wait_for_launches(c));   // the bake ends in a new grid: a queued launch still reads the old one
    c->rgrid = RadianceGridState{};   // a failing bake leaves no grid
    const NetState& n = c->net[which];
    const GridBox box(lo, hi, res);
    const Lattice l = probe_lattice(box, 1);   // the cells' centres, a chunk of them in the scratch buffer, the direction behind them
    HIPCHK(c, c->d_occ_scratch.reserve((size_t)l.chunk_cells * 3 + 3));
    HIPCHK(c, c->d_rgrid.reserve((size_t)box.cells * 4));
    float* points = c->d_occ_scratch.get();
    float* dir = dir3_host ? points + (size_t)l.chunk_cells * 3 : nullptr;
    if (dir) HIPCHK(c, hipMemcpyAsync(dir, dir3_host, 3 * sizeof(float), hipMemcpyHostToDevice, stream));
    for (int64_t first = 0; first < box.cells; first += l.chunk_cells) {   // the rows of a chunk go straight into the grid
        const int count = (int)std::min<int64_t>(l.chunk_cells, box.cells - first);
        launch_occ_probe_points(l.b, first, count, points, stream);
        QueryArgs q = {};
        q.points = points; q.dirs = dir; q.raw = c->d_rgrid.get() + first * 4; q.n_points = count; q.points_per_dir = count;
        if (precision == NWE_PREC_F32) launch_query_f32(q, n.f32, c->query_steps, c->cus, stream);
        else if (!launch_query_mfma(q, n.mf, precision == NWE_PREC_F16X3, c->query_steps, c->cus, stream))
            return fail(c, NWE_ERR_UNSUPPORTED, "no MFMA query kernel in this build for this network shape; use NWE_PREC_F32");
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(stream));
    install_grid(c->rgrid, box, {});
    return NWE_OK;
}

int nwe_render_grid(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near, float far,
                    int row_begin, int row_end, const nwe_grid_outputs* out, void* stream_) {
    const Camera m{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end};
    CHECK(c, check_render_grid(MaybeContext(c).p, out, m));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    Slot& slot = c->grid_slots[c->next_grid];   // not a slot of the render ring (see nwe_create_rays)
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, c2w, n_poses, stream));
    RenderArgs a = camera_args(m, slot.poses.get());
    if (a.n_rays == 0) return NWE_OK;
    a.white_bkgd = c->white_bkgd;   // nothing else of the context: the sampling tables and counts, no mode
    a.t_vals = c->d_t.get(); a.omt_vals = a.t_vals + kMaxSamples; a.u_vals = a.omt_vals + kMaxSamples;
    a.n_samples = c->ns; a.n_importance = c->ni;
    a.out.struct_bytes = sizeof(nwe_outputs);
    a.out.rgb = out->rgb; a.out.depth = out->depth; a.out.acc = out->acc; a.out.flags = out->flags;
    a.out.weights_coarse = out->weights_coarse; a.out.z_fine = out->z_fine; a.out.raw_fine = out->raw_fine;
    TRY(record_launch(c, slot, stream, [&]() -> int {
        launch_radiance_grid_render(a, radiance_grid_args(c), stream);
        return NWE_OK;
    }));
    c->last_grid = (int)(&slot - c->grid_slots);
    c->next_grid = (c->last_grid + 1) % nwe_ctx::kSlots;
    return NWE_OK;
}

float nwe_last_grid_ms(nwe_ctx* c) {
    if (!c || c->host_only || c->last_grid < 0 || !c->grid_slots[c->last_grid].used) return -1.f;
    return elapsed_ms(c, c->grid_slots[c->last_grid], "nwe_last_grid_ms");
}

int nwe_render_sparse(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near, float far,
                      int row_begin, int row_end, int which, int precision, float min_weight, int dilate, const nwe_sparse_outputs* out,
                      void* stream_) {
    const Camera m{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end};
    CHECK(c, check_render_sparse(MaybeContext(c).p, out, m, which, precision, min_weight, dilate));
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t n_rays = (int64_t)n_poses * (row_end - row_begin) * W;
    if (n_rays == 0) return NWE_OK;
    ON_DEVICE(c);
    TRY(wait_for_sparse(c, nullptr));   // an asynchronous call in flight still uses the scratch
    SparseSlot& slot = c->sparse_slots[c->next_sparse];   // not a slot of the render ring (see nwe_create_rays)
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, c2w, n_poses, stream));
    RenderArgs a = camera_args(m, slot.poses.get());
    a.white_bkgd = c->white_bkgd;   // nothing else of the context: the sampling tables and counts, no mode
    a.t_vals = c->d_t.get(); a.omt_vals = a.t_vals + kMaxSamples; a.u_vals = a.omt_vals + kMaxSamples;
    a.n_samples = c->ns; a.n_importance = c->ni;
    a.out.struct_bytes = sizeof(nwe_outputs);
    a.out.rgb = out->rgb; a.out.depth = out->depth; a.out.acc = out->acc; a.out.flags = out->flags;
    const NetState& net = c->net[which];
    const int S = c->ns + c->ni;
    // the rays of a chunk: 2^22 / S, which the test hook may lower; the scratch is laid out for that many
    int64_t cap = std::max<int64_t>(1, kSparseChunkSamples / S);
    if (c->sparse_chunk > 0) cap = std::min<int64_t>(cap, c->sparse_chunk);
    cap = std::min(cap, n_rays);
    const size_t M = (size_t)cap * S;
    size_t bytes = 0;
    const auto take = [&](size_t n) { const size_t at = bytes; bytes += (n + 255) / 256 * 256; return at; };
    const size_t at_grid = take(M * 16), at_rows = take(M * 16), at_z = take(M * 4), at_points = take(M * 12), at_dirs = take(M * 12),
                 at_offsets = take((size_t)cap * 4), at_total = take(4), at_mask = take(M);
    HIPCHK(c, c->d_sparse_scratch.reserve(bytes));   // grow-only; nothing of an earlier call still reads it: the call is synchronous
    if (!c->sparse_word) HIPCHK(c, hipHostMalloc(&c->sparse_word.h, sizeof(uint32_t), hipHostMallocDefault));
    uint8_t* const base = c->d_sparse_scratch.get();
    volatile uint32_t* const word = static_cast<uint32_t*>(c->sparse_word.h);
    SparseChunk k = {};
    k.S = S; k.min_weight = min_weight; k.dilate = dilate;
    k.row_grid = reinterpret_cast<float4*>(base + at_grid); k.rows = reinterpret_cast<const float4*>(base + at_rows);
    k.z = reinterpret_cast<float*>(base + at_z); k.points = reinterpret_cast<float*>(base + at_points);
    k.dirs = net.in_dir != 0 ? reinterpret_cast<float*>(base + at_dirs) : nullptr;
    k.offsets = reinterpret_cast<uint32_t*>(base + at_offsets); k.total = reinterpret_cast<uint32_t*>(base + at_total);
    k.mask = base + at_mask;
    k.weights_coarse = out->weights_coarse; k.z_fine = out->z_fine; k.weights_grid = out->weights_grid; k.raw_fine = out->raw_fine;
    k.selected = out->selected;
    const RadianceGrid grid = radiance_grid_args(c);
    int64_t selected = 0;
    int host_waits = 0;
    const int rc = record_launch(c, slot, stream, [&]() -> int {
        for (int64_t first = 0; first < n_rays; first += cap) {
            k.first = first; k.count = (int)std::min<int64_t>(cap, n_rays - first);
            launch_sparse_mark(a, grid, k, stream);
            launch_sparse_scan(k, stream);
            launch_sparse_emit(a, k, stream);
            HIPCHK(c, hipGetLastError());
            // the one read-back of the chunk: the query's launch needs its n_points on the host
            HIPCHK(c, hipMemcpyAsync(c->sparse_word.h, k.total, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIPCHK(c, hipStreamSynchronize(stream));
            ++host_waits;
            const uint32_t n_points = *word;
            if ((uint64_t)n_points > (uint64_t)k.count * S) return fail(c, NWE_ERR_HIP, "sparse frame: the chunk's point count is out of range");
            selected += n_points;
            if (n_points > 0) {   // the raw path of nwe_query_points, one direction per point; a chunk with nothing selected launches no query
                QueryArgs q = {};
                q.points = k.points; q.dirs = k.dirs; q.raw = reinterpret_cast<float*>(base + at_rows); q.n_points = (int)n_points; q.points_per_dir = 1;
                if (precision == NWE_PREC_F32) launch_query_f32(q, net.f32, c->query_steps, c->cus, stream);
                else if (!launch_query_mfma(q, net.mf, precision == NWE_PREC_F16X3, c->query_steps, c->cus, stream))
                    return fail(c, NWE_ERR_UNSUPPORTED, "no MFMA query kernel in this build for this network shape; use NWE_PREC_F32");
            }
            launch_sparse_composite(a, k, stream);
        }
        return NWE_OK;
    });
    // synchronous, on every path: nothing of the call may still run, or read the scratch, when it returns
    const hipError_t waited = hipStreamSynchronize(stream);
    if (rc) return rc;
    HIPCHK(c, waited);
    c->last_sparse = (int)(&slot - c->sparse_slots);
    c->next_sparse = (c->last_sparse + 1) % nwe_ctx::kSlots;
    c->sparse_selected = selected; c->sparse_total = n_rays * S;
    c->sparse_async = false; c->sparse_host_waits = host_waits + 1;
    return NWE_OK;
}

int nwe_render_sparse_async(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near, float far,
                            int row_begin, int row_end, int which, int precision, float min_weight, int dilate, const nwe_sparse_outputs* out,
                            void* stream_) {
    const Camera m{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end};
    CHECK(c, check_render_sparse(MaybeContext(c).p, out, m, which, precision, min_weight, dilate));
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t n_rays = (int64_t)n_poses * (row_end - row_begin) * W;
    if (n_rays == 0) return NWE_OK;
    ON_DEVICE(c);
    const NetState& net = c->net[which];
    const int S = c->ns + c->ni;
    // the chunks and the scratch of the synchronous call: 2^22 / S rays, which the test hook may lower
    int64_t cap = std::max<int64_t>(1, kSparseChunkSamples / S);
    if (c->sparse_chunk > 0) cap = std::min<int64_t>(cap, c->sparse_chunk);
    cap = std::min(cap, n_rays);
    const size_t M = (size_t)cap * S;
    size_t bytes = 0;
    const auto take = [&](size_t n) { const size_t at = bytes; bytes += (n + 255) / 256 * 256; return at; };
    const size_t at_grid = take(M * 16), at_rows = take(M * 16), at_z = take(M * 4), at_points = take(M * 12), at_dirs = take(M * 12),
                 at_offsets = take((size_t)cap * 4), at_total = take(4), at_mask = take(M);
    int host_waits = 0;
    // the host waits only here: for every sparse call in flight if the scratch has to grow (growing drops it), and for the call that
    // used this slot of the ring four calls ago, normally long finished
    if (bytes > c->d_sparse_scratch.cap) {
        TRY(wait_for_sparse(c, &host_waits));
        HIPCHK(c, c->d_sparse_scratch.reserve(bytes));
    }
    SparseSlot& slot = c->sparse_slots[c->next_sparse];
    if (slot.used && hipEventQuery(slot.ev1) != hipSuccess) { ++host_waits; (void)hipGetLastError(); }
    TRY(prepare_slot(c, slot));
    HIPCHK(c, slot.tally.reserve(1));
    if (!slot.word) HIPCHK(c, hipHostMalloc(&slot.word.h, sizeof(unsigned long long), hipHostMallocDefault));
    // on the device: behind the previous sparse call of either kind, whose chunks use the same scratch, on whatever stream it ran
    if (c->last_sparse >= 0 && c->sparse_slots[c->last_sparse].used) HIPCHK(c, hipStreamWaitEvent(stream, c->sparse_slots[c->last_sparse].ev1, 0));
    TRY(upload_poses(c, slot, c2w, n_poses, stream));
    RenderArgs a = camera_args(m, slot.poses.get());
    a.white_bkgd = c->white_bkgd;   // nothing else of the context: the sampling tables and counts, no mode
    a.t_vals = c->d_t.get(); a.omt_vals = a.t_vals + kMaxSamples; a.u_vals = a.omt_vals + kMaxSamples;
    a.n_samples = c->ns; a.n_importance = c->ni;
    a.out.struct_bytes = sizeof(nwe_outputs);
    a.out.rgb = out->rgb; a.out.depth = out->depth; a.out.acc = out->acc; a.out.flags = out->flags;
    uint8_t* const base = c->d_sparse_scratch.get();
    SparseChunk k = {};
    k.S = S; k.min_weight = min_weight; k.dilate = dilate;
    k.row_grid = reinterpret_cast<float4*>(base + at_grid); k.rows = reinterpret_cast<const float4*>(base + at_rows);
    k.z = reinterpret_cast<float*>(base + at_z); k.points = reinterpret_cast<float*>(base + at_points);
    k.dirs = net.in_dir != 0 ? reinterpret_cast<float*>(base + at_dirs) : nullptr;
    k.offsets = reinterpret_cast<uint32_t*>(base + at_offsets); k.total = reinterpret_cast<uint32_t*>(base + at_total);
    k.mask = base + at_mask;
    k.weights_coarse = out->weights_coarse; k.z_fine = out->z_fine; k.weights_grid = out->weights_grid; k.raw_fine = out->raw_fine;
    k.selected = out->selected;
    const RadianceGrid grid = radiance_grid_args(c);
    unsigned long long* const tally = slot.tally.get();
    const int rc = record_launch(c, slot, stream, [&]() -> int {
        HIPCHK(c, hipMemsetAsync(tally, 0, sizeof(unsigned long long), stream));
        for (int64_t first = 0; first < n_rays; first += cap) {   // the one buffer is reused in stream order
            k.first = first; k.count = (int)std::min<int64_t>(cap, n_rays - first);
            launch_sparse_mark(a, grid, k, stream);
            launch_sparse_scan(k, stream);
            launch_sparse_emit(a, k, stream);
            launch_sparse_tally(k, tally, stream);
            // the counted query: sized for the chunk's samples, it reads the scan's total on the device
            QueryArgs q = {};
            q.points = k.points; q.dirs = k.dirs; q.raw = reinterpret_cast<float*>(base + at_rows); q.n_points = k.count * S; q.points_per_dir = 1;
            if (precision == NWE_PREC_F32) launch_query_f32_counted(q, k.total, net.f32, c->query_steps, c->cus, stream);
            else if (!launch_query_mfma_counted(q, k.total, net.mf, precision == NWE_PREC_F16X3, c->query_steps, c->cus, stream))
                return fail(c, NWE_ERR_UNSUPPORTED, "no MFMA query kernel in this build for this network shape; use NWE_PREC_F32");
            launch_sparse_composite(a, k, stream);
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipMemcpyAsync(slot.word.h, tally, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        return NWE_OK;
    });
    if (rc) {   // a call that failed half way leaves nothing running, as the synchronous one
        (void)hipStreamSynchronize(stream);
        return rc;
    }
    c->last_sparse = (int)(&slot - c->sparse_slots);
    c->next_sparse = (c->last_sparse + 1) % nwe_ctx::kSlots;
    c->sparse_total = n_rays * S;
    c->sparse_async = true; c->sparse_host_waits = host_waits;
    return NWE_OK;
}

int nwe_debug_last_sparse_host_waits(nwe_ctx* c) { return c && c->last_sparse >= 0 ? c->sparse_host_waits : -1; }
unsigned nwe_debug_query_counted_grid(int64_t capacity, int packet, int forced_steps, int cus) {
    return query_counted_grid(capacity, packet, forced_steps, cus);
}

int nwe_debug_set_sparse_chunk(nwe_ctx* c, int rays) { return set_on(rays < 0 ? nullptr : c, [&] { c->sparse_chunk = rays; }); }

float nwe_last_sparse_ms(nwe_ctx* c) {
    if (!c || c->host_only || c->last_sparse < 0 || !c->sparse_slots[c->last_sparse].used) return -1.f;
    return elapsed_ms(c, c->sparse_slots[c->last_sparse], "nwe_last_sparse_ms");
}

int nwe_last_sparse_samples(nwe_ctx* c, int64_t* out2) {
    if (!c || !out2) return NWE_ERR_INVALID;
    if (c->last_sparse < 0) return NWE_ERR_STATE;
    if (c->sparse_async) {   // the tally is in the slot's pinned word once the call's end event has passed
        const SparseSlot& slot = c->sparse_slots[c->last_sparse];
        ON_DEVICE(c);
        HIPCHK(c, hipEventSynchronize(slot.ev1));
        c->sparse_selected = (int64_t)*static_cast<volatile unsigned long long*>(slot.word.h);
        c->sparse_async = false;   // read once
    }
    out2[0] = c->sparse_selected; out2[1] = c->sparse_total;
    return NWE_OK;
}

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
