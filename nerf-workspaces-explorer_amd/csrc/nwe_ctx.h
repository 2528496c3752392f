// Private to the units of the C ABI (nwe_abi.hip: context, networks, the render, tiled, ray and query calls; nwe_abi_grids.hip: the
// three grids and the grid frame; nwe_abi_sparse.hip: the sparse frames; nwe_abi_adaptive.hip: the adaptive frame; nwe_abi_pixels.hip: the pixel list): the context, what it owns on its device, and the
// helpers that more than one of the units needs (defined in nwe_abi.hip unless said otherwise).
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "nwe_check.h"
#include "nwe_host.h"

namespace nwe {

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
    // pixel list (nwe_render_pixels): the word the launch's flags go through (or_masked_flags_kernel: only the rgb / depth / acc bits
    // reach the caller's) and, where the call renders through a ray table, the clamped list and the table (last reader: prepare_slot)
    DevBuf<uint32_t> pixel_flags;
    DevBuf<int32_t> pixel_list;
    DevBuf<float> pixel_rays;
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
    // The box as the kernels read it, in the head of a grid's descriptor: OccGrid, CoarseGrid, RadianceGrid
    template <class G>
    G args() const {
        G g = {};
        for (int i = 0; i < 3; ++i) { g.lo[i] = lo[i]; g.inv[i] = inv[i]; g.res[i] = res[i]; }
        return g;
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

// A ring of launch slots and the two places in it.  next(): the slot the next call takes.  commit(): the call has been RECORDED,
// the ring moves on - a refused call commits nothing and leaves the reports alone.  last(): the most recent recorded launch, or null.
template <class S>
struct Ring {
    static constexpr int kSlots = 4;
    S slots[kSlots];
    int next_slot = 0, last_slot = -1;
    S& next() { return slots[next_slot]; }
    void commit(const S& s) { last_slot = (int)(&s - slots); next_slot = (last_slot + 1) % kSlots; }
    const S* last() const { return last_slot >= 0 && slots[last_slot].used ? &slots[last_slot] : nullptr; }
};

}  // namespace nwe

using namespace nwe;   // the units of the ABI, which alone include this header, are written in it

struct nwe_ctx {
    int device = -1;
    bool host_only = false;
    int cus = 256;            // the device's compute units, asked once by nwe_create: what the launch plans and the query's steps count rounds in
    NetState net[2];
    DevBuf<float> d_t;        // t_vals | one_minus_t | u, at 0, kMaxSamples and 2 kMaxSamples
    int ns = 0, ni = 0;
    Ring<RenderSlot> render;             // nwe_render, nwe_render_rays: last() is what nwe_last_kernel_ms and the other reports of a launch describe
    Slot rays_slot;                      // nwe_create_rays: a pose table and events of its own, outside the timing ring
    // nwe_query_points: a ring of its own, outside the render ring like rays_slot, so that a query moves none of the render
    // launches' reports (nwe_last_query_ms)
    Ring<Slot> query;
    int query_steps = 0;      // nwe_debug_set_query_steps: 0 = automatic
    // nwe_render_grid: a ring of its own as well, so that a grid frame moves none of the render launches' or the query's reports
    // (nwe_last_grid_ms)
    Ring<Slot> grid;
    // nwe_render_sparse: one more ring of its own (nwe_last_sparse_ms), what the last call selected of how many samples
    // (nwe_last_sparse_samples); the chunks' scratch, grow-only, and the pinned word a chunk's total is read back through.
    // nwe_render_sparse_async shares the ring, the scratch and the reports: sparse_async says which kind the last call was (its selected
    // samples are then in the slot's pinned word), sparse_host_waits how often it made the host wait (nwe_debug_last_sparse_host_waits)
    Ring<SparseSlot> sparse;
    int64_t sparse_selected = 0, sparse_total = 0;
    bool sparse_async = false;
    int sparse_host_waits = -1;
    int sparse_chunk = 0;     // nwe_debug_set_sparse_chunk: 0 = the default
    DevBuf<uint8_t> d_sparse_scratch;
    Owned<void*, hipHostFree> sparse_word;
    // nwe_render_adaptive: a slot of its own for its pose table and the span of the call (nwe_last_adaptive) - its two render launches
    // take slots of the render ring -, the scratch, grow-only, the pinned word the kind 1 count is read back through, and the counts of
    // the last call that ran {pixels, lattice, rendered, interpolated}
    Slot adaptive_slot;
    DevBuf<uint8_t> d_adaptive_scratch;
    Owned<void*, hipHostFree> adaptive_word;
    int64_t adaptive_counts[4] = {0, 0, 0, 0};
    bool adaptive_ran = false;
    int adaptive_lists = 0;   // nwe_set_adaptive_pixel_lists: 0 = off
    // nwe_render_adaptive_levels: its own slot, its pinned words - {next pass, busy cells} of a read-back, then the interpolated
    // counts - and its report {pixels, lattice, levels, render_launches, rendered[4], interpolated[4]}; the scratch is d_adaptive_scratch
    Slot adaptive_levels_slot;
    Owned<void*, hipHostFree> adaptive_levels_words;
    int64_t adaptive_levels_counts[4 + 2 * kAdaptiveMaxLevels] = {};
    bool adaptive_levels_ran = false;
    // nwe_last_pixels: the last pixel-list launch that was recorded - nwe_render_pixels, or a render launch of the adaptive frame
    // under nwe_set_adaptive_pixel_lists - its pixels and its path (1 list kernels, 0 ray table); -1: none yet
    int64_t pixels_n = 0;
    int pixels_path = -1;
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

namespace nwe {

int fail(nwe_ctx* c, int code, const std::string& msg);   // c's error, or - c is null - nwe_create's; returns code
ContextDesc describe_context(const nwe_ctx* c);           // the context as plain data: what a call is checked against and planned from
int prepare_slot(nwe_ctx* c, Slot& s);                    // waits for the launch that used the slot last
int upload_poses(nwe_ctx* c, Slot& s, const float* c2w, int n_poses, hipStream_t stream);
RenderArgs camera_args(const Camera& m, const float* poses_dev);
void context_args(const nwe_ctx* ctx, RenderArgs& a);     // what the context holds for every render call
// The camera-only RenderArgs of a grid or sparse frame: of the context the background, the sampling tables and the counts, no mode
RenderArgs frame_args(const nwe_ctx* c, const Camera& m, const float* poses_dev, float* rgb, float* depth, float* acc, uint32_t* flags);
int wait_for_sparse(nwe_ctx* c, int* waits);              // the sparse calls in flight; *waits counts the slots that had not finished
int wait_for_launches(nwe_ctx* c);                        // all of the context's launches
float elapsed_ms(nwe_ctx* c, const Slot* last, const char* who);   // the time of a ring's last() launch, or -1
// One query launch: the fp32 or the MFMA kernel by the precision, in its counted form (q.n_points a capacity, *count the points, on
// the device) where `count` is given.  Refuses where the build has no MFMA query kernel for the network's shape.
int run_query(nwe_ctx* c, const NetState& net, const QueryArgs& q, int precision, hipStream_t stream, const uint32_t* count = nullptr);
// One render launch of a ray list on the next slot of the render ring, planned and carried out as every render launch is:
// nwe_render_rays with its one-shot hooks and training tables (hooks), nwe_render_adaptive without.  The checks are the caller's.
// flags_mask != 0: the launch raises its flag bits into a word of its slot's, and only the bits of the mask reach out.flags.
int render_ray_list(nwe_ctx* c, const ContextDesc& desc, const float* rays_dev, int64_t n_rays, int precision, const nwe_outputs& out, bool hooks,
                    hipStream_t stream, uint32_t flags_mask = 0);
// One render launch of a pixel list on the list kernels (render_mfma_list_kernel), on the next slot of the render ring: ray i is
// the ray of pixel list_dev[i], clamped, of the pinhole view `cam` (camera_args over a pose table on the device that stays valid
// until the launch has run) with n_poses poses.  The caller has checked pixel_list_path (nwe_check.h); lean outputs only.
int render_pixel_list(nwe_ctx* c, const ContextDesc& desc, const RenderArgs& cam, int n_poses, const int32_t* list_dev, int64_t n, int precision,
                      const nwe_outputs& out, hipStream_t stream, uint32_t flags_mask = 0);
int prepare_slot(nwe_ctx* c, RenderSlot& s);              // ... and forgets the render slot's parts
CoarseGrid coarse_grid_args(const nwe_ctx* ctx);          // the context's grids as their kernels take them (nwe_abi_grids.hip)
RadianceGrid radiance_grid_args(const nwe_ctx* ctx);

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

// describe_context of a context that may be null: what the checks that refuse a null context take
struct MaybeContext {
    ContextDesc d;
    const ContextDesc* p = nullptr;
    explicit MaybeContext(const nwe_ctx* c) { if (c) { d = describe_context(c); p = &d; } }
};

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

template <class T>
int copy_out(const std::vector<T>* v, void* host_dst, int64_t count) {
    if (!v || !host_dst || count != (int64_t)v->size()) return NWE_ERR_INVALID;
    std::memcpy(host_dst, v->data(), (size_t)count * sizeof(T));
    return NWE_OK;
}

// The setters' guard: they refuse a null context and say nothing else (no error text).
template <class Set>
int set_on(nwe_ctx* c, Set&& set) { if (!c) return NWE_ERR_INVALID; set(); return NWE_OK; }

}  // namespace nwe
