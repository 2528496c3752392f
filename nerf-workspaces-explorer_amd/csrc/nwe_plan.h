// The plan of a render call: which launches it is, what each of them gets and what the slot must hold for them.  Plain C++
// without HIP (nwe_plan.cpp), pure arithmetic on a handful of integers: nwe_abi.hip describes the call, plan_call() decides,
// and the launchers carry the plan out (nwe_kernel_mfma.hip).  Nothing here asks a device: the CU count is an argument.
// The chunks and the scratch of a sparse frame are planned here as well (plan_sparse; nwe_abi_sparse.hip carries them out).
// The plain constants the decisions rest on live here too, and the device headers take them from here.
#pragma once
#include <stdint.h>

#include "nwe_pack.h"   // Form
#include "nwe_packet_blocks.h"

namespace nwe {

constexpr int kMaxSamples = 128;     // n_samples upper bound (LDS tables)
constexpr int kMaxImportance = 256;  // n_importance upper bound

constexpr int kWaves = 4;
constexpr int kRaysPerWave = 32;
static_assert(kBlockW * kBlockH == kRaysPerWave, "a packet is one pixel block");

// Coarse samples the LDS weight / cdf buffer holds: four packets per workgroup keep one buffer per wave (64 samples); the
// sample-split decomposition has ONE packet per workgroup and one shared buffer, which holds the ABI's full 128 samples
// in half the space - so more than 64 coarse samples always take that decomposition (plan_pass).
constexpr int kPacketMaxSamples = 64;
constexpr int kSplitMaxSamples = kMaxSamples;

// The role of a launch in a call of two (RenderArgs::share & 0xff): the shared coarse pass and separate passes
constexpr int kShareOff = 0, kShareProducer = 1, kShareConsumer = 2;

// The kernel variants a shape is built in, beside its query kernels (nwe_mfma_query.h).  One instantiation unit holds one variant
// of one group of shapes (nwe_mfma_inst.hip); the dispatcher's table has one launcher per shape and variant.
//   plain: eight kernels (three-pass / single-pass, packets / sample split, lean / full)
//   term:  four, early termination (TERM; lean)        share: four, shared coarse pass (SHARE; lean)
//   occ:   four, occupancy grid (render_mfma_occ_kernel; lean)
//   tail:  two, render_mfma_tail_kernel (three-pass / single-pass, each holding both decompositions; lean)
//   list:  four, pixel list (render_mfma_list_kernel; lean): the rays of listed pixels of a pinhole view (nwe_render_pixels)
// The first four and the last are what a plan's `variant` may say (nwe_debug_plan reports the number); the tail kernel is taken
// through PassPlan::tail.
enum Variant { kVariantPlain, kVariantTerm, kVariantShare, kVariantOcc, kVariantTail, kVariantList, kVariants };

// Whether a shape has a variant's kernels: the terminating, the sharing, the occupancy and the list kernels exist for the product
// formulations, kFormReference is a comparison path; every form has the plain kernels and, with them, the queue and the tail kernel.
constexpr bool variant_built(int variant, int form) {
    return variant == kVariantTerm || variant == kVariantShare || variant == kVariantOcc || variant == kVariantList ? form != kFormReference : true;
}

// The grid of a queued MFMA launch of n work items (nwe_debug_set_work_queue): n plus a quarter, rounded up to a multiple of 8.
// The hardware deals a grid's workgroups to the 8 XCDs in turn, an eighth each; with a quarter more workgroups than items an
// XCD up to 25 % faster than the mean still finds workgroups in its eighth to take tickets with.
inline unsigned queue_grid(unsigned n) { return (unsigned)(((uint64_t)n + (n + 3) / 4 + 7) / 8 * 8); }

// workgroups (= work items) of a launch of `rays` rays (split: one packet per workgroup)
inline unsigned mfma_workgroups(int64_t rays, bool split) {
    const int64_t per_wg = split ? kRaysPerWave : kWaves * kRaysPerWave;
    return (unsigned)((rays + per_wg - 1) / per_wg);
}

// ---- one launch group: the MFMA launches of one stage of a call ----

struct PassDesc {
    int64_t n_rays = 0;
    int n_samples = 0, n_importance = 0;
    int role = kShareOff;          // costs the launch: a producer runs the coarse pass alone, a consumer the fine pass alone
    int variant = kVariantPlain;   // the kernels the stage takes: plain, term, share, occ or list; -1 = none can serve it (the plan is not ok)
    bool lean = false;             // only rgb / depth / acc / flags of pinhole views, no hook, no table (is_lean without the stamps)
    bool stamps = false;           // a stamp buffer is set (nwe_debug_set_stamps): such a launch is not lean ...
    bool stamped_build = false;    // ... except, in a -DNWE_STAMPS build, for the tail path, whose kernel stamps all the same
    bool tail_built = false;       // the shape has the tail kernel
    int decomposition = -1;        // nwe_debug_set_decomposition: -1 = by cost, 0 / 1 / 2 forces a plan
    int queue_mode = -1;           // nwe_debug_set_work_queue: -1 = a launch with more work items than CUs, 1 = every launch
    bool may_queue = false;        // the queue may be used at all: plain and list kernels only, and not under queue mode 0
    bool side = false;             // a side stream is on offer for the second launch (NWE_WORK_QUEUE_BACKFILL)
    bool tail = false;             // the tail path is allowed (NWE_WORK_QUEUE_TAIL)
};

// One kernel launch: `rays` rays from ray_first on, as `items` work items of four packets or (split) one packet each; grid = the
// workgroups of a queued launch, which take tickets from the call's counter of this launch's index, 0 = dealt by the hardware.
struct LaunchPlan {
    int64_t ray_first = 0, rays = 0;
    bool split = false;
    unsigned items = 0, grid = 0;
};

enum Fork { kForkNone, kForkFront, kForkBehind };

struct PassPlan {
    bool ok = false;          // false: no kernel serves the description (the caller refuses the call); the rest then says nothing
    int variant = kVariantPlain;
    int plan = -1;            // 0 = all packets, 1 = all sample-split, 2 = hybrid: full rounds as packets, the ragged rest sample-split
    int n_launches = 0;       // 1, or 2 under plan 2 (either of which may be empty)
    LaunchPlan launch[2];
    // Plan 2 with a queued launch and a side stream on offer: the second launch goes to the side stream, which forks from the
    // caller's stream in front of the first launch (backfill: its quarter-size items are there the moment the packets run out)
    // or - tail path - behind it (the second launch reads the third counter's final value), and is joined behind the second.
    int fork = kForkNone;
    // The tail path: the surplus workgroups of the queued packets launch render the split items (tail kernel, both launches),
    // taken only when they cover every one of them; tail_items = those items, 0 when the path is not taken.
    bool tail = false;
    unsigned tail_items = 0;
    bool queued() const { return launch[0].grid || launch[1].grid; }
};

PassPlan plan_pass(const PassDesc& d, int cus);

// ---- the whole call ----

struct CallDesc {
    int64_t n_rays = 0;
    int64_t n_rep = 0;             // representatives of the call at the context's k (share_n_rep): the producer's rays under sharing
    int n_samples = 0, n_importance = 0;
    bool mfma = false;             // an MFMA precision (the fp32 launcher has no plan: its passes are not planned)
    bool term = false;             // nwe_set_early_termination > 0
    bool occ = false;              // an occupancy grid is set (nwe_set_occupancy): excludes term, sharing and separate passes
    int share_k = 1;               // nwe_set_shared_coarse
    bool separate = false;         // nwe_set_separate_passes
    bool baked = false;            // a coarse density grid is set (nwe_set_coarse_grid): excludes term, occ, k > 1 and separate passes
    bool lean = false, stamps = false, stamped_build = false;   // as in PassDesc
    bool w_in = false;             // the coarse-weights hook is armed (nwe_debug_set_coarse_weights)
    bool want_weights_coarse = false, want_flags = false;        // outputs requested
    bool built[2][kVariants] = {};                               // per network (coarse, fine): the variants its shape has
    int decomposition = -1, queue_mode = -1;
    bool backfill = true, tail = true;
    int rows = 0, width = 0;       // a pinhole call: the rows rendered per pose and the image width; 0 for a ray list
    bool packet_blocks = false;    // nwe_debug_set_packet_blocks
    // A pixel-list call (nwe_render_pixels on the list kernels): planned as a ray list of n_rays rays (rows = width = 0: no packet
    // blocks, no tail path), but lean - its kernels make the rays themselves - and on the shape's list kernels.  The caller has
    // checked pixel_list_path (nwe_check.h): no mode is on.
    bool list = false;
};

// One stage = one launch group with its own RenderArgs: the coarse stage (the producer of a shared coarse pass, the coarse
// launch of separate passes) where the call has one, and the main stage, which every call has.
struct StagePlan {
    bool active = false;
    int role = kShareOff;     // with k: RenderArgs::share = role | k << 8
    int64_t n_rays = 0;
    int n_importance = 0;
    int net = 0;              // the network (0 coarse, 1 fine) in BOTH descriptor slots under separate passes; -1: (coarse, fine)
    PassPlan pass;            // MFMA precisions only
};

struct CallPlan {
    bool separate = false;        // two launches, each with its own network's kernels
    bool share = false;           // ... through the sharing kernels (and every shared coarse pass)
    bool full = false;            // ... through the full kernels: separate && !share
    bool coarse_launch = false;   // the call has a coarse stage (none with the coarse-weights hook armed under `full`)
    bool may_queue = false;       // a launch of the main stage is queued: the slot provides zeroed counters and, with the
    bool need_side = false;       //   backfill on, the side streams exist
    bool need_evals = false;      // early termination, occupancy grid: the slot provides a zeroed evaluation counter
    bool occ = false;             // the main stage reads the context's occupancy grid (both kernels' occupancy instantiations)
    bool baked = false;           // baked coarse pass: the coarse stage is the grid producer (nwe_coarse_grid.hip), which has no
                                  //   PassPlan; the main stage is the sharing consumer at k = 1 with the fine network's kernels
    int share_k = 1;              // the k in both stages' share word
    bool blocks = false;          // the call is blocked (nwe_packet_blocks.h): the launches carry kPacketBlocksBit
    int64_t table_elems = 0;      // the slot's weight table must hold this many floats (0: none, or the caller's own table serves)
    bool coarse_flags = false;    // the coarse launch's flags go through a word of the slot's (masked into the caller's)
    int64_t evals_full = 0, evals_run = 0, share_rays = 0;   // nwe_last_ray_evaluations, nwe_last_coarse_launch
    StagePlan coarse, main;
};

CallPlan plan_call(const CallDesc& c, int cus);

// ---- point query (nwe_query_points) ----
constexpr int kQueryPacket = 128;      // points per step of query_mfma_kernel (32 per wave)
constexpr int kQueryPacketF32 = 16;    // ... of query_f32_kernel
constexpr int kQueryMaxSteps = 256;    // steps per workgroup at the most: one packet workgroup's worth of evaluations of the bench frame (64 + 192 samples)

// Steps per workgroup of a query of `packets` packets; forced (nwe_debug_set_query_steps) > 0 overrides the rule.
// The rule: a workgroup holds a CU by itself, so a launch runs in rounds of one workgroup per CU.  A large query gets EIGHT
// workgroups per CU - the last round, in which CUs idle once their workgroup is done, is then an eighth of the launch at the
// most - and as many steps per workgroup as that leaves, up to kQueryMaxSteps: steps = clamp(packets / (8 CUs), 1, 256).
// The prologue a workgroup amortises over its steps is small (one bias table, ~10 KB from L2, and a barrier: a few per cent
// of ONE step), so a query of up to 8 CUs packets runs one step per workgroup and spreads as widely as it can.
int query_steps(int64_t packets, int forced, int cus);
// Workgroups of a COUNTED query launch (nwe_render_sparse_async: the point count is a device word, the host knows a capacity):
// min(ceil(capacity / packet), 8 CUs) - the eight workgroups per CU of the rule above, which then walk the packets below the
// count in strides of the grid; forced (nwe_debug_set_query_steps) > 0 makes it ceil(ceil(capacity / packet) / forced), so that
// a small test walks more than one packet per workgroup.  0 for a capacity of 0.
unsigned query_counted_grid(int64_t capacity, int packet, int forced, int cus);

// ---- sparse frame (nwe_render_sparse, nwe_render_sparse_async) ----
constexpr int64_t kSparseChunkSamples = (int64_t)1 << 22;   // samples of a chunk at the most: rays * S

// The chunks of a sparse call of either kind and the scratch they share, laid out for the rays of one chunk.  The regions, in the
// order of their offsets, each rounded up to 256 bytes: the grid's and the query's rows (16 M each), z (4 M), points and directions
// (12 M each), the rays' offsets (4 cap), the chunk's total (4), the mask (M).  n_rays >= 1, S >= 1: a call without rays plans nothing.
struct SparsePlan {
    int64_t cap = 0;       // rays of a chunk: 2^22 / S, at least 1, at most the hook (nwe_debug_set_sparse_chunk, 0 = none) and n_rays
    int64_t chunks = 0, M = 0;   // ceil(n_rays / cap) chunks, of cap * S samples
    int64_t at_grid = 0, at_rows = 0, at_z = 0, at_points = 0, at_dirs = 0, at_offsets = 0, at_total = 0, at_mask = 0;   // byte offsets
    int64_t bytes = 0;     // of the whole scratch: the end of the last region
};
SparsePlan plan_sparse(int64_t n_rays, int S, int chunk_hook);

// ---- adaptive frame (nwe_render_adaptive) ----
constexpr int kAdaptiveMaxK = 64;
constexpr int64_t kAdaptiveMaxRays = (int64_t)1 << 24;   // rays of a call at the most: bounds the scratch

// One axis of a call's lattice (include/nwe.h), in LOCAL coordinates 0 .. len - 1 (a row axis: h - row_begin): the entries
// {i k < len} and len - 1, ascending.  The kernels of nwe_adaptive.hip and the planner compile these few functions.
struct AdaptiveAxis {
    int len, k;
    int n;        // lattice entries: ceil(len / k), and one more where len - 1 is no multiple of k
    int cells;    // max(n - 1, 1): a single entry bounds one degenerate cell
};
NWE_HOST_DEVICE inline AdaptiveAxis adaptive_axis(int len, int k) {
    AdaptiveAxis x;
    x.len = len; x.k = k;
    x.n = (len + k - 1) / k + ((len - 1) % k != 0 ? 1 : 0);
    x.cells = x.n > 1 ? x.n - 1 : 1;
    return x;
}
NWE_HOST_DEVICE inline int adaptive_entry(const AdaptiveAxis& x, int i) { const int v = i * x.k; return v < x.len - 1 ? v : x.len - 1; }   // i < n
NWE_HOST_DEVICE inline bool adaptive_on_lattice(const AdaptiveAxis& x, int v) { return v % x.k == 0 || v == x.len - 1; }
NWE_HOST_DEVICE inline int adaptive_index(const AdaptiveAxis& x, int v) { return v % x.k == 0 ? v / x.k : x.n - 1; }   // of a lattice coordinate
// min(largest i with entry(i) <= v, cells - 1)
NWE_HOST_DEVICE inline int adaptive_cell(const AdaptiveAxis& x, int v) { const int i = v / x.k; return i < x.cells - 1 ? i : x.cells - 1; }

// The lattice and the scratch of an adaptive call.  The regions, in the order of their offsets, each rounded up to 256 bytes: the
// pixel list (4 per ray of the larger launch), its rays (4 cols each), the compact rgb / depth / acc of both launches (lattice
// first; 12 + 4 + 4 per pixel), the kinds (1 per pixel), the counts and their scan (4 per pixel), the cells' busy marks (1 per
// cell), the total and the render launches' flag word (4 each).  n_poses, rows, width >= 1: a call without rays plans nothing.
struct AdaptivePlan {
    AdaptiveAxis h, w;
    int n_poses = 0, cols = 0;
    int64_t pixels = 0, lattice = 0, cells = 0;   // of the whole call
    int64_t list = 0;                              // rays of a render launch at the most: max(lattice, pixels - lattice)
    int64_t at_list = 0, at_rays = 0, at_rgb = 0, at_depth = 0, at_acc = 0, at_kind = 0, at_counts = 0, at_busy = 0, at_total = 0, at_flags = 0;
    int64_t bytes = 0;
};
AdaptivePlan plan_adaptive(int n_poses, int rows, int width, int k, int ray_cols);
// The lattice of [first, last_excl) in image coordinates, ascending, into out[0 .. cap): returns its entries, or -1 for an empty
// range, k outside 1 .. kAdaptiveMaxK, a null array or one that is too small.
int adaptive_lattice(int first, int last_excl, int k, int32_t* out, int cap);

// ---- multi-level adaptive frame (nwe_render_adaptive_levels) ----
constexpr int kAdaptiveMaxLevels = 4;
// The spacing of level l of `levels` over the finest spacing k: k 2^(levels - 1 - l)
NWE_HOST_DEVICE inline int adaptive_level_spacing(int k, int levels, int l) { return k << (levels - 1 - l); }
// levels in 1 .. kAdaptiveMaxLevels and the coarsest spacing within kAdaptiveMaxK
inline bool adaptive_levels_ok(int k, int levels) {
    return k >= 1 && k <= kAdaptiveMaxK && levels >= 1 && levels <= kAdaptiveMaxLevels && ((int64_t)k << (levels - 1)) <= kAdaptiveMaxK;
}

// The lattices and the scratch of a multi-level call.  Level l has the axes h[l], w[l] (adaptive_axis at its spacing); render pass 0
// holds the level 0 lattice, pass l = 1 .. levels - 1 at the most the pixels of the level l lattice that are not on level l - 1's,
// pass `levels` at the most the pixels off the finest lattice.  The regions, in the order of their offsets, each rounded up to 256
// bytes: the pixel list (4 per pixel of the largest pass), its rays (4 cols each), the compact rgb / depth / acc of all passes in
// the order they run (12 + 4 + 4 per pixel), the slots (4 per pixel), the counts and their scan (4 per pixel), the cells' states
// (1 per cell, level by level), the words ({next pass, busy cells} per level, 4 each), the interpolated pixels per level (4 each)
// and the render launches' flag word (4).  n_poses, rows, width >= 1 and adaptive_levels_ok(k, levels).
struct AdaptiveLevelsPlan {
    int levels = 0, n_poses = 0, cols = 0;
    AdaptiveAxis h[kAdaptiveMaxLevels], w[kAdaptiveMaxLevels];
    int64_t pixels = 0, lattice = 0;                      // of the whole call; lattice = pass 0
    int64_t cells[kAdaptiveMaxLevels] = {};               // of the whole call, per level
    int64_t pass_max[kAdaptiveMaxLevels + 1] = {};        // the most pixels each render pass can hold
    int64_t list = 0;                                     // max over pass_max
    int64_t at_list = 0, at_rays = 0, at_rgb = 0, at_depth = 0, at_acc = 0, at_slot = 0, at_counts = 0, at_state[kAdaptiveMaxLevels] = {},
            at_words = 0, at_interp = 0, at_flags = 0;
    int64_t bytes = 0;
};
AdaptiveLevelsPlan plan_adaptive_levels(int n_poses, int rows, int width, int k, int levels, int ray_cols);
// The lattice of level `level` of `levels` over [first, last_excl), as adaptive_lattice; -1 also where adaptive_levels_ok fails or
// the level is outside 0 .. levels - 1.
int adaptive_levels_lattice(int first, int last_excl, int k, int levels, int level, int32_t* out, int cap);

}  // namespace nwe
