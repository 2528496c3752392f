// Host/device shared descriptors of the two render kernels and their launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nwe_device.h"
#include "nwe_pack.h"   // LayerF32, NetF32, NetMfma, Form, kTileBytes, kMaxDepth: shared with the HIP-free packers

namespace nwe {

// a.min_trans > 0 (early ray termination, with a.evals set) takes the terminating instantiation of either kernel,
// a.share != kShareOff (shared coarse pass, with a.share_w set) the sharing one
void launch_render_f32(const RenderArgs& a, const NetF32& nc, const NetF32& nf, hipStream_t stream);

// true if a kernel instantiation exists for this shape (in_dir == 0 exactly for kFormNoViewDirs)
bool mfma_supported(int D, int W, int in_xyz, int in_dir, int skip, int form);
// returns false if the shape has no instantiation.  decomposition: -1 = pick by frame size, 0 = four ray packets per
// workgroup, 1 = one packet per workgroup with its samples dealt to the four waves, 2 = full rounds as 0 and the ragged
// last round as 1 in a second launch (bit-identical results)
// *info (may be null): in, `mid` = an event to record between the two launches of plan 2 (or null); out, the plan taken
// (0 / 1 / 2 as above) and the rays the first launch got (all of them unless plan 2)
// Work queue (nwe_debug_set_work_queue; plain kernels only, a terminating or sharing launch stays static): in, `queue` = two
// zeroed device counters, one per launch of the plan, or null, and queue_mode: -1 = queue a launch with more workgroups than the
// device has CUs, 1 = every launch; out, per launch its work items and its grid (0, 0 = not queued).  With a queue the second
// launch of plan 2 goes to `side` (in: a low-priority stream, with `fork` and `join` events of the caller's; all three or
// none), which starts behind `fork` on the caller's stream in front of the first launch and which the caller's stream joins
// behind the second; out, side_used.  false with a side launch queued: the join could not be queued, *info says side_used.
// Tail path (render_mfma_tail_kernel): `queue` then has a third zeroed counter; in, `tail` = the caller allows it; out, tail_items =
// the plan's split items if the path was taken - lean call, queued first launch whose surplus workgroups cover them all, tail
// kernel built, side stream given - and 0 otherwise.  The side stream then forks behind the first launch, not in front of it.
struct LaunchInfo {
    hipEvent_t mid = nullptr;
    int plan = -1;
    int64_t rays_first = 0;
    bool mid_recorded = false;
    unsigned* queue = nullptr;
    int queue_mode = -1;
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    unsigned items[2] = {0, 0}, grid[2] = {0, 0};
    bool side_used = false;
    bool tail = false;
    unsigned tail_items = 0;
};
// true if a plain launch of `a` under this decomposition and queue mode deals at least one launch of its plan from a queue: the
// same plan and the same size test as launch_render_mfma's, for the caller that has to provide the counters and the stream
bool mfma_queues(const RenderArgs& a, int decomposition, int queue_mode);
bool launch_render_mfma(const RenderArgs& a, const NetMfma& nc, const NetMfma& nf, bool three_pass, int decomposition, hipStream_t stream,
                        LaunchInfo* info);

// true if the shape's terminating kernels (early ray termination) were built: every supported shape but kFormReference
bool mfma_term_supported(int D, int W, int skip, int form);

// true if the shape's sharing kernels (shared coarse pass) were built: the same shapes
bool mfma_share_supported(int D, int W, int skip, int form);

// true if the MFMA launch of `a` takes the lean instantiations: no output beyond rgb / depth / acc / flags, no hook, no table, no
// precomputed rays (is_lean, nwe_mfma_render.h)
bool mfma_is_lean(const RenderArgs& a);

int mfma_max_samples();      // n_samples the MFMA kernel's per-wave LDS buffers are sized for

// ---- point query (nwe_query_points): run_network at arbitrary points ----
// Kernel arguments of a query launch (by value).  n_points is below 2^31 (the ABI refuses more), points_per_dir is at least 1
// and clamped to n_points by the launcher, so row and direction indices are 32-bit; offsets are formed in 64 bits.
struct QueryArgs {
    const float* points;    // [n_points, 3] world coordinates (the kernel divides by 10, handler.py:93)
    const float* dirs;      // [ceil(n_points / points_per_dir), 3] view directions, used as given; null: zeros (sigma needs none)
    float* raw;             // [n_points, 4] or null
    float* sigma;           // [n_points] or null
    uint32_t* flags;        // [1] or null
    int n_points;
    int points_per_dir;
    int steps;              // packets (128 points on the MFMA kernels, 16 on the fp32 kernel) a workgroup walks, one per step
    int density_only;       // launch-uniform: raw is null, so the colour layers may be left out where the shape has that path
};

constexpr int kQueryPacket = 128;      // points per step of query_mfma_kernel (32 per wave)
constexpr int kQueryPacketF32 = 16;    // ... of query_f32_kernel
constexpr int kQueryMaxSteps = 256;    // steps per workgroup at the most: one packet workgroup's worth of evaluations of the bench frame (64 + 192 samples)

// Steps per workgroup of a query of `packets` packets; forced (nwe_debug_set_query_steps) > 0 overrides the rule.
// The rule: a workgroup holds a CU by itself, so a launch runs in rounds of one workgroup per CU.  A large query gets EIGHT
// workgroups per CU - the last round, in which CUs idle once their workgroup is done, is then an eighth of the launch at the
// most - and as many steps per workgroup as that leaves, up to kQueryMaxSteps: steps = clamp(packets / (8 CUs), 1, 256).
// The prologue a workgroup amortises over its steps is small (one bias table, ~10 KB from L2, and a barrier: a few per cent
// of ONE step), so a query of up to 8 CUs packets runs one step per workgroup and spreads as widely as it can.
int query_steps(int64_t packets, int forced);
void launch_query_f32(const QueryArgs& a, const NetF32& net, int forced_steps, hipStream_t stream);
// false: no query kernel for the network's shape (the shapes of mfma_supported), or its stream does not fit the instantiation
bool launch_query_mfma(const QueryArgs& a, const NetMfma& net, bool three_pass, int forced_steps, hipStream_t stream);

// Self-test kernels (nwe_selftest.hip)
int run_selftest(int32_t* report8, hipStream_t stream);

}  // namespace nwe
