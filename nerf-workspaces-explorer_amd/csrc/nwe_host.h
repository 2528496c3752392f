// Host/device shared descriptors of the two render kernels and their launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nwe_device.h"
#include "nwe_pack.h"   // LayerF32, NetF32, NetMfma, Form, kTileBytes, kMaxDepth: shared with the HIP-free packers
#include "nwe_plan.h"   // PassPlan and the constants of planning: shared with the HIP-free planner

namespace nwe {

// a.min_trans > 0 (early ray termination, with a.evals set) takes the terminating instantiation of either kernel,
// a.share != kShareOff (shared coarse pass, with a.share_w set) the sharing one
void launch_render_f32(const RenderArgs& a, const NetF32& nc, const NetF32& nf, hipStream_t stream);
// the occupancy kernel of the fp32 path (an occupancy grid is set: a.occ and a.evals); the MFMA launcher takes its own from the
// plan's variant
void launch_render_f32_occ(const RenderArgs& a, const NetF32& nc, const NetF32& nf, hipStream_t stream);

// true if a kernel instantiation exists for this shape (in_dir == 0 exactly for kFormNoViewDirs)
bool mfma_supported(int D, int W, int in_xyz, int in_dir, int skip, int form);
// Carries out the plan of one launch group (plan_pass, nwe_plan.h): looks up the shape's launcher of the plan's variant and issues
// the launches, events and stream waits the plan names.  false: the plan is not ok, or the descriptors do not fit the shape's
// kernels (nothing was launched) - or, with out->side_used, the join of the side launch could not be queued.
struct LaunchResources {
    hipEvent_t mid = nullptr;        // recorded between the two launches of plan 2 (or null)
    unsigned* counters = nullptr;    // a plan with a queued launch: four zeroed words - one ticket counter per launch, the tail
                                     // path's, and the items its second launch rendered
    hipStream_t side = nullptr;      // a plan that forks: the low-priority stream of the second launch, and the events of its
    hipEvent_t fork = nullptr, join = nullptr;   // fork from and join into the caller's stream
};
// What execution reports back.  The side stream is used only if the fork could be recorded and waited on; otherwise the
// second launch follows the first on the caller's stream.
struct LaunchReport {
    bool mid_recorded = false, side_used = false;
};
bool launch_render_mfma(const RenderArgs& a, const NetMfma& nc, const NetMfma& nf, bool three_pass, const PassPlan& plan,
                        const LaunchResources& res, hipStream_t stream, LaunchReport* out);

// true if the shape's kernels of this variant (nwe_plan.h: Variant) are in this library; the terminating and the sharing kernels
// exist for every supported shape but kFormReference
bool mfma_variant_built(int D, int W, int skip, int form, int variant);

// true if the MFMA launch of `a` takes the lean instantiations: no output beyond rgb / depth / acc / flags, no hook, no table, no
// precomputed rays, no stamps (is_lean, nwe_mfma_render.h)
bool mfma_is_lean(const RenderArgs& a);

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

// kQueryPacket, kQueryPacketF32, kQueryMaxSteps, query_steps and query_counted_grid: nwe_plan.h (HIP-free)
void launch_query_f32(const QueryArgs& a, const NetF32& net, int forced_steps, int cus, hipStream_t stream);
// false: no query kernel for the network's shape (the shapes of mfma_supported), or its stream does not fit the instantiation
bool launch_query_mfma(const QueryArgs& a, const NetMfma& net, bool three_pass, int forced_steps, int cus, hipStream_t stream);
// The counted forms (nwe_render_sparse_async): a.n_points is a CAPACITY, the point count is the device word `count`, which the
// kernels read as they start - min(*count, capacity) - so nothing of the launch depends on a value the host would have to wait
// for.  The grid is query_counted_grid's (nwe_plan.h); a.steps is not read.
void launch_query_f32_counted(const QueryArgs& a, const uint32_t* count, const NetF32& net, int forced_steps, int cus, hipStream_t stream);
bool launch_query_mfma_counted(const QueryArgs& a, const uint32_t* count, const NetMfma& net, bool three_pass, int forced_steps, int cus,
                               hipStream_t stream);

// ---- nwe_build_occupancy (nwe_occupancy.hip) ----
// The box of a build as its kernels read it: per axis lo and step = (float)(((double)hi - (double)lo) / res), the step of
// NeRFReplicaInferenceHandler.grid_centres, whose centres are the probes = 1 lattice.
struct OccBuild {
    float lo[3], step[3];
    int res[3];
    int probes;
};
// the probe points [n_cells * probes^3, 3] of cells first .. first + n_cells - 1, cell-major
void launch_occ_probe_points(const OccBuild& b, int64_t first, int n_cells, float* points, hipStream_t stream);
// ORs the bit of every cell of the chunk with a value > threshold or not finite among its per_cell values into `bits`
void launch_occ_reduce_bits(const float* sigma, int64_t first, int n_cells, int per_cell, float threshold, uint32_t* bits, hipStream_t stream);
// dst = src dilated by one cell with the 3 x 3 x 3 box; res = (rx, ry, rz)
void launch_occ_dilate(const uint32_t* src, uint32_t* dst, const int* res, hipStream_t stream);

// ---- baked coarse pass (nwe_set_coarse_grid; nwe_coarse_grid.hip) ----
// The coarse density grid of a context as its producer kernel reads it (by value): inv = (float)res / (hi - lo), formed once on
// the host in fp32; sigma = res[0] * res[1] * res[2] values of sigma_raw at the cell centres, z fastest, on the device.
struct CoarseGrid {
    float lo[3], inv[3];
    int res[3];
    int pad;
    const float* sigma;
};
// The producer: one thread per ray of `a` (pinhole rays: a.poses, the camera, a.t_vals / a.omt_vals, a.n_samples).  table
// [n_samples][n_rays] (the consumer's, sample-major), sigma and weights [n_rays][n_samples]; each may be null.
void launch_coarse_grid_weights(const RenderArgs& a, const CoarseGrid& g, float* table, float* sigma, float* weights, hipStream_t stream);

// ---- radiance grid (nwe_set_radiance_grid, nwe_render_grid; nwe_radiance_grid.hip) ----
// The radiance grid of a context as its kernel reads it (by value): the box as CoarseGrid holds it; rows = res[0] * res[1] * res[2]
// rows (rgb_raw[3], sigma_raw) at the cell centres, z fastest, on the device (16-byte aligned: a device allocation).
struct RadianceGrid {
    float lo[3], inv[3];
    int res[3];
    int pad;
    const float4* rows;
};
constexpr int kGridThreads = 64;   // rays of a workgroup of radiance_grid_render_kernel: one wave
// One thread per ray of `a` (pinhole rays: a.poses, the camera, the sampling tables and counts, a.white_bkgd), both passes from
// the grid; a.out: rgb / depth / acc / flags and the diagnostics weights_coarse / z_fine / raw_fine, each may be null.
void launch_radiance_grid_render(const RenderArgs& a, const RadianceGrid& g, hipStream_t stream);

// ---- sparse frame (nwe_render_sparse; nwe_sparse.hip) ----
// kSparseChunkSamples, the samples of a chunk at the most, and the chunks and scratch of a call (plan_sparse): nwe_plan.h (HIP-free)
// One chunk of a sparse call: rays [first, first + count) of the call `a` describes (camera, tables, counts, white_bkgd, a.n_rays =
// the whole call's).  The [count, S] tables are stored SAMPLE-major, element (s, r) at s * count + r, so that the threads of a
// wave, one per ray, read and write consecutive addresses as they walk their samples.  The compacted lists are ray-major: the
// selected samples of ray r, in sample order, start at offsets[r].
struct SparseChunk {
    int64_t first;          // first ray of the chunk within the call
    int count;              // its rays
    int S;                  // samples of the output pass
    float min_weight;
    int dilate;
    float* z;               // [S][count]
    float4* row_grid;       // [S][count]
    uint8_t* mask;          // [S][count]  selected, 0 / 1
    uint32_t* offsets;      // [count] the rays' selected counts (mark), then their exclusive scan (scan)
    uint32_t* total;        // [1]  the chunk's selected samples (scan)
    float* points;          // [N, 3]  N <= count * S
    float* dirs;            // [N, 3]  or null: a network without view directions
    const float4* rows;     // [N]     the query's rows at `points`
    // the call's outputs, indexed by the ray of the CALL; each may be null
    float *weights_coarse, *z_fine, *weights_grid, *raw_fine;
    uint8_t* selected;
};
// mark: the proposal of every ray of the chunk (z, row_grid, the mask, the counts; weights_coarse / weights_grid straight to the
// caller); scan: counts -> offsets and the total; emit: points and directions of the selected samples; composite: the mix, store_ray
// into a.out, the other diagnostics and the flags.
void launch_sparse_mark(const RenderArgs& a, const RadianceGrid& g, const SparseChunk& c, hipStream_t stream);
void launch_sparse_scan(const SparseChunk& c, hipStream_t stream);
void launch_sparse_emit(const RenderArgs& a, const SparseChunk& c, hipStream_t stream);
void launch_sparse_composite(const RenderArgs& a, const SparseChunk& c, hipStream_t stream);
// nwe_render_sparse_async (nwe_sparse_async.hip): *tally += *c.total, behind the chunk's scan on `stream`
void launch_sparse_tally(const SparseChunk& c, unsigned long long* tally, hipStream_t stream);

// ---- adaptive frame (nwe_render_adaptive; nwe_adaptive.hip) ----
// The frame of an adaptive call as its kernels read it (by value): the lattice axes of the call's rows and columns (nwe_plan.h), the
// regions of the scratch (AdaptivePlan) and the caller's outputs.  Pixel p of the call is ray p of nwe_render's order, below 2^24.
struct AdaptiveFrame {
    AdaptiveAxis h, w;
    int n_poses;
    int pixels, lattice;        // of the whole call
    float tol_rgb, tol_depth;
    int32_t* list;              // [n]  the pixels of a render launch: the lattice's, then the kind 1 pixels in pixel order
    float *c_rgb, *c_depth, *c_acc;   // compact outputs of both launches: the lattice pixels, [pose][i][j], then the kind 1 pixels
    uint8_t* kinds;             // [pixels]
    uint32_t* counts;           // [pixels] 1 for a kind 1 pixel, then the exclusive scan
    uint8_t* busy;              // [n_poses][h.cells][w.cells]
    uint32_t* total;            // [1] the kind 1 pixels
    const uint32_t* render_flags;   // [1] what the two render launches raised
    float *rgb, *depth, *acc;   // the caller's; each may be null
    uint8_t* kind;
    uint32_t* flags;
};
// the lattice pixels into f.list, pose-major, lattice rows then columns
void launch_adaptive_lattice(const AdaptiveFrame& f, hipStream_t stream);
// rays[i] = the row create_rays_kernel writes for pixel f.list[i] of the camera `a` (a.rays null), `cols` = 11 or 8 columns, i < n
void launch_adaptive_rays(const RenderArgs& a, const AdaptiveFrame& f, int n, int cols, float* rays, hipStream_t stream);
// cells -> busy marks; pixels -> kinds and counts; counts -> their exclusive scan and *total; the kind 1 pixels into f.list
void launch_adaptive_classify(const AdaptiveFrame& f, hipStream_t stream);
// every pixel of the frame from the compact outputs: copied (kind 0, 1) or interpolated (kind 2); the kinds and the flags
void launch_adaptive_compose(const AdaptiveFrame& f, hipStream_t stream);

// ---- multi-level adaptive frame (nwe_render_adaptive_levels; nwe_adaptive_levels.hip) ----
// The frame of a multi-level call as its kernels read it (by value): the axes of every level, the regions of the scratch
// (AdaptiveLevelsPlan) and the caller's outputs.  The compact outputs hold the render passes one behind the other in the order
// they ran; slot[p] is pixel p's index in them, -1 while no pass has rendered it.
struct AdaptiveLevelsFrame {
    AdaptiveAxis h[kAdaptiveMaxLevels], w[kAdaptiveMaxLevels];
    int levels, n_poses, pixels;
    float tol_rgb, tol_depth;
    int32_t* list;                    // [n] the pixels of a render pass, ascending
    float *c_rgb, *c_depth, *c_acc;   // compact outputs of all passes
    int32_t* slot;                    // [pixels]
    uint32_t* counts;                 // [pixels] 1 for a pixel of the next pass, then the exclusive scan
    uint8_t* state[kAdaptiveMaxLevels];   // per level [n_poses][h.cells][w.cells]: kAdaptiveInactive / Flat / Busy
    uint32_t* words;                  // [levels][2] {the pixels of pass l + 1, the busy cells of level l}
    uint32_t* interp;                 // [levels] the kind 2 pixels by the level of their cell
    const uint32_t* render_flags;     // [1] what the render launches raised
    // compose alone: the first slot of pass i = 0 .. levels (INT32_MAX for a pass that never ran) and the levels that were classified
    int base[kAdaptiveMaxLevels + 1];
    int classified;
    float *rgb, *depth, *acc;         // the caller's; each may be null
    uint8_t *kind, *level;
    uint32_t* flags;
};
constexpr uint8_t kAdaptiveInactive = 0, kAdaptiveFlat = 1, kAdaptiveBusy = 2;
// pass 0: the level 0 lattice pixels into f.list, pose-major, lattice rows then columns, and their slots
void launch_adaptive_levels_lattice(const AdaptiveLevelsFrame& f, int lattice, hipStream_t stream);
// level l: cells -> states and the busy count; pixels -> the members of pass l + 1; their scan and total; the members into f.list and
// their slots from `first` on
void launch_adaptive_levels_classify(const AdaptiveLevelsFrame& f, int l, int first, hipStream_t stream);
// every pixel of the frame from the compact outputs: copied or interpolated; kinds, levels, flags and the interpolated counts
void launch_adaptive_levels_compose(const AdaptiveLevelsFrame& f, hipStream_t stream);

// Self-test kernels (nwe_selftest.hip)
int run_selftest(int32_t* report8, hipStream_t stream);

}  // namespace nwe
