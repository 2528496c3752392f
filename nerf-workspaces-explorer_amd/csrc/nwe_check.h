// Whether a call may run, and the words it is refused with: plain C++ without HIP (nwe_check.cpp), decided from plain data.
// nwe_abi.hip reads its context into a ContextDesc in one place (describe_context); the checks here and the planner's CallDesc
// (nwe_plan.h) are both made from that.  A check returns a Refusal, the ABI hands its code and text to fail().  Nothing here
// asks a device: what the launchers know of a network (mfma_supported, mfma_variant_built) comes in with the description.
#pragma once
#include <stdint.h>
#include <string>

#include "../../include/nwe.h"
#include "nwe_pack.h"   // NetShape
#include "nwe_plan.h"   // kVariants

namespace nwe {

struct Refusal {
    int code = NWE_OK;
    std::string text;   // stays empty on the way of a call that runs: no check builds a string before it refuses
    explicit operator bool() const { return code != NWE_OK; }
};

// ---- the context as the checks and the planner read it ----

struct NetDesc : NetShape {
    bool set = false;
    int form = kFormFolded;          // MFMA stream: which formulation it holds (nwe_pack.h: Form)
    bool mfma_ok = false;            // mfma_supported() of the shape
    bool built[kVariants] = {};      // mfma_variant_built() of the shape, per variant
};

struct GridDesc {
    bool set = false;
    int res[3] = {};
};

struct ContextDesc {
    NetDesc net[2];
    int ns = 0, ni = 0;
    bool host_only = false;
    float min_trans = 0.f;           // nwe_set_early_termination: 0 = off
    int share_k = 1;                 // nwe_set_shared_coarse: 1 = off
    bool separate = false;           // nwe_set_separate_passes
    GridDesc occ, cgrid;             // nwe_set_occupancy, nwe_set_coarse_grid
    GridDesc rgrid;                  // nwe_set_radiance_grid: read by nwe_render_grid alone, no mode of a render call
    bool stamps = false;             // a stamp buffer is armed (nwe_debug_set_stamps)
    // read by the planner alone
    int decomposition = -1, queue_mode = -1;
    bool backfill = true, tail = true, packet_blocks = true;
};

// ---- render calls ----

// nwe_render / a tile of nwe_render_tiled (pinhole), nwe_render_rays (not), and nwe_debug_plan for either (planning, which a
// host-only context serves).  d: null for a null context.  The modes' refusals come last, in the order of their table.
Refusal check_ready(const ContextDesc* d, const nwe_outputs* out, int precision, bool pinhole, bool planning = false);

// The camera of nwe_render, nwe_render_tiled, nwe_create_rays and nwe_coarse_grid_weights: poses, image, intrinsics, depth range and
// the rows asked for.
struct Camera { const float* c2w; int n_poses, H, W; float fx, fy, cx, cy, near, far; int row_begin, row_end; };
// The one check of a camera, in the order every entry point refuses in; two of its texts are the entry point's own.
enum CameraOf { kCameraOfRender, kCameraOfTiled, kCameraOfCreateRays };
Refusal check_camera(const Camera& m, CameraOf entry = kCameraOfRender);

// The rays of one call: a pinhole call's product of poses, rows and width, or a ray list's count and pointer.
Refusal check_ray_count(int64_t n_rays, bool ray_list, bool null_rays = false);

Refusal check_precision(int precision);
// A network that an MFMA precision is to run has no MFMA kernel.
Refusal no_mfma_kernel();
// An entry point that launches was given no context, or a host-only one.
Refusal check_on_device(bool have_device);

// ---- setters ----

// nwe_set_network (view_dirs) and nwe_set_network_no_view_dirs; null_args: the context, w or b is null.
Refusal check_network(bool null_args, int which, int depth, int width, int in_xyz, int in_dir, int output_ch, bool view_dirs,
                      const float* const* w, const float* const* b);
Refusal check_sampling(bool null_ctx, const float* t_vals, const float* one_minus_t, int n_samples, const float* u, int n_importance);
Refusal check_early_termination(float min_transmittance);
Refusal check_shared_coarse(int k);
Refusal check_separate_passes(int on);

// ---- nwe_query_points: everything it refuses before it needs its device ----
Refusal check_query(const ContextDesc* d, int which, const float* points, int64_t n_points, const float* dirs, int64_t points_per_dir,
                    int precision, const nwe_point_outputs* out);

// ---- the grids ----

// What tells the refusals of the occupancy grid, the coarse density grid and the radiance grid apart.
struct GridKind {
    const char* word;       // opens every text
    int max_res;            // per axis
    bool finite_inv;        // the fp32 resolution / (hi - lo) must be finite too
    const char* values;     // what nwe_set_* calls its array when it is null ...
    const char* from_host;  // ... and when a host-only context is told that it lies on a device
};
extern const GridKind kOccupancyGrid, kCoarseGrid, kRadianceGrid;

// Null pointers, a box that is not finite or not lo < hi on every axis, a resolution outside 1 .. max_res per axis.
Refusal check_grid_box(const GridKind& kind, const float* lo, const float* hi, const int* res);
// nwe_set_occupancy, nwe_set_coarse_grid, nwe_set_radiance_grid: the box, then the array.
Refusal check_set_grid(const GridKind& kind, const float* lo, const float* hi, const int* res, const void* values, bool on_device, bool host_only);
// nwe_build_occupancy, nwe_bake_coarse_grid: what they refuse before they need their device.
Refusal check_build_occupancy(const ContextDesc* d, const float* lo, const float* hi, const int* res, int probes, float threshold, int dilate,
                              int precision);
Refusal check_bake_coarse_grid(const ContextDesc* d, const float* lo, const float* hi, const int* res, int precision);
// nwe_bake_radiance_grid: the same, and the direction rules of the query for the one direction of the bake.
Refusal check_bake_radiance_grid(const ContextDesc* d, const float* lo, const float* hi, const int* res, int which, const float* dir3,
                                 int precision);
// nwe_render_grid, in the order it refuses in: the context, the outputs, the camera, the ray count, grid and sampling, and last -
// so that everything in front can be asked of a host-only context - the device.
Refusal check_render_grid(const ContextDesc* d, const nwe_grid_outputs* out, const Camera& m);
// nwe_render_sparse, in the order it refuses in: the context, the outputs, the camera, the ray count, `which`, the precision, the two
// parameters, grid, sampling and network, the device, and last the query's refusal of a shape without an MFMA kernel.
Refusal check_render_sparse(const ContextDesc* d, const nwe_sparse_outputs* out, const Camera& m, int which, int precision, float min_weight,
                            int dilate);
constexpr int kSparseMaxDilate = 8;
// nwe_render_adaptive, in the order it refuses in: the context, the outputs, the camera, the ray count (nwe_render's, then the
// call's own 2^24), k and the tolerances, the precision, everything check_ready refuses for a lean-output nwe_render_rays, and last -
// so that everything in front can be asked of a host-only context - the device.
Refusal check_adaptive(const ContextDesc* d, const nwe_adaptive_outputs* out, const Camera& m, int precision, int k, float tol_rgb,
                       float tol_depth);
// nwe_render_adaptive_levels: check_adaptive in its order and words, with one refusal more directly behind k: levels outside 1 .. 4 or
// a coarsest spacing k 2^(levels - 1) above 64.
Refusal check_adaptive_levels(const ContextDesc* d, const nwe_adaptive_levels_outputs* out, const Camera& m, int precision, int k, int levels,
                              float tol_rgb, float tol_depth);
Refusal check_adaptive_pixel_lists(int on);
// nwe_render_pixels, in the order it refuses in: the context, the outputs, the camera and its ray count as nwe_render refuses them,
// the list (null_pixels: no list was given), the precision, everything check_ready refuses for a lean-output nwe_render_rays, and
// last - so that everything in front can be asked of a host-only context - the device.
Refusal check_pixels(const ContextDesc* d, const nwe_pixel_outputs* out, const Camera& m, int64_t n_pixels, bool null_pixels, int precision);
// Which way a pixel list that check_pixels (or check_adaptive) has let through is rendered: true = the list kernels (kVariantList),
// false = a ray table through nwe_render_rays' launch.  The list kernels are taken under an MFMA precision when both networks that
// run have one shape whose list kernels are built - which says that they are packed in a product formulation - and neither
// separate passes nor a stamp buffer ask for other kernels.
bool pixel_list_path(const ContextDesc& d, int precision);

}  // namespace nwe
