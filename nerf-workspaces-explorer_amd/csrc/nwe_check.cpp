// The refusals of the C ABI (nwe_check.h): plain C++ without HIP.
#include "nwe_check.h"

#include <cmath>
#include <cstring>

namespace nwe {

namespace {

Refusal refuse(int code, std::string text) { return Refusal{code, std::move(text)}; }
Refusal invalid(std::string text) { return refuse(NWE_ERR_INVALID, std::move(text)); }
Refusal unsupported(std::string text) { return refuse(NWE_ERR_UNSUPPORTED, std::move(text)); }
Refusal state(std::string text) { return refuse(NWE_ERR_STATE, std::move(text)); }

// nwe_set_sampling lets no more samples through than the sample-split MFMA kernels hold, so no render call asks about them
static_assert(kMaxSamples <= kSplitMaxSamples, "check_ready would have to refuse n_samples under the MFMA precisions");

std::string times(const int* res) { return std::to_string(res[0]) + " x " + std::to_string(res[1]) + " x " + std::to_string(res[2]); }

// ---- the opt-in modes of a context and which of them are not built together ----
//
// A mode is one row of kModes; what it cannot be combined with is one row of kExclusions per pair.  check_ready walks the modes
// that are on in the order of the table: first the mode's exclusions, in the order of theirs, then the calls the mode cannot
// serve.  The texts grew mode by mode and are not uniform; what differs is data here, and none of it may be regularised -
// callers and tests match the texts.

enum ModeId { kModeShare, kModeTerm, kModeSeparate, kModeOcc, kModeBaked, kModes };

struct Mode {
    const char* name;       // as the mode that refuses and as the other party of an exclusion
    const char* is_on;      // ... " is on" / " are on" / " is set", in front of its setter and parameters
    const char* setter;
    const char* it_is;      // the subject of "... not built together with"
    const char* off;        // closes a refusal: how to switch the mode off for the call
    bool mfma_only;         // as the mode that refuses it stands aside under NWE_PREC_F32 (as the other party it does not)
    // the modes with kernels of their own, lean pinhole calls only: nwe_render_rays in the mode's words, what its kernels are
    // called, their variant; fine_only: the coarse network runs no kernel; no_stamps: nor is there one for a stamped launch
    const char* no_rays;
    const char* kind;
    int variant;
    bool fine_only, no_stamps;
};

const Mode kModeTable[kModes] = {
    {"the shared coarse pass", " is on", "nwe_set_shared_coarse", "it is", "; set shared_coarse to 1 for this call", false,
     "nwe_render_rays has no pixel grid to share over", "sharing", kVariantShare, false, false},
    {"early termination", " is on", "nwe_set_early_termination", "it is", "; set min_transmittance to 0 for this call", false,
     "nwe_render_rays, its hooks and its training tables are not terminated", "terminating", kVariantTerm, false, false},
    {"separate passes", " are on", "nwe_set_separate_passes", "they are", "; set separate_passes to 0 for this call", true,
     nullptr, nullptr, -1, false, false},
    {"an occupancy grid", " is set", "nwe_set_occupancy", "it is", "; call nwe_clear_occupancy for this call", false,
     "nwe_render_rays, its hooks and its training tables do not read the grid", "occupancy", kVariantOcc, false, true},
    {"a coarse density grid", " is set", "nwe_set_coarse_grid", "it is", "; call nwe_clear_coarse_grid for this call", false,
     "nwe_render_rays, its hooks and its training tables do not read the grid", "sharing", kVariantShare, true, true},
};

struct Exclusion {
    ModeId mode, other;     // `mode` refuses while `other` is on
    const char* because;    // behind the other party's name
    const char* remedy;
};

const Exclusion kExclusions[] = {
    {kModeShare, kModeTerm, "", "switch one of them off"},
    {kModeSeparate, kModeTerm, ", which would need terminating consumer kernels", "switch one of them off"},
    {kModeOcc, kModeTerm, "", "switch one of them off"},
    {kModeOcc, kModeShare, "", "switch one of them off"},
    {kModeOcc, kModeSeparate, "", "switch one of them off"},
    {kModeBaked, kModeTerm, "", "switch one of them off"},
    {kModeBaked, kModeShare, "", "switch one of them off"},
    {kModeBaked, kModeSeparate, "", "switch one of them off"},
    {kModeBaked, kModeOcc, "", "clear one of them"},
};

bool mode_on(int m, const ContextDesc& d) {
    switch (m) {
        case kModeShare: return d.share_k > 1;
        case kModeTerm: return d.min_trans > 0.f;
        case kModeSeparate: return d.separate;
        case kModeOcc: return d.occ.set;
        default: return d.cgrid.set;
    }
}

// "name (setter, parameters)" with `between` behind the name; a grid names its resolution only where it is the mode that refuses
std::string mode_text(int m, const ContextDesc& d, const char* between, bool refusing) {
    std::string s = std::string(kModeTable[m].name) + between + " (" + kModeTable[m].setter;
    if (m == kModeShare) s += ", k = " + std::to_string(d.share_k);
    if (m == kModeTerm) s += ", min_transmittance = " + std::to_string(d.min_trans);
    if (m == kModeOcc && refusing) s += ", " + times(d.occ.res);
    if (m == kModeBaked && refusing) s += ", " + times(d.cgrid.res);
    return s + ")";
}

// What a mode with kernels of its own cannot render, or nothing: everything but lean pinhole calls, and under the MFMA
// precisions a network whose shape or formulation has no such kernel.  What only a ray's own full passes can give is refused by
// name rather than changed in silence.
std::string mode_cannot(const Mode& mode, const ContextDesc& d, const nwe_outputs& out, int precision, bool pinhole) {
    if (!pinhole) return mode.no_rays;
    nwe_outputs rest = out;
    rest.struct_bytes = 0; rest.rgb = rest.depth = rest.acc = nullptr; rest.flags = nullptr;
    const nwe_outputs none = {};
    if (std::memcmp(&rest, &none, sizeof(none)) != 0) return "only rgb / depth / acc / flags can be requested";
    if (precision != NWE_PREC_F32)
        // fine_only (baked coarse pass): with n_importance == 0 the call is the ordinary one
        for (int i = mode.fine_only ? 1 : 0; i < (d.ni > 0 ? 2 : 1); ++i) {
            const NetDesc& n = d.net[i];
            if (n.built[mode.variant]) continue;
            const std::string kind = mode.kind;
            return (n.form == kFormReference ? "a network packed unfolded (nwe_debug_set_fold(0)) has no " + kind + " MFMA kernel"
                                             : "no " + kind + " MFMA kernel was built for this network shape") + "; use NWE_PREC_F32";
        }
    if (mode.no_stamps && d.stamps) return std::string("a stamped launch (nwe_debug_set_stamps) has no ") + mode.kind + " kernel";
    return {};
}

Refusal check_modes(const ContextDesc& d, const nwe_outputs& out, int precision, bool pinhole) {
    for (int m = 0; m < kModes; ++m) {
        const Mode& mode = kModeTable[m];
        if (!mode_on(m, d) || (mode.mfma_only && precision == NWE_PREC_F32)) continue;
        const auto opener = [&] { return mode_text(m, d, mode.is_on, true) + ": "; };
        for (const Exclusion& x : kExclusions)
            if (x.mode == m && mode_on(x.other, d))
                return unsupported(opener() + mode.it_is + " not built together with " + mode_text(x.other, d, "", false) + x.because + "; " + x.remedy);
        std::string cannot;
        if (mode.kind) cannot = mode_cannot(mode, d, out, precision, pinhole);
        else if (d.ni > 0 && d.net[0].form != d.net[1].form)   // separate passes
            cannot = "coarse and fine networks must be packed in the same formulation (nwe_debug_set_fold); use NWE_PREC_F32";
        if (!cannot.empty()) return unsupported(opener() + cannot + mode.off);
    }
    return {};
}

}  // namespace

Refusal check_precision(int precision) {
    if (precision != NWE_PREC_F16X3 && precision != NWE_PREC_F16X1 && precision != NWE_PREC_F32) return invalid("unknown precision");
    return {};
}

Refusal no_mfma_kernel() {
    return unsupported("no MFMA kernel for this network shape (have widths 128 and 256 with depth 6 or 8 and the skip after layer 4, or depth 4 without, "
                       "63 + 27 or, without view directions, 63 inputs); use NWE_PREC_F32");
}

Refusal check_on_device(bool have_device) {
    if (!have_device) return state("needs a device context");
    return {};
}

Refusal check_ready(const ContextDesc* d, const nwe_outputs* out, int precision, bool pinhole, bool planning) {
    if (!d || !out) return invalid("null context or outputs");
    if (out->struct_bytes != sizeof(nwe_outputs))
        return invalid("nwe_outputs.struct_bytes != sizeof(nwe_outputs): the caller was built against another version of include/nwe.h");
    if (d->host_only && !planning) return state("host-only context cannot render");
    if (d->ns <= 0) return state("nwe_set_sampling has not been called");
    const NetDesc &nc = d->net[0], &nf = d->net[1];
    if (!nc.set) return state("coarse network not set");
    if (d->ni > 0 && !nf.set) return state("fine network not set but n_importance > 0");
    if (Refusal r = check_precision(precision)) return r;
    if (d->ni > 0 && (nc.in_dir == 0) != (nf.in_dir == 0))
        return state("coarse and fine networks must both have, or both lack, view directions");
    // one Embedding serves both networks in the reference (handler.py:93-103) and one gamma(d) per ray both passes here
    if (d->ni > 0 && (nc.in_xyz != nf.in_xyz || nc.in_dir != nf.in_dir))
        return state("coarse and fine networks must share their encodings: in_xyz " + std::to_string(nc.in_xyz) + " / " + std::to_string(nf.in_xyz) +
                     ", in_dir " + std::to_string(nc.in_dir) + " / " + std::to_string(nf.in_dir) + " (coarse / fine)");
    if (out->feat_map) {
        if (d->ni <= 0 || nf.in_dir == 0)
            return invalid("feat_map is the fine pass's view-layer output: it needs n_importance > 0 and networks with view directions");
        if (precision != NWE_PREC_F32) return unsupported("feat_map (endpoint_feat) is computed by the NWE_PREC_F32 kernel only");
    }
    if (precision != NWE_PREC_F32) {
        // a baked coarse pass (nwe_set_coarse_grid) runs no kernel of the coarse network: its shape is not constrained
        const bool coarse_runs = !(d->cgrid.set && d->ni > 0);
        if ((coarse_runs && !nc.mfma_ok) || (d->ni > 0 && !nf.mfma_ok)) return no_mfma_kernel();
    }
    return check_modes(*d, *out, precision, pinhole);
}

Refusal check_camera(const Camera& m, CameraOf entry) {
    if (!m.c2w || m.n_poses < 1 || m.H < 1 || m.W < 1 || m.row_begin < 0 || m.row_end > m.H || m.row_begin > m.row_end)
        return invalid(entry == kCameraOfTiled ? "bad pose / image" : "bad pose / image / row range");
    if (!(m.fx != 0.f) || !(m.fy != 0.f)) return invalid("fx and fy must be non-zero");
    if (m.far < m.near)
        return invalid(entry == kCameraOfCreateRays ? "far < near: nwe_render_rays needs near <= far on every ray"
                                                    : "far < near: the sorted merge of the fine pass needs ascending depths");
    return {};
}

Refusal check_ray_count(int64_t n_rays, bool ray_list, bool null_rays) {
    if (!ray_list) return n_rays > INT32_MAX ? invalid("more than 2^31 - 1 rays in one call") : Refusal{};
    if (n_rays < 0 || n_rays > INT32_MAX || (null_rays && n_rays > 0)) return invalid("bad rays (null, or more than 2^31 - 1)");
    return {};
}

Refusal check_network(bool null_args, int which, int depth, int width, int in_xyz, int in_dir, int output_ch, bool view_dirs,
                      const float* const* w, const float* const* b) {
    if (null_args) return invalid("null argument");
    if (which != NWE_NET_COARSE && which != NWE_NET_FINE) return invalid("which must be 0 or 1");
    if (depth < 1 || depth > kMaxDepth) return unsupported("depth must be in 1..16");
    if (width < 2 || width > 256 || width % 2) return unsupported("width must be even and <= 256");
    const bool bad_xyz = in_xyz < 3 || in_xyz > 93 || (in_xyz - 3) % 6;
    if (view_dirs) {
        if (bad_xyz || in_dir < 3 || in_dir > 63 || (in_dir - 3) % 6)
            return unsupported("encoded widths must be 3 + 6*num_freqs (xyz <= 93, dir <= 63)");
    } else {
        if (bad_xyz) return unsupported("encoded width must be 3 + 6*num_freqs (<= 93)");
        if (output_ch < 4 || output_ch > 256) return unsupported("output_ch must be in 4..256 (rgb_raw, sigma_raw, ignored rest)");
    }
    for (int i = 0; i < (view_dirs ? depth + 4 : depth + 1); ++i)
        if (!w[i] || !b[i]) return invalid("null weight or bias pointer");
    return {};
}

Refusal check_sampling(bool null_ctx, const float* t_vals, const float* one_minus_t, int n_samples, const float* u, int n_importance) {
    if (null_ctx || !t_vals || !one_minus_t) return invalid("null argument");
    if (n_samples < 2 || n_samples > kMaxSamples) return unsupported("n_samples must be in 2..128");
    if (n_importance < 0 || n_importance > kMaxImportance) return unsupported("n_importance must be in 0..256");
    if (n_importance > 0 && (!u || n_samples < 3)) return invalid("importance sampling needs u and n_samples >= 3");
    return {};
}

Refusal check_early_termination(float min_transmittance) {
    if (!(min_transmittance >= 0.f && min_transmittance < 1.f)) return invalid("min_transmittance must be in [0, 1) (0 = off)");
    return {};
}

Refusal check_shared_coarse(int k) {
    if (k < 1 || k > 16) return invalid("shared_coarse k must be in 1..16 (1 = off)");
    return {};
}

Refusal check_separate_passes(int on) {
    if (on != 0 && on != 1) return invalid("separate_passes must be 0 or 1 (0 = off)");
    return {};
}

Refusal check_query(const ContextDesc* d, int which, const float* points, int64_t n_points, const float* dirs, int64_t points_per_dir,
                    int precision, const nwe_point_outputs* out) {
    if (Refusal r = check_on_device(d && !d->host_only)) return r;
    if (!out) return invalid("null outputs");
    if (out->struct_bytes != sizeof(nwe_point_outputs))
        return invalid("nwe_point_outputs.struct_bytes != sizeof(nwe_point_outputs): the caller was built against another version of include/nwe.h");
    if (which != NWE_NET_COARSE && which != NWE_NET_FINE) return invalid("which must be 0 or 1");
    if (n_points < 0 || n_points > INT32_MAX) return invalid("bad n_points (negative, or more than 2^31 - 1)");
    if (points_per_dir < 1) return invalid("points_per_dir must be at least 1");
    if (!points && n_points > 0) return invalid("null points");
    if (!out->raw && !out->sigma) return invalid("neither raw nor sigma requested");
    if (Refusal r = check_precision(precision)) return r;
    const NetDesc& net = d->net[which];
    if (!net.set) return state(which == NWE_NET_COARSE ? "coarse network not set" : "fine network not set");
    if (net.in_dir == 0 && dirs) return invalid("the network takes no view directions (nwe_set_network_no_view_dirs): dirs_dev must be null");
    if (net.in_dir != 0 && !dirs && out->raw)
        return invalid("raw output of a network with view directions needs dirs_dev (only sigma does not depend on the direction)");
    if (precision != NWE_PREC_F32 && !net.mfma_ok) return no_mfma_kernel();
    return {};
}

// occupancy: 1024^3 = 2^30 cells at the most, so a cell's index and the probes of a chunk stay below 2^31
const GridKind kOccupancyGrid = {"occupancy", 1024, false, "bits", "bits"};
const GridKind kCoarseGrid = {"coarse grid", 512, true, "sigma", "values"};
const GridKind kRadianceGrid = {"radiance grid", 512, true, "rows", "rows"};

Refusal check_grid_box(const GridKind& kind, const float* lo, const float* hi, const int* res) {
    const std::string word = std::string(kind.word) + ": ";
    if (!lo || !hi || !res) return invalid(word + "null lo, hi or resolution");
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || !std::isfinite(hi[i] - lo[i])) return invalid(word + "the box must be finite");
        if (!(lo[i] < hi[i])) return invalid(word + "the box must have lo < hi on every axis");
    }
    for (int i = 0; i < 3; ++i)
        if (res[i] < 1 || res[i] > kind.max_res)
            return invalid(word + "the resolution must be in 1.." + std::to_string(kind.max_res) + " on every axis");
    for (int i = 0; kind.finite_inv && i < 3; ++i)
        if (!std::isfinite((float)res[i] / (hi[i] - lo[i]))) return invalid(word + "the box must be finite (resolution / (hi - lo) is not, in fp32)");
    return {};
}

Refusal check_set_grid(const GridKind& kind, const float* lo, const float* hi, const int* res, const void* values, bool on_device, bool host_only) {
    if (Refusal r = check_grid_box(kind, lo, hi, res)) return r;
    if (!values) return invalid(std::string(kind.word) + ": null " + kind.values);
    if (on_device && host_only) return invalid(std::string(kind.word) + ": a host-only context takes its " + kind.from_host + " from the host");
    return {};
}

Refusal check_build_occupancy(const ContextDesc* d, const float* lo, const float* hi, const int* res, int probes, float threshold, int dilate,
                              int precision) {
    if (Refusal r = check_on_device(d && !d->host_only)) return r;
    if (Refusal r = check_grid_box(kOccupancyGrid, lo, hi, res)) return r;
    if (probes < 1 || probes > 4) return invalid("occupancy: probes must be in 1..4");
    if (dilate < 0 || dilate > 2) return invalid("occupancy: dilate must be in 0..2");
    if (threshold != threshold) return invalid("occupancy: the threshold must not be NaN");
    if (Refusal r = check_precision(precision)) return r;
    if (!d->net[0].set && !d->net[1].set) return state("occupancy: no network is set");
    for (const NetDesc& n : d->net)
        if (n.set && precision != NWE_PREC_F32 && !n.mfma_ok) return no_mfma_kernel();
    return {};
}

Refusal check_bake_coarse_grid(const ContextDesc* d, const float* lo, const float* hi, const int* res, int precision) {
    if (Refusal r = check_on_device(d && !d->host_only)) return r;
    if (Refusal r = check_grid_box(kCoarseGrid, lo, hi, res)) return r;
    if (Refusal r = check_precision(precision)) return r;
    const NetDesc& n = d->net[NWE_NET_COARSE];
    if (!n.set) return state("coarse grid: the coarse network is not set");
    if (precision != NWE_PREC_F32 && !n.mfma_ok) return no_mfma_kernel();
    return {};
}

Refusal check_bake_radiance_grid(const ContextDesc* d, const float* lo, const float* hi, const int* res, int which, const float* dir3,
                                 int precision) {
    if (Refusal r = check_on_device(d && !d->host_only)) return r;
    if (Refusal r = check_grid_box(kRadianceGrid, lo, hi, res)) return r;
    if (which != NWE_NET_COARSE && which != NWE_NET_FINE) return invalid("which must be 0 or 1");
    if (Refusal r = check_precision(precision)) return r;
    const NetDesc& n = d->net[which];
    if (!n.set) return state(which == NWE_NET_COARSE ? "radiance grid: the coarse network is not set" : "radiance grid: the fine network is not set");
    if (n.in_dir == 0 && dir3) return invalid("the network takes no view directions (nwe_set_network_no_view_dirs): dir3_host must be null");
    if (n.in_dir != 0 && !dir3) return invalid("radiance grid: the rows of a network with view directions need dir3_host");
    if (precision != NWE_PREC_F32 && !n.mfma_ok) return no_mfma_kernel();
    return {};
}

Refusal check_render_grid(const ContextDesc* d, const nwe_grid_outputs* out, const Camera& m) {
    if (!d) return invalid("null context");
    if (!out) return invalid("null outputs");
    if (out->struct_bytes != sizeof(nwe_grid_outputs))
        return invalid("nwe_grid_outputs.struct_bytes != sizeof(nwe_grid_outputs): the caller was built against another version of include/nwe.h");
    if (!out->rgb && !out->depth && !out->acc && !out->weights_coarse && !out->z_fine && !out->raw_fine)
        return invalid("none of rgb / depth / acc / weights_coarse / z_fine / raw_fine requested");
    if (Refusal r = check_camera(m)) return r;
    if (Refusal r = check_ray_count((int64_t)m.n_poses * (m.row_end - m.row_begin) * m.W, false)) return r;
    if (!d->rgrid.set) return state("radiance grid: no grid is set (nwe_set_radiance_grid, nwe_bake_radiance_grid)");
    if (d->ns <= 0) return state("nwe_set_sampling has not been called");
    return check_on_device(!d->host_only);
}

Refusal check_render_sparse(const ContextDesc* d, const nwe_sparse_outputs* out, const Camera& m, int which, int precision, float min_weight,
                            int dilate) {
    if (!d) return invalid("null context");
    if (!out) return invalid("null outputs");
    if (out->struct_bytes != sizeof(nwe_sparse_outputs))
        return invalid("nwe_sparse_outputs.struct_bytes != sizeof(nwe_sparse_outputs): the caller was built against another version of include/nwe.h");
    if (!out->rgb && !out->depth && !out->acc && !out->weights_coarse && !out->z_fine && !out->weights_grid && !out->selected && !out->raw_fine)
        return invalid("none of rgb / depth / acc / weights_coarse / z_fine / weights_grid / selected / raw_fine requested");
    if (Refusal r = check_camera(m)) return r;
    if (Refusal r = check_ray_count((int64_t)m.n_poses * (m.row_end - m.row_begin) * m.W, false)) return r;
    if (which != NWE_NET_COARSE && which != NWE_NET_FINE) return invalid("which must be 0 or 1");
    if (Refusal r = check_precision(precision)) return r;
    if (min_weight != min_weight) return invalid("sparse frame: min_weight must not be NaN");
    if (dilate < 0 || dilate > kSparseMaxDilate) return invalid("sparse frame: dilate must be in 0..8");
    if (!d->rgrid.set) return state("sparse frame: no radiance grid is set (nwe_set_radiance_grid, nwe_bake_radiance_grid)");
    if (d->ns <= 0) return state("nwe_set_sampling has not been called");
    const NetDesc& net = d->net[which];
    if (!net.set) return state(which == NWE_NET_COARSE ? "sparse frame: the coarse network is not set" : "sparse frame: the fine network is not set");
    if (Refusal r = check_on_device(!d->host_only)) return r;
    if (precision != NWE_PREC_F32 && !net.mfma_ok) return no_mfma_kernel();
    return {};
}

// Everything both adaptive calls refuse behind their outputs; levels: null for nwe_render_adaptive, which has none.
static Refusal check_adaptive_call(const ContextDesc* d, const Camera& m, int precision, int k, const int* levels, float tol_rgb, float tol_depth) {
    if (Refusal r = check_camera(m)) return r;
    const int64_t n_rays = (int64_t)m.n_poses * (m.row_end - m.row_begin) * m.W;
    if (Refusal r = check_ray_count(n_rays, false)) return r;
    if (n_rays > kAdaptiveMaxRays) return invalid("adaptive frame: more than 2^24 rays in one call");
    if (k < 1 || k > kAdaptiveMaxK) return invalid("adaptive frame: k must be in 1..64");
    if (levels && !adaptive_levels_ok(k, *levels)) return invalid("adaptive frame: levels must be in 1..4 and k * 2^(levels - 1) at most 64");
    if (tol_rgb != tol_rgb || tol_depth != tol_depth) return invalid("adaptive frame: the tolerances must not be NaN");
    if (Refusal r = check_precision(precision)) return r;
    // the render launches are nwe_render_rays launches with lean outputs: what that call refuses of the context, in its words
    static float somewhere;
    nwe_outputs lean = {};
    lean.struct_bytes = sizeof(nwe_outputs);
    lean.rgb = &somewhere;
    if (Refusal r = check_ready(d, &lean, precision, false, true)) return r;
    if (d->host_only) return state("host-only context cannot render");
    return {};
}

Refusal check_adaptive(const ContextDesc* d, const nwe_adaptive_outputs* out, const Camera& m, int precision, int k, float tol_rgb,
                       float tol_depth) {
    if (!d) return invalid("null context");
    if (!out) return invalid("null outputs");
    if (out->struct_bytes != sizeof(nwe_adaptive_outputs))
        return invalid("nwe_adaptive_outputs.struct_bytes != sizeof(nwe_adaptive_outputs): the caller was built against another version of include/nwe.h");
    if (!out->rgb && !out->depth && !out->acc) return invalid("none of rgb / depth / acc requested");
    return check_adaptive_call(d, m, precision, k, nullptr, tol_rgb, tol_depth);
}

Refusal check_adaptive_levels(const ContextDesc* d, const nwe_adaptive_levels_outputs* out, const Camera& m, int precision, int k, int levels,
                              float tol_rgb, float tol_depth) {
    if (!d) return invalid("null context");
    if (!out) return invalid("null outputs");
    if (out->struct_bytes != sizeof(nwe_adaptive_levels_outputs))
        return invalid("nwe_adaptive_levels_outputs.struct_bytes != sizeof(nwe_adaptive_levels_outputs): the caller was built against another version of include/nwe.h");
    if (!out->rgb && !out->depth && !out->acc) return invalid("none of rgb / depth / acc requested");
    return check_adaptive_call(d, m, precision, k, &levels, tol_rgb, tol_depth);
}

Refusal check_adaptive_pixel_lists(int on) {
    if (on != 0 && on != 1) return invalid("adaptive_pixel_lists must be 0 or 1 (0 = off)");
    return {};
}

Refusal check_pixels(const ContextDesc* d, const nwe_pixel_outputs* out, const Camera& m, int64_t n_pixels, bool null_pixels, int precision) {
    if (!d) return invalid("null context");
    if (!out) return invalid("null outputs");
    if (out->struct_bytes != sizeof(nwe_pixel_outputs))
        return invalid("nwe_pixel_outputs.struct_bytes != sizeof(nwe_pixel_outputs): the caller was built against another version of include/nwe.h");
    if (!out->rgb && !out->depth && !out->acc) return invalid("none of rgb / depth / acc requested");
    if (Refusal r = check_camera(m)) return r;
    if (Refusal r = check_ray_count((int64_t)m.n_poses * (m.row_end - m.row_begin) * m.W, false)) return r;
    if (n_pixels < 0 || n_pixels > INT32_MAX || (null_pixels && n_pixels > 0)) return invalid("bad pixels (null, a negative count, or more than 2^31 - 1)");
    if (Refusal r = check_precision(precision)) return r;
    // the launch is an nwe_render_rays launch with lean outputs, or stands in for one: what that call refuses of the context, in its words
    static float somewhere;
    nwe_outputs lean = {};
    lean.struct_bytes = sizeof(nwe_outputs);
    lean.rgb = &somewhere;
    if (Refusal r = check_ready(d, &lean, precision, false, true)) return r;
    if (d->host_only) return state("host-only context cannot render");
    return {};
}

bool pixel_list_path(const ContextDesc& d, int precision) {
    if (precision == NWE_PREC_F32 || d.separate || d.stamps) return false;
    const NetDesc &nc = d.net[0], &nf = d.net[1];
    if (!nc.set || !nc.mfma_ok || !nc.built[kVariantList]) return false;
    if (d.ni > 0 && (!nf.set || !nf.mfma_ok || !nf.built[kVariantList] || nf.D != nc.D || nf.W != nc.W || nf.skip != nc.skip || nf.form != nc.form))
        return false;
    return true;
}

}  // namespace nwe
