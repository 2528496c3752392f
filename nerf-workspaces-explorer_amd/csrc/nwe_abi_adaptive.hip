// C ABI of libnwe_hip.so (include/nwe.h), the adaptive frames: nwe_render_adaptive and nwe_render_adaptive_levels, their reports and
// their lattice calls.  Host code only: the kernels are in nwe_adaptive.hip and nwe_adaptive_levels.hip, the render launches are the
// context's own (render_ray_list, render_pixel_list).
#include "nwe_ctx.h"

namespace {

// One render launch of the call: the rays of the first n pixels of the list, rendered into the compact outputs from `first` on, the
// flags into the scratch's word.  rgb, depth and acc are always rendered: the cells are judged on all of them.
// Under nwe_set_adaptive_pixel_lists, where the list kernels can serve the call (pixel_list_path), the list itself is the launch's
// input - it is in nwe_render's ray order, which is what the list kernels read - and no ray table is written: the same bits.
int render_list(nwe_ctx* c, const ContextDesc& desc, const RenderArgs& cam, const AdaptiveFrame& f, const AdaptivePlan& p, float* rays, uint32_t* flags,
                int64_t first, int n, int precision, hipStream_t stream) {
    nwe_outputs o = {};
    o.struct_bytes = sizeof(nwe_outputs);
    o.rgb = f.c_rgb + first * 3; o.depth = f.c_depth + first; o.acc = f.c_acc + first;
    o.flags = flags;
    if (c->adaptive_lists && pixel_list_path(desc, precision)) {
        TRY(render_pixel_list(c, desc, cam, p.n_poses, f.list, n, precision, o, stream));
        c->pixels_n = n; c->pixels_path = 1;
        return NWE_OK;
    }
    launch_adaptive_rays(cam, f, n, p.cols, rays, stream);
    HIPCHK(c, hipGetLastError());
    return render_ray_list(c, desc, rays, n, precision, o, false, stream);
}

int render_adaptive(nwe_ctx* c, const Camera& m, int precision, int k, float tol_rgb, float tol_depth, const nwe_adaptive_outputs* out, hipStream_t stream) {
    const MaybeContext desc(c);
    CHECK(c, check_adaptive(desc.p, out, m, precision, k, tol_rgb, tol_depth));
    const int rows = m.row_end - m.row_begin;
    if ((int64_t)m.n_poses * rows * m.W == 0) return NWE_OK;
    ON_DEVICE(c);
    const AdaptivePlan p = plan_adaptive(m.n_poses, rows, m.W, k, c->net[0].in_dir == 0 ? 8 : 11);
    Slot& slot = c->adaptive_slot;   // not a slot of the render ring: the two render launches take theirs
    TRY(prepare_slot(c, slot));
    c->adaptive_ran = false;   // from here on the slot describes no call until this one has run
    TRY(upload_poses(c, slot, m.c2w, m.n_poses, stream));
    HIPCHK(c, c->d_adaptive_scratch.reserve((size_t)p.bytes));   // grow-only; the call is synchronous, so nothing still reads it
    if (!c->adaptive_word) HIPCHK(c, hipHostMalloc(&c->adaptive_word.h, sizeof(uint32_t), hipHostMallocDefault));
    const RenderArgs cam = camera_args(m, slot.poses.get());   // what the ray kernel reads: the camera alone
    uint8_t* const base = c->d_adaptive_scratch.get();
    AdaptiveFrame f = {};
    f.h = p.h; f.w = p.w; f.n_poses = m.n_poses; f.pixels = (int)p.pixels; f.lattice = (int)p.lattice;
    f.tol_rgb = tol_rgb; f.tol_depth = tol_depth;
    f.list = reinterpret_cast<int32_t*>(base + p.at_list);
    f.c_rgb = reinterpret_cast<float*>(base + p.at_rgb); f.c_depth = reinterpret_cast<float*>(base + p.at_depth);
    f.c_acc = reinterpret_cast<float*>(base + p.at_acc);
    f.kinds = base + p.at_kind; f.counts = reinterpret_cast<uint32_t*>(base + p.at_counts); f.busy = base + p.at_busy;
    uint32_t* const render_flags = reinterpret_cast<uint32_t*>(base + p.at_flags);   // what the two render launches raise, masked by compose
    f.total = reinterpret_cast<uint32_t*>(base + p.at_total); f.render_flags = render_flags;
    f.rgb = out->rgb; f.depth = out->depth; f.acc = out->acc; f.kind = out->kind; f.flags = out->flags;
    float* const rays = reinterpret_cast<float*>(base + p.at_rays);
    volatile uint32_t* const word = static_cast<uint32_t*>(c->adaptive_word.h);
    int64_t rendered = 0;
    const int rc = record_launch(c, slot, stream, [&]() -> int {
        HIPCHK(c, hipMemsetAsync(render_flags, 0, sizeof(uint32_t), stream));
        launch_adaptive_lattice(f, stream);
        TRY(render_list(c, desc.d, cam, f, p, rays, render_flags, 0, f.lattice, precision, stream));
        launch_adaptive_classify(f, stream);
        HIPCHK(c, hipGetLastError());
        // the one read-back of the call: the second render launch needs its ray count on the host
        HIPCHK(c, hipMemcpyAsync(c->adaptive_word.h, f.total, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(c, hipStreamSynchronize(stream));
        rendered = *word;
        if (rendered > p.pixels - p.lattice) return fail(c, NWE_ERR_HIP, "adaptive frame: the rendered pixel count is out of range");
        if (rendered > 0) TRY(render_list(c, desc.d, cam, f, p, rays, render_flags, p.lattice, (int)rendered, precision, stream));   // no busy cell: one launch
        launch_adaptive_compose(f, stream);
        return NWE_OK;
    });
    // nothing of the call may still run, or read the scratch, when it returns; nor may anything of one that failed half way
    const hipError_t waited = hipStreamSynchronize(stream);
    if (rc) return rc;
    HIPCHK(c, waited);
    c->adaptive_counts[0] = p.pixels; c->adaptive_counts[1] = p.lattice; c->adaptive_counts[2] = rendered;
    c->adaptive_counts[3] = p.pixels - p.lattice - rendered;
    c->adaptive_ran = true;
    return NWE_OK;
}

// nwe_render_adaptive_levels: pass 0, then per level classify, one read-back of two words and the level's render pass, until a
// level has no busy cell; compose.  The render launches are render_list's, on a frame that names the list and the compact outputs.
int render_adaptive_levels(nwe_ctx* c, const Camera& m, int precision, int k, int levels, float tol_rgb, float tol_depth,
                           const nwe_adaptive_levels_outputs* out, hipStream_t stream) {
    const MaybeContext desc(c);
    CHECK(c, check_adaptive_levels(desc.p, out, m, precision, k, levels, tol_rgb, tol_depth));
    const int rows = m.row_end - m.row_begin;
    if ((int64_t)m.n_poses * rows * m.W == 0) return NWE_OK;
    ON_DEVICE(c);
    const AdaptiveLevelsPlan p = plan_adaptive_levels(m.n_poses, rows, m.W, k, levels, c->net[0].in_dir == 0 ? 8 : 11);
    Slot& slot = c->adaptive_levels_slot;
    TRY(prepare_slot(c, slot));
    c->adaptive_levels_ran = false;   // from here on the slot describes no call until this one has run
    TRY(upload_poses(c, slot, m.c2w, m.n_poses, stream));
    HIPCHK(c, c->d_adaptive_scratch.reserve((size_t)p.bytes));   // grow-only; both adaptive calls are synchronous, so nothing still reads it
    constexpr int kWords = 2 + kAdaptiveMaxLevels;   // a read-back's two words, then the interpolated counts
    if (!c->adaptive_levels_words) HIPCHK(c, hipHostMalloc(&c->adaptive_levels_words.h, kWords * sizeof(uint32_t), hipHostMallocDefault));
    const RenderArgs cam = camera_args(m, slot.poses.get());
    uint8_t* const base = c->d_adaptive_scratch.get();
    AdaptiveLevelsFrame f = {};
    for (int l = 0; l < levels; ++l) { f.h[l] = p.h[l]; f.w[l] = p.w[l]; f.state[l] = base + p.at_state[l]; }
    f.levels = levels; f.n_poses = m.n_poses; f.pixels = (int)p.pixels;
    f.tol_rgb = tol_rgb; f.tol_depth = tol_depth;
    f.list = reinterpret_cast<int32_t*>(base + p.at_list);
    f.c_rgb = reinterpret_cast<float*>(base + p.at_rgb); f.c_depth = reinterpret_cast<float*>(base + p.at_depth);
    f.c_acc = reinterpret_cast<float*>(base + p.at_acc);
    f.slot = reinterpret_cast<int32_t*>(base + p.at_slot); f.counts = reinterpret_cast<uint32_t*>(base + p.at_counts);
    f.words = reinterpret_cast<uint32_t*>(base + p.at_words); f.interp = reinterpret_cast<uint32_t*>(base + p.at_interp);
    uint32_t* const render_flags = reinterpret_cast<uint32_t*>(base + p.at_flags);
    f.render_flags = render_flags;
    f.rgb = out->rgb; f.depth = out->depth; f.acc = out->acc; f.kind = out->kind; f.level = out->level; f.flags = out->flags;
    for (int i = 0; i <= kAdaptiveMaxLevels; ++i) f.base[i] = INT32_MAX;
    float* const rays = reinterpret_cast<float*>(base + p.at_rays);
    // what render_list reads of the one-level call's frame and plan
    AdaptiveFrame rf = {};
    rf.list = f.list; rf.c_rgb = f.c_rgb; rf.c_depth = f.c_depth; rf.c_acc = f.c_acc;
    AdaptivePlan rp;
    rp.n_poses = p.n_poses; rp.cols = p.cols;
    volatile uint32_t* const word = static_cast<uint32_t*>(c->adaptive_levels_words.h);
    int64_t rendered[kAdaptiveMaxLevels] = {};
    int64_t done = 0;   // pixels rendered so far: the first slot of the next pass
    int launches = 0;
    const int rc = record_launch(c, slot, stream, [&]() -> int {
        HIPCHK(c, hipMemsetAsync(f.slot, 0xff, (size_t)p.pixels * sizeof(int32_t), stream));   // -1: not rendered
        HIPCHK(c, hipMemsetAsync(f.words, 0, (size_t)(p.at_flags + 4 - p.at_words), stream));    // words, interpolated counts, flag word
        launch_adaptive_levels_lattice(f, (int)p.lattice, stream);
        f.base[0] = 0;
        TRY(render_list(c, desc.d, cam, rf, rp, rays, render_flags, 0, (int)p.lattice, precision, stream));
        done = p.lattice; launches = 1;
        for (int l = 0; l < levels; ++l) {
            launch_adaptive_levels_classify(f, l, (int)done, stream);
            HIPCHK(c, hipGetLastError());
            f.classified = l + 1;
            // the level's read-back: the pixels of its render pass and its busy cells
            HIPCHK(c, hipMemcpyAsync(c->adaptive_levels_words.h, f.words + 2 * l, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIPCHK(c, hipStreamSynchronize(stream));
            const int64_t next = word[0], busy = word[1];
            if (next > p.pass_max[l + 1] || next > p.pixels - done || busy > p.cells[l] || (busy == 0 && next != 0))
                return fail(c, NWE_ERR_HIP, "adaptive frame: a level's pixel or cell count is out of range");
            rendered[l] = next;
            f.base[l + 1] = (int)done;
            if (next > 0) {
                TRY(render_list(c, desc.d, cam, rf, rp, rays, render_flags, done, (int)next, precision, stream));
                done += next; ++launches;
            }
            if (busy == 0) break;   // every active cell is flat: nothing further to launch, classify or read back
        }
        launch_adaptive_levels_compose(f, stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(static_cast<uint32_t*>(c->adaptive_levels_words.h) + 2, f.interp, kAdaptiveMaxLevels * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, stream));   // rides on the wait that ends the call
        return NWE_OK;
    });
    // nothing of the call may still run, or read the scratch, when it returns; nor may anything of one that failed half way
    const hipError_t waited = hipStreamSynchronize(stream);
    if (rc) return rc;
    HIPCHK(c, waited);
    int64_t* const r = c->adaptive_levels_counts;
    r[0] = p.pixels; r[1] = p.lattice; r[2] = levels; r[3] = launches;
    int64_t interpolated = 0;
    for (int l = 0; l < levels; ++l) { r[4 + l] = rendered[l]; r[4 + levels + l] = word[2 + l]; interpolated += word[2 + l]; }
    if (done + interpolated != p.pixels) return fail(c, NWE_ERR_HIP, "adaptive frame: the interpolated pixel counts are out of range");
    c->adaptive_levels_ran = true;
    return NWE_OK;
}

}  // namespace

extern "C" {

int nwe_render_adaptive_levels(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
                               float far, int row_begin, int row_end, int precision, int k, int levels, float tol_rgb, float tol_depth,
                               const nwe_adaptive_levels_outputs* out, void* stream) {
    return render_adaptive_levels(c, Camera{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end}, precision, k, levels, tol_rgb,
                                  tol_depth, out, (hipStream_t)stream);
}

int nwe_last_adaptive_levels(nwe_ctx* c, int64_t* out, int cap, float* ms) {
    if (!c || !out) return NWE_ERR_INVALID;
    if (!c->adaptive_levels_ran) return NWE_ERR_STATE;
    const int n = 4 + 2 * (int)c->adaptive_levels_counts[2];
    if (cap < n) return NWE_ERR_INVALID;
    for (int i = 0; i < n; ++i) out[i] = c->adaptive_levels_counts[i];
    if (ms) {
        *ms = elapsed_ms(c, &c->adaptive_levels_slot, "nwe_last_adaptive_levels");
        if (*ms < 0.f) return NWE_ERR_HIP;
    }
    return NWE_OK;
}

int nwe_debug_adaptive_levels_lattice(int first, int last_excl, int k, int levels, int level, int32_t* out, int cap) {
    return adaptive_levels_lattice(first, last_excl, k, levels, level, out, cap);
}

int nwe_debug_adaptive_levels_plan(int n_poses, int rows, int width, int k, int levels, int ray_cols, int64_t* out, int cap) {
    if (n_poses < 1 || rows < 1 || width < 1 || (int64_t)n_poses * rows * width > kAdaptiveMaxRays || !adaptive_levels_ok(k, levels) ||
        (ray_cols != 8 && ray_cols != 11) || !out || cap < 5 + 2 * levels)
        return -1;
    const AdaptiveLevelsPlan p = plan_adaptive_levels(n_poses, rows, width, k, levels, ray_cols);
    int n = 0;
    out[n++] = p.pixels; out[n++] = p.lattice; out[n++] = p.list; out[n++] = p.bytes;
    for (int l = 0; l < levels; ++l) out[n++] = p.cells[l];
    for (int i = 0; i <= levels; ++i) out[n++] = p.pass_max[i];
    return n;
}


int nwe_render_adaptive(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near, float far,
                        int row_begin, int row_end, int precision, int k, float tol_rgb, float tol_depth, const nwe_adaptive_outputs* out,
                        void* stream) {
    return render_adaptive(c, Camera{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end}, precision, k, tol_rgb, tol_depth, out,
                           (hipStream_t)stream);
}

int nwe_last_adaptive(nwe_ctx* c, int64_t* out4, float* ms) {
    if (!c || !out4) return NWE_ERR_INVALID;
    if (!c->adaptive_ran) return NWE_ERR_STATE;
    for (int i = 0; i < 4; ++i) out4[i] = c->adaptive_counts[i];
    if (ms) {
        *ms = elapsed_ms(c, &c->adaptive_slot, "nwe_last_adaptive");
        if (*ms < 0.f) return NWE_ERR_HIP;
    }
    return NWE_OK;
}

int nwe_debug_adaptive_lattice(int first, int last_excl, int k, int32_t* out, int cap) { return adaptive_lattice(first, last_excl, k, out, cap); }

}  // extern "C"
