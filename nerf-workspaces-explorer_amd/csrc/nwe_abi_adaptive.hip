// C ABI of libnwe_hip.so (include/nwe.h), the adaptive frame: nwe_render_adaptive, its report and its lattice call.  Host code
// only: the kernels are in nwe_adaptive.hip, the render launches are the context's own (render_ray_list, nwe_abi.hip).
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

}  // namespace

extern "C" {

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
