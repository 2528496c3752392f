// C ABI of libnwe_hip.so (include/nwe.h), the pixel list: nwe_render_pixels, its report, and the switch that lets the adaptive frame
// render its lists the same way.  Host code and one small kernel: the list kernels are render_mfma_list_kernel (nwe_mfma_render.h), the
// ray table of the other path is written by the adaptive frame's `rays` kernel (nwe_adaptive.hip), and both launches are the
// context's own (render_pixel_list, render_ray_list: nwe_abi.hip).  Which path a call takes is nwe_check.cpp's decision.
#include "nwe_ctx.h"

namespace {

// The ray-table path: the list as load_ray may read it.  The list kernels clamp as they load; the `rays` kernel reads its list as
// it stands, so it is given this copy.  hi = the rays of the camera's own frame - 1.
__global__ void __launch_bounds__(256) clamp_pixels_kernel(const int32_t* __restrict__ in, int n, int hi, int32_t* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = min(max(in[t], 0), hi);
}

constexpr uint32_t kPixelFlags = NWE_FLAG_RGB | NWE_FLAG_DEPTH | NWE_FLAG_ACC;

int render_pixels(nwe_ctx* c, const Camera& m, const int32_t* pixels_dev, int64_t n_pixels, int precision, const nwe_pixel_outputs* out,
                  hipStream_t stream) {
    const MaybeContext desc(c);
    CHECK(c, check_pixels(desc.p, out, m, n_pixels, !pixels_dev, precision));
    if (n_pixels == 0) return NWE_OK;
    ON_DEVICE(c);
    const bool lists = pixel_list_path(desc.d, precision);
    // the slot the launch will take: its pose table serves the list kernels and the `rays` kernel alike
    RenderSlot& slot = c->render.next();
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, m.c2w, m.n_poses, stream));
    const RenderArgs cam = camera_args(m, slot.poses.get());
    nwe_outputs o = {};
    o.struct_bytes = sizeof(nwe_outputs);
    o.rgb = out->rgb; o.depth = out->depth; o.acc = out->acc; o.flags = out->flags;
    const int n = (int)n_pixels;
    if (lists) {
        TRY(render_pixel_list(c, desc.d, cam, m.n_poses, pixels_dev, n, precision, o, stream, kPixelFlags));
    } else {
        const int cols = c->net[0].in_dir == 0 ? 8 : 11;
        HIPCHK(c, slot.pixel_list.reserve((size_t)n));
        HIPCHK(c, slot.pixel_rays.reserve((size_t)n * cols));
        hipLaunchKernelGGL(clamp_pixels_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, pixels_dev, n, (int)(cam.n_rays - 1),
                           slot.pixel_list.get());
        AdaptiveFrame f = {};
        f.list = slot.pixel_list.get();
        launch_adaptive_rays(cam, f, n, cols, slot.pixel_rays.get(), stream);
        HIPCHK(c, hipGetLastError());
        TRY(render_ray_list(c, desc.d, slot.pixel_rays.get(), n, precision, o, false, stream, kPixelFlags));
    }
    c->pixels_n = n_pixels; c->pixels_path = lists ? 1 : 0;
    return NWE_OK;
}

}  // namespace

extern "C" {

int nwe_render_pixels(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near, float far,
                      int row_begin, int row_end, const int32_t* pixels_dev, int64_t n_pixels, int precision, const nwe_pixel_outputs* out,
                      void* stream) {
    return render_pixels(c, Camera{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end}, pixels_dev, n_pixels, precision, out,
                         (hipStream_t)stream);
}

int nwe_last_pixels(nwe_ctx* c, int64_t* n_pixels, int* path) {
    if (!c || !n_pixels || !path) return NWE_ERR_INVALID;
    if (c->pixels_path < 0) return NWE_ERR_STATE;
    *n_pixels = c->pixels_n; *path = c->pixels_path;
    return NWE_OK;
}

int nwe_set_adaptive_pixel_lists(nwe_ctx* c, int on) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_adaptive_pixel_lists(on));
    c->adaptive_lists = on;
    return NWE_OK;
}
int nwe_get_adaptive_pixel_lists(const nwe_ctx* c) { return c ? c->adaptive_lists : -1; }

int nwe_debug_pixels_path(const nwe_ctx* c, int precision) {
    if (!c || check_precision(precision)) return -1;
    return pixel_list_path(describe_context(c), precision) ? 1 : 0;
}

}  // extern "C"
