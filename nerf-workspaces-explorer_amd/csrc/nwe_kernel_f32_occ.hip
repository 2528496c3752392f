// The occupancy kernel of the fp32 path, in a translation unit of its own: the code object of nwe_kernel_f32.hip keeps the
// kernels it had, descriptors included (tools/device_code_digest.py).
#include "nwe_kernel_f32_layers.h"

namespace nwe {

// OCC: the occupancy grid (include/nwe.h, nwe_set_occupancy; the MFMA kernels' version and its argument: nwe_mfma_render.h), in
// a kernel of its own name so that render_f32_kernel's instantiations keep theirs.  In both passes the 16 owners look up the
// cell of this iteration's point and the workgroup votes on a barrier of its own that all 256 threads pass
// (__syncthreads_and: uniform by construction).  If every live ray's sample lies in an empty cell the evaluation is left out -
// no barrier of the evaluation is entered, all threads alike - and the owners composite raw = (0, 0, 0, 0); otherwise the
// network runs and the owners in empty cells replace its four outputs by 0.  The group is this kernel's own: the 16
// consecutive rays of a workgroup (include/nwe.h states it for nwe_last_ray_evaluations).  One atomic per workgroup counts its live rays
// times the iterations it evaluated, both passes.
__global__ void __launch_bounds__(256) render_f32_occ_kernel(RenderArgs a, NetF32 nc, NetF32 nf) {
    constexpr bool TERM = false, SHARE = false, OCC = true;
    const OccGrid* const occ = a.occ;
#include "nwe_kernel_f32_body.h"
}

void launch_render_f32_occ(const RenderArgs& a, const NetF32& nc, const NetF32& nf, hipStream_t stream) {
    const int64_t blocks = (a.n_rays + kRP - 1) / kRP;
    hipLaunchKernelGGL(render_f32_occ_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a, nc, nf);
}

}  // namespace nwe
