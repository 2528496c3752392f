// fp32 render kernel (NWE_PREC_F32): the whole ray pipeline of
// nerf/inference/nerf_replica_inference_handler.py:203-277 with the MLP GEMMs as fp32 FMA chains on
// the vector ALU.  Any layer shape with width <= 256.  It is the on-device reference the MFMA kernel
// is compared with at full frame size (where the CPU oracle needs minutes), and the path for network
// shapes the MFMA kernel has no instantiation for.
//
// One 256-thread workgroup owns a packet of 16 rays and walks their samples in lock step: thread n is
// output neuron n of the current layer and keeps 16 accumulators (one per ray of the packet), the
// layer input lives in LDS as [k][16] so one ds_read_b128 broadcast feeds 4 FMAs.  Weights are read
// transposed ([k][n], coalesced, L2-resident).
#include "nwe_kernel_f32_layers.h"   // dense16, encode16: shared with the occupancy kernel (nwe_kernel_f32_occ.hip)

namespace nwe {

// TERM: early ray termination (include/nwe.h, nwe_set_early_termination; the rule and its argument: render_mfma_kernel,
// nwe_mfma_render.h).  The 16 owners vote at the top of every sample iteration of the pass that produces the outputs, on a
// barrier of its own that all 256 threads pass, and the workgroup leaves the loop with no lag: min(S, M) iterations for the
// largest stop index M of its rays.  One atomic per workgroup counts the ray evaluations.
// SHARE: the coarse pass shared by k x k pixel blocks (nwe_set_shared_coarse; render_mfma_kernel, nwe_mfma_render.h): the
// producer launch walks the representative rays through pass 0 and writes their weights to a.share_w, the consumer launch
// fills s_w from its rays' representatives and runs the fine pass.
template <bool TERM, bool SHARE = false>
__global__ void __launch_bounds__(256) render_f32_kernel(RenderArgs a, NetF32 nc, NetF32 nf) {
    static_assert(!(TERM && SHARE), "shared coarse pass: not with early termination");
    constexpr bool OCC = false;
    const OccGrid* const occ = nullptr;
#include "nwe_kernel_f32_body.h"
}

void launch_render_f32(const RenderArgs& a, const NetF32& nc, const NetF32& nf, hipStream_t stream) {
    const int64_t blocks = (a.n_rays + kRP - 1) / kRP;
    if (a.share != kShareOff) hipLaunchKernelGGL((render_f32_kernel<false, true>), dim3((unsigned)blocks), dim3(256), 0, stream, a, nc, nf);
    else if (a.min_trans > 0.f && a.evals) hipLaunchKernelGGL(render_f32_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a, nc, nf);
    else hipLaunchKernelGGL(render_f32_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a, nc, nf);
}

// The point query of the fp32 path (include/nwe.h: nwe_query_points; the MFMA one: nwe_mfma_query.h): run_network of
// nerf/models/model_utils.py:13-30 in the arithmetic of render_f32_kernel's evaluation block - encode16 and dense16, the trunk
// with its skip, then the heads - for any shape of the fp32 domain.  A workgroup owns a.steps x 16 consecutive points and
// walks them 16 per step: the first 16 threads own one point each, gamma(d) is encoded again every step (the direction
// belongs to the point), a thread past n_points takes the last point and stores nothing, and a step that lies wholly past
// n_points is not run (uniform: it depends on the block, the step and n_points).  With raw == null the evaluation is still the
// full one and the colour is dropped.  VIEW: the network has view directions (net.in_dir != 0), else the one output layer.
template <bool VIEW>
__global__ void __launch_bounds__(256) query_f32_kernel(QueryArgs a, NetF32 net) {
    __shared__ __attribute__((aligned(16))) float s_gx[96 * kRP];
    __shared__ __attribute__((aligned(16))) float s_gd[64 * kRP];
    __shared__ __attribute__((aligned(16))) float s_ha[256 * kRP];
    __shared__ __attribute__((aligned(16))) float s_hb[256 * kRP];
    __shared__ __attribute__((aligned(16))) float s_pt[3 * kRP];
    __shared__ __attribute__((aligned(16))) float s_dir[3 * kRP];
    __shared__ __attribute__((aligned(16))) float s_raw[4 * kRP];
    static_assert(kQueryPacketF32 == kRP, "a step is one packet of the fp32 kernels");
    const int tid = threadIdx.x;
    const bool owner = tid < kRP;
    const int n = a.n_points;
    uint32_t flags = 0;
    for (int step = 0; step < a.steps; ++step) {
        const int64_t first = ((int64_t)blockIdx.x * a.steps + step) * kRP;
        if (first >= n) break;
#include "nwe_kernel_f32_query_step.h"   // the step, shared as text with query_f32_counted_kernel (nwe_kernel_f32_counted.hip)
    }
    if (flags && a.flags) atomicOr(a.flags, flags);
}

void launch_query_f32(const QueryArgs& a_in, const NetF32& net, int forced_steps, int cus, hipStream_t stream) {
    if (a_in.n_points <= 0) return;
    QueryArgs a = a_in;
    const int64_t packets = ((int64_t)a.n_points + kRP - 1) / kRP;
    a.steps = query_steps(packets, forced_steps, cus);
    const dim3 grid((unsigned)((packets + a.steps - 1) / a.steps));
    if (net.in_dir != 0) hipLaunchKernelGGL(query_f32_kernel<true>, grid, dim3(256), 0, stream, a, net);
    else hipLaunchKernelGGL(query_f32_kernel<false>, grid, dim3(256), 0, stream, a, net);
}

}  // namespace nwe
