// The counted point query of the fp32 path (nwe_render_sparse_async).  A translation unit of its own: every other code object
// keeps the kernels it had, byte for byte.
#include "nwe_kernel_f32_layers.h"   // dense16, encode16

namespace nwe {

// The counted form (nwe_render_sparse_async; query_mfma_counted_kernel, nwe_mfma_query.h): a.n_points is a capacity, the count a
// device word read once; the workgroup walks the packets blockIdx.x, + grid, + 2 grid, ... below n = min(*count, capacity) and
// returns before anything else if it has none.  The step is query_f32_kernel's, the same text.
template <bool VIEW>
__global__ void __launch_bounds__(256) query_f32_counted_kernel(QueryArgs a, NetF32 net, const uint32_t* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) float s_gx[96 * kRP];
    __shared__ __attribute__((aligned(16))) float s_gd[64 * kRP];
    __shared__ __attribute__((aligned(16))) float s_ha[256 * kRP];
    __shared__ __attribute__((aligned(16))) float s_hb[256 * kRP];
    __shared__ __attribute__((aligned(16))) float s_pt[3 * kRP];
    __shared__ __attribute__((aligned(16))) float s_dir[3 * kRP];
    __shared__ __attribute__((aligned(16))) float s_raw[4 * kRP];
    const uint32_t counted = *count;
    const int n = (int)(counted < (uint32_t)a.n_points ? counted : (uint32_t)a.n_points);
    if ((int64_t)blockIdx.x * kRP >= n) return;   // workgroup-uniform; no barrier has been met
    const int tid = threadIdx.x;
    const bool owner = tid < kRP;
    uint32_t flags = 0;
    for (int64_t packet = blockIdx.x;; packet += gridDim.x) {
        const int64_t first = packet * kRP;
        if (first >= n) break;   // workgroup-uniform
#include "nwe_kernel_f32_query_step.h"
    }
    if (flags && a.flags) atomicOr(a.flags, flags);
}

void launch_query_f32_counted(const QueryArgs& a_in, const uint32_t* count, const NetF32& net, int forced_steps, int cus, hipStream_t stream) {
    if (a_in.n_points <= 0) return;
    QueryArgs a = a_in;
    a.steps = 0;   // not read: the walk is strided over the grid
    const dim3 grid(query_counted_grid(a.n_points, kRP, forced_steps, cus));
    if (net.in_dir != 0) hipLaunchKernelGGL(query_f32_counted_kernel<true>, grid, dim3(256), 0, stream, a, net, count);
    else hipLaunchKernelGGL(query_f32_counted_kernel<false>, grid, dim3(256), 0, stream, a, net, count);
}

}  // namespace nwe
