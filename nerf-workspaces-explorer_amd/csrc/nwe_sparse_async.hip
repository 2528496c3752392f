// What nwe_render_sparse_async (include/nwe.h) adds to the four kernels of nwe_sparse.hip, which it launches unchanged: the tally of
// the selected samples, kept on the device.  A translation unit of its own: every other code object keeps the kernels it had.  The
// counted query kernels the call runs between emit and composite: nwe_mfma_query.h, nwe_kernel_f32_counted.hip.
#include "nwe_host.h"

namespace nwe {

// One thread: the chunk's selected samples (the scan's total) onto the call's tally.
__global__ void sparse_tally_kernel(const uint32_t* __restrict__ total, unsigned long long* __restrict__ tally) {
    atomicAdd(tally, (unsigned long long)*total);
}

void launch_sparse_tally(const SparseChunk& c, unsigned long long* tally, hipStream_t stream) {
    if (c.count <= 0) return;
    hipLaunchKernelGGL(sparse_tally_kernel, dim3(1), dim3(1), 0, stream, c.total, tally);
}

}  // namespace nwe
