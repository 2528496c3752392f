// The point query on the MFMA path (include/nwe.h: nwe_query_points): run_network of nerf/models/model_utils.py:13-30 - points
// and view directions in, the raw network output out - as the packets loop of nwe_mfma_render_item.h with the renderer taken
// away.  No ray, no depth, no compositing, no sampler and no second network: what is left is the weight stream, gamma(x),
// gamma(d) and mlp_eval, used exactly as the render kernels use them (nwe_mfma_eval.h and nwe_mfma_stream.h are included, not
// edited), so a point evaluates to the bits a ray sample at the same position evaluates to.
#pragma once
#include "nwe_mfma_render.h"   // Shape, Walker, Frags, encode, mlp_eval, density_only_built, store_raw, bad

namespace nwe {

static_assert(kQueryPacket == kWaves * kRaysPerWave, "a step is one packet per wave: wave w owns points 32 w .. 32 w + 31 of it");

// LDS of a query workgroup: the two chunk buffers, ONE network's bias table (with the dot rows of the folded formulation), the
// three tail slots of the Walker and the waves' gamma(d) fragments.  Neither coarse-weight buffers nor sampling tables nor
// exchange buffers (Smem of nwe_mfma_render.h has them).
template <int W, int D>
struct QuerySmem {
    using S = Shape<W, D>;
    static constexpr int CHUNKS = 2 * S::CHUNK_BYTES;
    static constexpr int BOFF = CHUNKS;
    static constexpr int BIAS_BYTES = ((S::N_CHUNKS * 32 * 4 + 255) / 256) * 256;
    static constexpr int LOFF = BOFF + BIAS_BYTES;                                   // three tail slots of two tiles (Walker)
    static constexpr int GOFF = LOFF + 3 * 2 * kTileBytes;                           // gamma(d) fragments, (hi, lo) per k-step and wave
    static constexpr int TOTAL = GOFF + kWaves * 2 * S::KD * kTileBytes;
    static_assert(LOFF % 16 == 0 && GOFF % 16 == 0 && TOTAL <= 160 * 1024, "LDS budget");
};

// A 256-thread workgroup owns the contiguous run of a.steps x 128 points that starts at point item x a.steps x 128, item =
// blockIdx.x, and walks it one packet of 128 per step; all four waves share one weight stream.  One step is one sample iteration
// of the render kernels' packets plan: prime the stream (chunks 0 and 1), load the point, gamma(x) of p / 10, the barrier that
// publishes chunk 0, the first PD fragments, mlp_eval, the store.  What differs from the renderer:
//   * gamma(d) belongs to the point, not to a ray: every step each wave encodes its 32 directions again (see the write below);
//   * a lane past n_points takes the last point, computes along (its wave streams a quarter of every chunk and passes every
//     barrier) and stores nothing; a step whose 128 points all lie past n_points is not run: the test depends on item, step
//     and n_points only, so all four waves leave together, at the top of a step where no LDS-DMA piece is in flight and no
//     barrier is half passed (the exit of the terminating render kernels, nwe_mfma_render.h);
//   * density_only is launch-uniform; nothing is atomic but the final OR of the flag word; nothing waits for another
//     workgroup; the only blockIdx-dependent value is the item.
// A row depends on its point and its direction alone: lanes do not exchange values (the one cross-lane operation of mlp_eval
// is the swap between the two halves of a lane pair, which carry the same point), so neither n_points nor the neighbours nor
// the position in the workgroup nor the step count nor the other output reach it.
template <int W, int D, int SKIP, bool X3, int FORM>
__global__ void __launch_bounds__(256) query_mfma_kernel(QueryArgs a, NetMfma net) {
    using S = Shape<W, D>;
    using SM = QuerySmem<W, D>;
    __shared__ __attribute__((aligned(16))) char smem[SM::TOTAL];
    const unsigned item = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5;

    float* s_bias = reinterpret_cast<float*>(smem + SM::BOFF);
    constexpr int NCH = S::n_chunks(FORM);       // the launcher checks the network's n_chunks against it
    constexpr int NROWS = S::n_bias_rows(FORM);  // kFormFolded: the alpha layer's weights and bias ride behind the bias rows
    static_assert(NROWS * 32 * 4 <= SM::BIAS_BYTES, "bias table too small for the dot rows");
    for (int i = threadIdx.x; i < NROWS * 32; i += 256) s_bias[i] = net.bias[i];
    const float* bias = s_bias;
    const float* dot_tab = bias + NCH * 32;

    Walker<S::CHUNK_BYTES, X3> wk;
    wk.buf0 = smem; wk.lds_chunks = (uint32_t)(uintptr_t)(LDS_AS char*)smem;
    wk.tail0 = smem + SM::LOFF; wk.lds_tail = wk.lds_chunks + SM::LOFF; wk.t3 = 0;
    wk.b = 0; wk.wave = wave; wk.lane_off = lane * 16;

    char* gd_lds = smem + SM::GOFF + wave * (2 * S::KD * kTileBytes) + lane * 16;
    const bool density_only = a.density_only != 0;
    const int n = a.n_points;
    __syncthreads();   // the bias table

    uint32_t flags = 0;
    for (int step = 0; step < a.steps; ++step) {
        const int64_t first = ((int64_t)item * a.steps + step) * kQueryPacket;   // of the workgroup's packet
        if (first >= n) break;   // workgroup-uniform
#include "nwe_mfma_query_step.h"   // the step, shared as text with query_mfma_counted_kernel below
    }
    if (flags && a.flags) atomicOr(a.flags, flags);
}

// The counted form (nwe_render_sparse_async): the host knows only a CAPACITY, a.n_points, and sizes the grid for it
// (query_counted_grid, nwe_plan.h); the point count is a device word an earlier kernel on the stream has written.  Every
// workgroup reads n = min(*count, capacity) once and walks the packets item, item + grid, item + 2 grid, ... below n - a strided
// walk: a contiguous run sized for the capacity would leave the whole of a thinly selected chunk to the first few workgroups.
// a.steps is not read.  A workgroup with no packet below n (all of them when n == 0) returns before the bias table, before any
// LDS-DMA piece and before any barrier; the others leave at the top of a step as the kernel above does.  Both tests depend on
// item, the grid and n only, so the four waves leave together.  The step is the kernel's above, the same text: a row is the same
// bits in either kernel, whatever packet of whichever workgroup it falls into.
template <int W, int D, int SKIP, bool X3, int FORM>
__global__ void __launch_bounds__(256) query_mfma_counted_kernel(QueryArgs a, NetMfma net, const uint32_t* __restrict__ count) {
    using S = Shape<W, D>;
    using SM = QuerySmem<W, D>;
    __shared__ __attribute__((aligned(16))) char smem[SM::TOTAL];
    const unsigned item = blockIdx.x;
    const uint32_t counted = *count;
    const int n = (int)(counted < (uint32_t)a.n_points ? counted : (uint32_t)a.n_points);
    if ((int64_t)item * kQueryPacket >= n) return;   // workgroup-uniform; nothing has been touched
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5;

    float* s_bias = reinterpret_cast<float*>(smem + SM::BOFF);
    constexpr int NCH = S::n_chunks(FORM);
    constexpr int NROWS = S::n_bias_rows(FORM);
    static_assert(NROWS * 32 * 4 <= SM::BIAS_BYTES, "bias table too small for the dot rows");
    for (int i = threadIdx.x; i < NROWS * 32; i += 256) s_bias[i] = net.bias[i];
    const float* bias = s_bias;
    const float* dot_tab = bias + NCH * 32;

    Walker<S::CHUNK_BYTES, X3> wk;
    wk.buf0 = smem; wk.lds_chunks = (uint32_t)(uintptr_t)(LDS_AS char*)smem;
    wk.tail0 = smem + SM::LOFF; wk.lds_tail = wk.lds_chunks + SM::LOFF; wk.t3 = 0;
    wk.b = 0; wk.wave = wave; wk.lane_off = lane * 16;

    char* gd_lds = smem + SM::GOFF + wave * (2 * S::KD * kTileBytes) + lane * 16;
    const bool density_only = a.density_only != 0;
    __syncthreads();   // the bias table

    uint32_t flags = 0;
    for (int64_t packet = item;; packet += gridDim.x) {
        const int64_t first = packet * kQueryPacket;
        if (first >= n) break;   // workgroup-uniform
#include "nwe_mfma_query_step.h"
    }
    if (flags && a.flags) atomicOr(a.flags, flags);
}

// One query launch of a shape's kernel: `blocks` workgroups of a.steps packets each.  Explicitly instantiated per shape
// (nwe_mfma_shapes.h, nwe_mfma_inst.hip), which instantiates the shape's two kernels (three-pass / single-pass).
template <int W, int D, int SKIP, int FORM>
void launch_one_query(QueryArgs a, const NetMfma& net, bool three_pass, unsigned blocks, hipStream_t stream) {
    if (blocks == 0) return;
    if (three_pass) hipLaunchKernelGGL((query_mfma_kernel<W, D, SKIP, true, FORM>), dim3(blocks), dim3(256), 0, stream, a, net);
    else hipLaunchKernelGGL((query_mfma_kernel<W, D, SKIP, false, FORM>), dim3(blocks), dim3(256), 0, stream, a, net);
}

// ... of a shape's counted kernel: `blocks` workgroups for the capacity a.n_points, the count at `count` on the device.
template <int W, int D, int SKIP, int FORM>
void launch_one_query_counted(QueryArgs a, const NetMfma& net, const uint32_t* count, bool three_pass, unsigned blocks, hipStream_t stream) {
    if (blocks == 0) return;
    if (three_pass) hipLaunchKernelGGL((query_mfma_counted_kernel<W, D, SKIP, true, FORM>), dim3(blocks), dim3(256), 0, stream, a, net, count);
    else hipLaunchKernelGGL((query_mfma_counted_kernel<W, D, SKIP, false, FORM>), dim3(blocks), dim3(256), 0, stream, a, net, count);
}

}  // namespace nwe
