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
        {   // start streaming chunks 0 and 1 (layer 0, tiles 0 and 1): they fly while the point is loaded and encoded
            wk.start(net.stream, bias);
            wk.begin(S::N_L0, 0, 0);
#pragma unroll
            for (int i = 0; i < S::N_L0; ++i) wk.piece(i);
            wk.begin(S::N_L0, 1, 1);
#pragma unroll
            for (int i = 0; i < S::N_L0; ++i) wk.piece(i);
        }
        const int64_t idx = first + wave * kRaysPerWave + (lane & 31);
        const bool live = idx < n && half == 0;          // this lane stores the outputs of its point
        const int row = (int)(idx < n ? idx : n - 1);    // a lane past the call's points computes the last one along
        const float* p = a.points + (int64_t)row * 3;
        const float px = p[0], py = p[1], pz = p[2];
        if constexpr (FORM != kFormNoViewDirs) {
            // gamma(d) of this step's points into the wave's OWN slots (model_utils.py:23-25 embeds the direction of every
            // point).  No barrier guards the write: the slots are private to the wave - slot address = f(wave, lane) - so the only
            // earlier accesses are this wave's own reads in the previous step's mlp_eval, and LDS serves the accesses of one
            // wave in the order it issued them; the reads of this step's mlp_eval are issued behind the write likewise (and
            // behind the lgkmcnt(0) of the barrier below).  LDS-DMA pieces never land here (chunk buffers and tail slots only).
            float vx = 0.f, vy = 0.f, vz = 0.f;          // no directions given: sigma does not depend on them
            if (a.dirs) {
                const float* d = a.dirs + (int64_t)(row / a.points_per_dir) * 3;
                vx = d[0]; vy = d[1]; vz = d[2];
            }
            h8 GDhi[S::KD], GDlo[S::KD];
            encode<2, S::KD, X3>(vx, vy, vz, half, GDhi, GDlo);
#pragma unroll
            for (int k = 0; k < S::KD; ++k) {
                *reinterpret_cast<h8*>(gd_lds + (2 * k) * kTileBytes) = GDhi[k];
                *reinterpret_cast<h8*>(gd_lds + (2 * k + 1) * kTileBytes) = GDlo[k];
            }
        }
        float rr, rg, rb, rs;
        {
            h8 Ghi[S::KG], Glo[S::KG];
            // handler.py:93: scalar_factor = 10, a true division (embedding.py:48)
            encode<5, S::KG, X3>(__fdiv_rn(px, 10.f), __fdiv_rn(py, 10.f), __fdiv_rn(pz, 10.f), half, Ghi, Glo);
            wk.template sync<false>();   // publishes chunk 0
            Frags F;
#pragma unroll
            for (int k = 0; k < PD; ++k) {
                F.hi[k] = *reinterpret_cast<const h8*>(wk.cur() + lane * 16 + (2 * k) * kTileBytes);
                if (X3) F.lo[k] = *reinterpret_cast<const h8*>(wk.cur() + lane * 16 + (2 * k + 1) * kTileBytes);
            }
            mlp_eval<W, D, SKIP, X3, FORM>(wk, F, lane, net.inv_scale, Ghi, Glo, gd_lds, dot_tab, density_only, rr, rg, rb, rs);
        }
        if (live) {
            if (a.raw && store_raw(a.raw + idx * 4, rr, rg, rb, rs)) flags |= NWE_FLAG_RAW;
            if (a.sigma) {
                a.sigma[idx] = rs;
                if (bad(rs)) flags |= NWE_FLAG_RAW;
            }
        }
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

}  // namespace nwe
