// The producer of the baked coarse pass (include/nwe.h, nwe_set_coarse_grid): coarse weights from a density grid instead of
// the coarse network.  A translation unit of its own: the code objects of the render kernels keep the kernels they had.
#include "nwe_host.h"

namespace nwe {

// a + (b - a) * f: three fp32 operations, each rounded on its own (this unit is compiled with -ffp-contract=off as well)
__device__ __forceinline__ float grid_lerp(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), f)); }

// sigma_raw of the grid at the fp32 sample point, before the division by 10: the rule of include/nwe.h, steps 2 to 4.
// The eight indices are clamped to the grid on every path, so no load leaves the buffer whatever the point holds.
__device__ __forceinline__ float coarse_grid_sigma(const CoarseGrid& g, const float* __restrict__ v, float px, float py, float pz) {
    const float p[3] = {px, py, pz};
    int i0[3], i1[3];
    float f[3];
    bool inside = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float gc = __fsub_rn(__fmul_rn(__fsub_rn(p[c], g.lo[c]), g.inv[c]), 0.5f);
        // (float)res - 0.5f is exact (res <= 512); a point that is not finite is outside whatever gc came to
        inside = inside && !bad(p[c]) && !(gc < -0.5f) && !(gc > __fsub_rn((float)g.res[c], 0.5f));
        const float fl = floorf(gc);
        f[c] = __fsub_rn(gc, fl);   // exact
        const int i = inside ? (int)fl : 0;
        i0[c] = min(max(i, 0), g.res[c] - 1);
        i1[c] = min(max(i + 1, 0), g.res[c] - 1);
    }
    if (!inside) return 0.f;
    const int ry = g.res[1], rz = g.res[2];
    // z fastest: the two z neighbours of a tap are adjacent in memory
    const float* r00 = v + ((int64_t)i0[0] * ry + i0[1]) * rz;
    const float* r01 = v + ((int64_t)i0[0] * ry + i1[1]) * rz;
    const float* r10 = v + ((int64_t)i1[0] * ry + i0[1]) * rz;
    const float* r11 = v + ((int64_t)i1[0] * ry + i1[1]) * rz;
    const float c00 = grid_lerp(r00[i0[2]], r00[i1[2]], f[2]);
    const float c01 = grid_lerp(r01[i0[2]], r01[i1[2]], f[2]);
    const float c10 = grid_lerp(r10[i0[2]], r10[i1[2]], f[2]);
    const float c11 = grid_lerp(r11[i0[2]], r11[i1[2]], f[2]);
    return grid_lerp(grid_lerp(c00, c01, f[1]), grid_lerp(c10, c11, f[1]), f[0]);
}

// One thread per ray of the call.  The ray is built as the lean kernels build it (seed_ray / make_ray), its coarse samples are
// walked in order, each sample's sigma_raw read from the grid and composited with the render kernels' own Composite for
// raw = (0, 0, 0, sigma_raw): the weight is raw2outputs' fourth return value (nerf/models/model_utils.py:49-100).
//   table   [n_samples][n_rays], sample-major: consecutive threads write consecutive floats; what the consumer reads at k = 1
//   sigma   [n_rays][n_samples], weights [n_rays][n_samples]: the test hook's ray-major outputs (nwe_coarse_grid_weights)
// Each may be null.  Bound by the latency of the eight loads per sample; no LDS.
__global__ void __launch_bounds__(256) coarse_grid_weights_kernel(RenderArgs a, CoarseGrid g, float* __restrict__ table,
                                                                  float* __restrict__ sigma, float* __restrict__ weights) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n_rays) return;
    const Ray r = make_ray<false>(a, seed_ray(a, idx));
    const int ns = a.n_samples;
    Composite comp;
    comp.reset();
    float z = coarse_z(r, a.t_vals[0], a.omt_vals[0]);
    for (int s = 0; s < ns; ++s) {
        const bool last = s + 1 == ns;
        const float z_next = last ? 0.f : coarse_z(r, a.t_vals[s + 1], a.omt_vals[s + 1]);
        float px, py, pz;
        point_at(r, z, px, py, pz);
        const float sig = coarse_grid_sigma(g, g.sigma, px, py, pz);
        const float w = comp.step(0.f, 0.f, 0.f, sig, z, z_next, last, r.dnorm);
        if (table) table[(int64_t)s * a.n_rays + idx] = w;
        if (sigma) sigma[idx * ns + s] = sig;
        if (weights) weights[idx * ns + s] = w;
        z = z_next;
    }
}

void launch_coarse_grid_weights(const RenderArgs& a, const CoarseGrid& g, float* table, float* sigma, float* weights, hipStream_t stream) {
    if (a.n_rays <= 0) return;
    hipLaunchKernelGGL(coarse_grid_weights_kernel, dim3((unsigned)((a.n_rays + 255) / 256)), dim3(256), 0, stream, a, g, table, sigma, weights);
}

}  // namespace nwe
