// The radiance grid's frame (include/nwe.h, nwe_render_grid): both passes of the reference pipeline with run_network replaced by a
// trilinear lookup of (rgb_raw, sigma_raw) rows.  No network, no MFMA, no weight stream: the kernel is bound by its gathers.
// A translation unit of its own: the code objects of the render kernels and of the baked coarse pass keep the kernels they had.
#include "nwe_host.h"

namespace nwe {

// a + (b - a) * f: three fp32 operations, each rounded on its own (this unit is compiled with -ffp-contract=off as well)
__device__ __forceinline__ float rgrid_lerp(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), f)); }
__device__ __forceinline__ float4 rgrid_lerp4(const float4& a, const float4& b, float f) {
    return make_float4(rgrid_lerp(a.x, b.x, f), rgrid_lerp(a.y, b.y, f), rgrid_lerp(a.z, b.z, f), rgrid_lerp(a.w, b.w, f));
}

// The grid's row at the fp32 sample point, before the division by 10: the coordinate, inside test, indices and fraction of the
// coarse density grid (include/nwe.h, nwe_set_coarse_grid, steps 2 to 4; restated here so that nwe_coarse_grid.hip's code object
// stays as it is), each of the four channels interpolated on its own along z, then y, then x.  Outside the box the row is zero.
// The eight indices are clamped to the grid on every path, so no load leaves the buffer whatever the point holds.  Nothing here
// depends on the compositing state: the eight 16-byte loads of a sample are issued together, ahead of the previous sample's shading.
__device__ __forceinline__ float4 radiance_grid_row(const RadianceGrid& g, const float4* __restrict__ v, float px, float py, float pz) {
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
    if (!inside) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int ry = g.res[1], rz = g.res[2];
    // z fastest, four channels innermost: the two z neighbours of a tap are 32 adjacent bytes
    const float4* r00 = v + ((int64_t)i0[0] * ry + i0[1]) * rz;
    const float4* r01 = v + ((int64_t)i0[0] * ry + i1[1]) * rz;
    const float4* r10 = v + ((int64_t)i1[0] * ry + i0[1]) * rz;
    const float4* r11 = v + ((int64_t)i1[0] * ry + i1[1]) * rz;
    const float4 t000 = r00[i0[2]], t001 = r00[i1[2]], t010 = r01[i0[2]], t011 = r01[i1[2]];
    const float4 t100 = r10[i0[2]], t101 = r10[i1[2]], t110 = r11[i0[2]], t111 = r11[i1[2]];
    const float4 c00 = rgrid_lerp4(t000, t001, f[2]), c01 = rgrid_lerp4(t010, t011, f[2]);
    const float4 c10 = rgrid_lerp4(t100, t101, f[2]), c11 = rgrid_lerp4(t110, t111, f[2]);
    return rgrid_lerp4(rgrid_lerp4(c00, c01, f[1]), rgrid_lerp4(c10, c11, f[1]), f[0]);
}

__device__ __forceinline__ float4 radiance_grid_at(const RadianceGrid& g, const Ray& r, float z) {
    float px, py, pz;
    point_at(r, z, px, py, pz);
    return radiance_grid_row(g, g.rows, px, py, pz);
}

// One wave per workgroup, one thread per ray of the call.  The ray is built as the lean kernels build it (seed_ray / make_ray).
// Pass 0 walks the coarse depths as coarse_grid_weights_kernel does, composites the grid's rows with the render kernels' own
// Composite and keeps each weight in the thread's LDS column (element i at wc[i * kGridThreads]: consecutive lanes, consecutive
// banks), where FineSampler reads it.  With n_importance > 0 the second pass walks FineSampler's merged depths, one depth ahead
// as the render kernels do, looks each up and composites; store_ray writes the pass that is the output.
// Both loops fetch the row of the NEXT sample before they shade the current one.
// LDS (dynamic): t[ns] | 1 - t[ns] | u[ni] | weights[ns][kGridThreads]: 16.5 KiB + 1 KiB of tables for 64 + 128 samples, 34 KiB at
// the domain's maximum.
//   a.out   rgb / depth / acc / flags as store_ray takes them; weights_coarse [R, ns], z_fine [R, S] and raw_fine [R, S, 4]
//           (S = ns + ni, the output pass) are the call's diagnostics.  Each may be null; the tests are kernel-uniform.
__global__ void __launch_bounds__(kGridThreads) radiance_grid_render_kernel(RenderArgs a, RadianceGrid g) {
    extern __shared__ float lds[];
    const int ns = a.n_samples, ni = a.n_importance, tid = threadIdx.x;
    float* s_t = lds;
    float* s_omt = s_t + ns;
    float* s_u = s_omt + ns;
    float* wc = s_u + ni + tid;
    for (int i = tid; i < ns; i += kGridThreads) { s_t[i] = a.t_vals[i]; s_omt[i] = a.omt_vals[i]; }
    for (int i = tid; i < ni; i += kGridThreads) s_u[i] = a.u_vals[i];
    __syncthreads();

    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + tid;
    uint32_t flags = 0;
    if (idx < a.n_rays) {
        const Ray r = make_ray<false>(a, seed_ray(a, idx));
        const bool single = ni == 0;   // the only pass is the output
        float* const w_out = a.out.weights_coarse ? a.out.weights_coarse + idx * ns : nullptr;
        Composite comp;
        comp.reset();
        float z = coarse_z(r, s_t[0], s_omt[0]);
        float4 row = radiance_grid_at(g, r, z);
        for (int s = 0; s < ns; ++s) {
            const bool last = s + 1 == ns;
            const float z_next = last ? 0.f : coarse_z(r, s_t[s + 1], s_omt[s + 1]);
            float4 row_next = row;
            if (!last) row_next = radiance_grid_at(g, r, z_next);
            const float w = comp.step(row.x, row.y, row.z, row.w, z, z_next, last, r.dnorm);
            wc[s * kGridThreads] = w;
            if (w_out) w_out[s] = w;
            if (single) {
                if (a.out.raw_fine) reinterpret_cast<float4*>(a.out.raw_fine)[idx * ns + s] = row;
                if (a.out.z_fine) a.out.z_fine[idx * ns + s] = z;
            }
            z = z_next; row = row_next;
        }
        if (!single) {
            FineSampler fs;
            fs.wc = wc; fs.stride = kGridThreads; fs.u_tab = s_u; fs.u_rand = nullptr; fs.ns = ns; fs.ni = ni;
            fs.cd.t_tab = s_t; fs.cd.omt_tab = s_omt; fs.cd.jitter = nullptr; fs.cd.row = 0; fs.cd.ns = ns;
            fs.prepare(r);
            comp.reset();
            const int S = ns + ni;
            float4* const raw_out = a.out.raw_fine ? reinterpret_cast<float4*>(a.out.raw_fine) + idx * S : nullptr;
            float* const z_out = a.out.z_fine ? a.out.z_fine + idx * S : nullptr;
            z = fs.next(r);
            row = radiance_grid_at(g, r, z);
            for (int s = 0; s < S; ++s) {
                const bool last = s + 1 == S;
                float z_next = 0.f;
                float4 row_next = row;
                if (!last) { z_next = fs.next(r); row_next = radiance_grid_at(g, r, z_next); }
                comp.step(row.x, row.y, row.z, row.w, z, z_next, last, r.dnorm);
                if (raw_out) raw_out[s] = row;
                if (z_out) z_out[s] = z;
                z = z_next; row = row_next;
            }
        }
        // the rgb / depth / acc bits only: no disparity is written, and the coarse bits are never raised
        flags = store_ray(a.out, idx, comp, true, a.white_bkgd != 0) & (NWE_FLAG_RGB | NWE_FLAG_DEPTH | NWE_FLAG_ACC);
    }
    if (a.out.flags) {   // one atomic per wave at the most
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) flags |= __shfl_xor(flags, off);
        if (tid == 0 && flags) atomicOr(a.out.flags, flags);
    }
}

void launch_radiance_grid_render(const RenderArgs& a, const RadianceGrid& g, hipStream_t stream) {
    if (a.n_rays <= 0) return;
    const size_t lds = ((size_t)2 * a.n_samples + a.n_importance + (size_t)a.n_samples * kGridThreads) * sizeof(float);
    hipLaunchKernelGGL(radiance_grid_render_kernel, dim3((unsigned)((a.n_rays + kGridThreads - 1) / kGridThreads)), dim3(kGridThreads), lds,
                       stream, a, g);
}

}  // namespace nwe
