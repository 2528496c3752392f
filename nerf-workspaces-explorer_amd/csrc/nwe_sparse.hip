// The sparse frame (include/nwe.h, nwe_render_sparse): the radiance grid's frame as a proposal, the network's rows where the proposal
// sees weight, the grid's rows elsewhere.  Plain HIP, no MFMA here: the network runs in the point query's kernels between the
// emit and the composite stage.  A translation unit of its own: every other code object keeps the kernels it had.  The grid lookup
// is restated from nwe_radiance_grid.hip, as that unit restated the coarse grid's, and must stay equal to it bit for bit
// (tests/test_gpu_sparse_fine.py compares the two proposals).
#include "nwe_host.h"

namespace nwe {

// a + (b - a) * f: three fp32 operations, each rounded on its own (this unit is compiled with -ffp-contract=off as well)
__device__ __forceinline__ float sparse_lerp(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), f)); }
__device__ __forceinline__ float4 sparse_lerp4(const float4& a, const float4& b, float f) {
    return make_float4(sparse_lerp(a.x, b.x, f), sparse_lerp(a.y, b.y, f), sparse_lerp(a.z, b.z, f), sparse_lerp(a.w, b.w, f));
}

// radiance_grid_row of nwe_radiance_grid.hip: the eight indices are clamped to the grid on every path, so no load leaves the
// buffer whatever the point holds; outside the box the row is zero.
__device__ __forceinline__ float4 sparse_grid_row(const RadianceGrid& g, const float4* __restrict__ v, float px, float py, float pz) {
    const float p[3] = {px, py, pz};
    int i0[3], i1[3];
    float f[3];
    bool inside = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float gc = __fsub_rn(__fmul_rn(__fsub_rn(p[c], g.lo[c]), g.inv[c]), 0.5f);
        inside = inside && !bad(p[c]) && !(gc < -0.5f) && !(gc > __fsub_rn((float)g.res[c], 0.5f));
        const float fl = floorf(gc);
        f[c] = __fsub_rn(gc, fl);   // exact
        const int i = inside ? (int)fl : 0;
        i0[c] = min(max(i, 0), g.res[c] - 1);
        i1[c] = min(max(i + 1, 0), g.res[c] - 1);
    }
    if (!inside) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int ry = g.res[1], rz = g.res[2];
    const float4* r00 = v + ((int64_t)i0[0] * ry + i0[1]) * rz;
    const float4* r01 = v + ((int64_t)i0[0] * ry + i1[1]) * rz;
    const float4* r10 = v + ((int64_t)i1[0] * ry + i0[1]) * rz;
    const float4* r11 = v + ((int64_t)i1[0] * ry + i1[1]) * rz;
    const float4 t000 = r00[i0[2]], t001 = r00[i1[2]], t010 = r01[i0[2]], t011 = r01[i1[2]];
    const float4 t100 = r10[i0[2]], t101 = r10[i1[2]], t110 = r11[i0[2]], t111 = r11[i1[2]];
    const float4 c00 = sparse_lerp4(t000, t001, f[2]), c01 = sparse_lerp4(t010, t011, f[2]);
    const float4 c10 = sparse_lerp4(t100, t101, f[2]), c11 = sparse_lerp4(t110, t111, f[2]);
    return sparse_lerp4(sparse_lerp4(c00, c01, f[1]), sparse_lerp4(c10, c11, f[1]), f[0]);
}

__device__ __forceinline__ float4 sparse_grid_at(const RadianceGrid& g, const Ray& r, float z) {
    float px, py, pz;
    point_at(r, z, px, py, pz);
    return sparse_grid_row(g, g.rows, px, py, pz);
}

// The selection of one ray, fed its samples in order.  hit[s] = !(w <= min_weight); selected[t] = OR of hit over t - d .. t + d.
// `win` holds the hits of the last 2 d + 1 samples, newest in bit 0: once sample s is in, the window is that of t = s - d, which is
// final.  Samples before 0 and behind S - 1 are no hits: `win` starts empty and finish() shifts in zeros.  d <= 8: 17 bits.
struct SparseSelector {
    uint8_t* mask;     // this ray's column of the chunk's mask, element t at mask[t * stride]
    int64_t stride;
    uint32_t win, keep;
    int d, count;
    __device__ __forceinline__ void reset(uint8_t* mask_, int64_t stride_, int dilate) {
        mask = mask_; stride = stride_; d = dilate; win = 0u; keep = (2u << (2 * dilate)) - 1u; count = 0;
    }
    __device__ __forceinline__ void settle(int t) {
        const bool sel = (win & keep) != 0u;
        mask[t * stride] = sel ? 1 : 0;
        count += sel ? 1 : 0;
    }
    __device__ __forceinline__ void push(int s, float w, float min_weight) {
        win = win << 1 | (!(w <= min_weight) ? 1u : 0u);
        if (s >= d) settle(s - d);
    }
    __device__ __forceinline__ void finish(int S) {
        for (int t = max(S - d, 0); t < S; ++t) { win <<= 1; settle(t); }
    }
};

// mark.  radiance_grid_render_kernel's walk, statement for statement: one wave per workgroup, one thread per ray of the chunk, the
// coarse weights in the thread's LDS column where FineSampler reads them (element i at wc[i * kGridThreads]).  Instead of storing
// the ray, the output pass leaves its depths, rows and the dilated mask in the chunk's sample-major tables and the ray's selected
// count in offsets[]; weights_coarse and weights_grid go straight to the caller.
// LDS (dynamic): t[ns] | 1 - t[ns] | u[ni] | weights[ns][kGridThreads], as that kernel.
__global__ void __launch_bounds__(kGridThreads) sparse_mark_kernel(RenderArgs a, RadianceGrid g, SparseChunk c) {
    extern __shared__ float lds[];
    const int ns = a.n_samples, ni = a.n_importance, tid = threadIdx.x;
    float* s_t = lds;
    float* s_omt = s_t + ns;
    float* s_u = s_omt + ns;
    float* wc = s_u + ni + tid;
    for (int i = tid; i < ns; i += kGridThreads) { s_t[i] = a.t_vals[i]; s_omt[i] = a.omt_vals[i]; }
    for (int i = tid; i < ni; i += kGridThreads) s_u[i] = a.u_vals[i];
    __syncthreads();

    const int local = blockIdx.x * kGridThreads + tid;
    if (local >= c.count) return;
    const int64_t idx = c.first + local, n = c.count;
    const Ray r = make_ray<false>(a, seed_ray(a, idx));
    const bool single = ni == 0;   // the only pass is the output
    float* const w_out = c.weights_coarse ? c.weights_coarse + idx * ns : nullptr;
    float* const wg_out = c.weights_grid ? c.weights_grid + idx * c.S : nullptr;
    float* const z_col = c.z + local;
    float4* const row_col = c.row_grid + local;
    SparseSelector sel;
    sel.reset(c.mask + local, n, c.dilate);
    Composite comp;
    comp.reset();
    float z = coarse_z(r, s_t[0], s_omt[0]);
    float4 row = sparse_grid_at(g, r, z);
    for (int s = 0; s < ns; ++s) {
        const bool last = s + 1 == ns;
        const float z_next = last ? 0.f : coarse_z(r, s_t[s + 1], s_omt[s + 1]);
        float4 row_next = row;
        if (!last) row_next = sparse_grid_at(g, r, z_next);
        const float w = comp.step(row.x, row.y, row.z, row.w, z, z_next, last, r.dnorm);
        wc[s * kGridThreads] = w;
        if (w_out) w_out[s] = w;
        if (single) {
            z_col[s * n] = z; row_col[s * n] = row;
            if (wg_out) wg_out[s] = w;
            sel.push(s, w, c.min_weight);
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
        z = fs.next(r);
        row = sparse_grid_at(g, r, z);
        for (int s = 0; s < S; ++s) {
            const bool last = s + 1 == S;
            float z_next = 0.f;
            float4 row_next = row;
            if (!last) { z_next = fs.next(r); row_next = sparse_grid_at(g, r, z_next); }
            const float w = comp.step(row.x, row.y, row.z, row.w, z, z_next, last, r.dnorm);
            z_col[s * n] = z; row_col[s * n] = row;
            if (wg_out) wg_out[s] = w;
            sel.push(s, w, c.min_weight);
            z = z_next; row = row_next;
        }
    }
    sel.finish(c.S);
    c.offsets[local] = (uint32_t)sel.count;
}

// scan.  One workgroup: offsets[] (the counts) becomes its exclusive scan in place, tile by tile of kScanThreads elements with the
// running sum carried in a register every thread holds; *total = the sum.  A chunk has at most 2^22 samples, so the sums fit 32 bits.
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads) sparse_scan_kernel(uint32_t* __restrict__ offsets, int count, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[kScanThreads / 64];
    __shared__ uint32_t s_tile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (int base = 0; base < count; base += kScanThreads) {   // block-uniform trip count: the barriers are met by every thread
        const int i = base + tid;
        const uint32_t v = i < count ? offsets[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        if (wave == 0) {
            const uint32_t w = lane < kScanThreads / 64 ? s_wave[lane] : 0u;
            uint32_t wi = w;
#pragma unroll
            for (int off = 1; off < kScanThreads / 64; off <<= 1) {
                const uint32_t up = __shfl_up(wi, off);
                if (lane >= off) wi += up;
            }
            if (lane < kScanThreads / 64) s_wave[lane] = wi - w;   // exclusive over the waves
            if (lane == kScanThreads / 64 - 1) s_tile = wi;
        }
        __syncthreads();
        if (i < count) offsets[i] = carry + s_wave[wave] + incl - v;
        carry += s_tile;
        __syncthreads();   // s_wave and s_tile are rewritten by the next tile
    }
    if (tid == 0) *total = carry;
}

// emit.  One thread per ray of the chunk: the point p = o + d * z (point_at, what every kernel encodes) and the ray's normalised view
// direction (make_ray<true>: the bits of create_rays' columns 8..10) of each selected sample, in sample order from offsets[ray].
// A ray with nothing selected builds no ray.
__global__ void __launch_bounds__(256) sparse_emit_kernel(RenderArgs a, SparseChunk c) {
    const int local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= c.count) return;
    const int64_t n = c.count;
    const uint32_t begin = c.offsets[local];
    const uint32_t end = local + 1 < c.count ? c.offsets[local + 1] : *c.total;
    if (begin == end) return;
    const Ray r = make_ray<true>(a, seed_ray(a, c.first + local));
    uint32_t k = begin;
    for (int s = 0; s < c.S && k < end; ++s) {
        if (!c.mask[s * n + local]) continue;
        float px, py, pz;
        point_at(r, c.z[s * n + local], px, py, pz);
        float* p = c.points + (int64_t)k * 3;
        p[0] = px; p[1] = py; p[2] = pz;
        if (c.dirs) {
            float* d = c.dirs + (int64_t)k * 3;
            d[0] = r.vx; d[1] = r.vy; d[2] = r.vz;
        }
        ++k;
    }
}

// composite.  One thread per ray of the chunk, one wave per workgroup as the grid's kernel (the flags take one atomic per wave at the
// most).  Walks the samples in order, one depth ahead as every compositing loop does; a selected sample takes the next of the
// ray's query rows, any other its grid row.
__global__ void __launch_bounds__(kGridThreads) sparse_composite_kernel(RenderArgs a, SparseChunk c) {
    const int local = blockIdx.x * kGridThreads + threadIdx.x;
    uint32_t flags = 0;
    if (local < c.count) {
        const int64_t idx = c.first + local, n = c.count;
        const int S = c.S;
        const Ray r = make_ray<false>(a, seed_ray(a, idx));
        const float4* q = c.rows + c.offsets[local];
        float4* const raw_out = c.raw_fine ? reinterpret_cast<float4*>(c.raw_fine) + idx * S : nullptr;
        float* const z_out = c.z_fine ? c.z_fine + idx * S : nullptr;
        uint8_t* const sel_out = c.selected ? c.selected + idx * S : nullptr;
        Composite comp;
        comp.reset();
        float z = c.z[local];
        for (int s = 0; s < S; ++s) {
            const bool last = s + 1 == S;
            const float z_next = last ? 0.f : c.z[(s + 1) * n + local];
            const bool sel = c.mask[s * n + local] != 0;
            float4 row;
            if (sel) row = *q++; else row = c.row_grid[s * n + local];
            comp.step(row.x, row.y, row.z, row.w, z, z_next, last, r.dnorm);
            if (raw_out) raw_out[s] = row;
            if (z_out) z_out[s] = z;
            if (sel_out) sel_out[s] = sel ? 1 : 0;
            z = z_next;
        }
        // the rgb / depth / acc bits only: no disparity is written, and the coarse bits are never raised
        flags = store_ray(a.out, idx, comp, true, a.white_bkgd != 0) & (NWE_FLAG_RGB | NWE_FLAG_DEPTH | NWE_FLAG_ACC);
    }
    if (a.out.flags) {   // one atomic per wave at the most
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) flags |= __shfl_xor(flags, off);
        if (threadIdx.x == 0 && flags) atomicOr(a.out.flags, flags);
    }
}

void launch_sparse_mark(const RenderArgs& a, const RadianceGrid& g, const SparseChunk& c, hipStream_t stream) {
    if (c.count <= 0) return;
    const size_t lds = ((size_t)2 * a.n_samples + a.n_importance + (size_t)a.n_samples * kGridThreads) * sizeof(float);
    hipLaunchKernelGGL(sparse_mark_kernel, dim3((unsigned)((c.count + kGridThreads - 1) / kGridThreads)), dim3(kGridThreads), lds, stream, a, g, c);
}

void launch_sparse_scan(const SparseChunk& c, hipStream_t stream) {
    if (c.count <= 0) return;
    hipLaunchKernelGGL(sparse_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, c.offsets, c.count, c.total);
}

void launch_sparse_emit(const RenderArgs& a, const SparseChunk& c, hipStream_t stream) {
    if (c.count <= 0) return;
    hipLaunchKernelGGL(sparse_emit_kernel, dim3((unsigned)((c.count + 255) / 256)), dim3(256), 0, stream, a, c);
}

void launch_sparse_composite(const RenderArgs& a, const SparseChunk& c, hipStream_t stream) {
    if (c.count <= 0) return;
    hipLaunchKernelGGL(sparse_composite_kernel, dim3((unsigned)((c.count + kGridThreads - 1) / kGridThreads)), dim3(kGridThreads), 0, stream, a, c);
}

}  // namespace nwe
