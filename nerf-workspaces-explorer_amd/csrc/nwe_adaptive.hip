// The adaptive frame (include/nwe.h, nwe_render_adaptive): a lattice of every k-th pixel rendered by the networks, the pixels of the
// cells whose corners disagree rendered as well, the rest interpolated.  Plain HIP, no MFMA here: the networks run in the render
// kernels, on the ray lists this unit writes, between its stages.  A translation unit of its own: every other code object keeps
// the kernels it had.  The lattice arithmetic is nwe_plan.h's, which the planner and nwe_debug_adaptive_lattice compile too.
#include "nwe_host.h"

namespace nwe {

// a + (b - a) * f: three fp32 operations, each rounded on its own (sparse_lerp of nwe_sparse.hip; -ffp-contract=off here as well)
__device__ __forceinline__ float adaptive_lerp(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), f)); }

// Pixel p of the call: its pose and its local row and column
struct AdaptivePixel { int pose, r, w; };
__device__ __forceinline__ AdaptivePixel adaptive_pixel(const AdaptiveFrame& f, int p) {
    const int per_pose = f.h.len * f.w.len;
    AdaptivePixel x;
    x.pose = p / per_pose;
    const int rem = p - x.pose * per_pose;
    x.r = rem / f.w.len; x.w = rem - x.r * f.w.len;
    return x;
}
// The compact index of lattice pixel (i, j) of a pose
__device__ __forceinline__ int lattice_at(const AdaptiveFrame& f, int pose, int i, int j) { return (pose * f.h.n + i) * f.w.n + j; }

// lattice.  One thread per lattice pixel of the call, in the compact order [pose][i][j]: its pixel of the call.
__global__ void __launch_bounds__(256) adaptive_lattice_kernel(AdaptiveFrame f) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= f.lattice) return;
    const int per_pose = f.h.n * f.w.n;
    const int pose = t / per_pose, rem = t - pose * per_pose;
    const int i = rem / f.w.n, j = rem - i * f.w.n;
    f.list[t] = (pose * f.h.len + adaptive_entry(f.h, i)) * f.w.len + adaptive_entry(f.w, j);
}

// rays.  One thread per pixel of the list: the row create_rays_kernel writes for it - load_ray on the same pixel of the same camera,
// so the same two divisions, the same matrix product and the same bits.  Without view directions the row ends behind near and far.
__global__ void __launch_bounds__(256) adaptive_rays_kernel(RenderArgs a, const int32_t* __restrict__ list, int n, int cols, float* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const Ray r = load_ray(a, list[t]);
    float* o = out + (int64_t)t * cols;
    o[0] = r.ox; o[1] = r.oy; o[2] = r.oz; o[3] = r.dx; o[4] = r.dy; o[5] = r.dz;
    o[6] = r.near; o[7] = r.far;
    if (cols > 8) { o[8] = r.vx; o[9] = r.vy; o[10] = r.vz; }
}

// cells.  One thread per cell of the call: busy unless every pair of its corners agrees.  !(|a - b| <= tol): a NaN difference is busy.
__global__ void __launch_bounds__(256) adaptive_cells_kernel(AdaptiveFrame f) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int per_pose = f.h.cells * f.w.cells;
    if (t >= f.n_poses * per_pose) return;
    const int pose = t / per_pose, rem = t - pose * per_pose;
    const int ci = rem / f.w.cells, cj = rem - ci * f.w.cells;
    const int i1 = min(ci + 1, f.h.n - 1), j1 = min(cj + 1, f.w.n - 1);
    const int c[4] = {lattice_at(f, pose, ci, cj), lattice_at(f, pose, ci, j1), lattice_at(f, pose, i1, cj), lattice_at(f, pose, i1, j1)};
    float v[4][5];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q][0] = f.c_rgb[c[q] * 3]; v[q][1] = f.c_rgb[c[q] * 3 + 1]; v[q][2] = f.c_rgb[c[q] * 3 + 2];
        v[q][3] = f.c_acc[c[q]]; v[q][4] = f.c_depth[c[q]];
    }
    bool flat = true;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = p + 1; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 5; ++e) flat = flat && fabsf(__fsub_rn(v[p][e], v[q][e])) <= (e < 4 ? f.tol_rgb : f.tol_depth);
    f.busy[t] = flat ? 0 : 1;
}

// kinds.  One thread per pixel of the call.  The cells whose closed rectangle holds the pixel: its own (adaptive_cell) and, where it
// lies on the lattice row (column) that opens that cell, the one before it; a pixel on both is a lattice pixel.
__global__ void __launch_bounds__(256) adaptive_kinds_kernel(AdaptiveFrame f) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= f.pixels) return;
    const AdaptivePixel x = adaptive_pixel(f, p);
    uint8_t kind = 0;
    if (!(adaptive_on_lattice(f.h, x.r) && adaptive_on_lattice(f.w, x.w))) {
        const int ci = adaptive_cell(f.h, x.r), cj = adaptive_cell(f.w, x.w);
        const int ci0 = ci > 0 && adaptive_entry(f.h, ci) == x.r ? ci - 1 : ci;
        const int cj0 = cj > 0 && adaptive_entry(f.w, cj) == x.w ? cj - 1 : cj;
        const uint8_t* busy = f.busy + (int64_t)x.pose * f.h.cells * f.w.cells;
        bool any = false;
        for (int i = ci0; i <= ci; ++i)
            for (int j = cj0; j <= cj; ++j) any = any || busy[i * f.w.cells + j] != 0;
        kind = any ? 1 : 2;
    }
    f.kinds[p] = kind;
    f.counts[p] = kind == 1 ? 1u : 0u;
}

// scan.  sparse_scan_kernel of nwe_sparse.hip: one workgroup, counts[] becomes its exclusive scan in place, tile by tile of
// kScanThreads elements with the running sum carried in a register every thread holds; *total = the sum (at most 2^24).
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads) adaptive_scan_kernel(uint32_t* __restrict__ counts, int count, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[kScanThreads / 64];
    __shared__ uint32_t s_tile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (int base = 0; base < count; base += kScanThreads) {   // block-uniform trip count: the barriers are met by every thread
        const int i = base + tid;
        const uint32_t v = i < count ? counts[i] : 0u;
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
        if (i < count) counts[i] = carry + s_wave[wave] + incl - v;
        carry += s_tile;
        __syncthreads();   // s_wave and s_tile are rewritten by the next tile
    }
    if (tid == 0) *total = carry;
}

// emit.  One thread per pixel: a kind 1 pixel goes to its place in the list, counts[p] < the kind 1 pixels <= pixels - lattice <= the
// list's room (AdaptivePlan::list).
__global__ void __launch_bounds__(256) adaptive_emit_kernel(AdaptiveFrame f) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= f.pixels) return;
    if (f.kinds[p] == 1) f.list[f.counts[p]] = p;
}

// compose.  One thread per pixel of the call, one wave per workgroup (the flags take one atomic per wave at the most): a lattice
// pixel and a rendered one are copied from the compact outputs of their launch, an interpolated one is mixed from the four
// corners of its cell - along w on the top and on the bottom pair, then along h.
constexpr int kComposeThreads = 64;
__global__ void __launch_bounds__(kComposeThreads) adaptive_compose_kernel(AdaptiveFrame f) {
    const int p = blockIdx.x * kComposeThreads + threadIdx.x;
    uint32_t flags = p == 0 ? *f.render_flags & (NWE_FLAG_RGB | NWE_FLAG_DEPTH | NWE_FLAG_ACC) : 0u;
    if (p < f.pixels) {
        const AdaptivePixel x = adaptive_pixel(f, p);
        const uint8_t kind = f.kinds[p];
        float v[5];   // r, g, b, depth, acc
        if (kind != 2) {
            const int c = kind == 0 ? lattice_at(f, x.pose, adaptive_index(f.h, x.r), adaptive_index(f.w, x.w)) : f.lattice + (int)f.counts[p];
            v[0] = f.c_rgb[(int64_t)c * 3]; v[1] = f.c_rgb[(int64_t)c * 3 + 1]; v[2] = f.c_rgb[(int64_t)c * 3 + 2];
            v[3] = f.c_depth[c]; v[4] = f.c_acc[c];
        } else {
            const int ci = adaptive_cell(f.h, x.r), cj = adaptive_cell(f.w, x.w);
            const int i1 = min(ci + 1, f.h.n - 1), j1 = min(cj + 1, f.w.n - 1);
            const int h0 = adaptive_entry(f.h, ci), h1 = adaptive_entry(f.h, i1), w0 = adaptive_entry(f.w, cj), w1 = adaptive_entry(f.w, j1);
            const float fy = h1 == h0 ? 0.f : __fdiv_rn((float)(x.r - h0), (float)(h1 - h0));
            const float fx = w1 == w0 ? 0.f : __fdiv_rn((float)(x.w - w0), (float)(w1 - w0));
            const int c00 = lattice_at(f, x.pose, ci, cj), c01 = lattice_at(f, x.pose, ci, j1);
            const int c10 = lattice_at(f, x.pose, i1, cj), c11 = lattice_at(f, x.pose, i1, j1);
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                const float* src = e < 3 ? f.c_rgb + e : e == 3 ? f.c_depth : f.c_acc;
                const int step = e < 3 ? 3 : 1;
                const float top = adaptive_lerp(src[(int64_t)c00 * step], src[(int64_t)c01 * step], fx);
                const float bottom = adaptive_lerp(src[(int64_t)c10 * step], src[(int64_t)c11 * step], fx);
                v[e] = adaptive_lerp(top, bottom, fy);
            }
            flags |= ((bad(v[0]) || bad(v[1]) || bad(v[2])) ? NWE_FLAG_RGB : 0) | (bad(v[3]) ? NWE_FLAG_DEPTH : 0) | (bad(v[4]) ? NWE_FLAG_ACC : 0);
        }
        if (f.rgb) { f.rgb[(int64_t)p * 3] = v[0]; f.rgb[(int64_t)p * 3 + 1] = v[1]; f.rgb[(int64_t)p * 3 + 2] = v[2]; }
        if (f.depth) f.depth[p] = v[3];
        if (f.acc) f.acc[p] = v[4];
        if (f.kind) f.kind[p] = kind;
    }
    if (f.flags) {   // one atomic per wave at the most
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) flags |= __shfl_xor(flags, off);
        if (threadIdx.x == 0 && flags) atomicOr(f.flags, flags);
    }
}

static unsigned blocks_of(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

void launch_adaptive_lattice(const AdaptiveFrame& f, hipStream_t stream) {
    if (f.lattice <= 0) return;
    hipLaunchKernelGGL(adaptive_lattice_kernel, dim3(blocks_of(f.lattice, 256)), dim3(256), 0, stream, f);
}

void launch_adaptive_rays(const RenderArgs& a, const AdaptiveFrame& f, int n, int cols, float* rays, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(adaptive_rays_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, stream, a, f.list, n, cols, rays);
}

void launch_adaptive_classify(const AdaptiveFrame& f, hipStream_t stream) {
    if (f.pixels <= 0) return;
    hipLaunchKernelGGL(adaptive_cells_kernel, dim3(blocks_of((int64_t)f.n_poses * f.h.cells * f.w.cells, 256)), dim3(256), 0, stream, f);
    hipLaunchKernelGGL(adaptive_kinds_kernel, dim3(blocks_of(f.pixels, 256)), dim3(256), 0, stream, f);
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, f.counts, f.pixels, f.total);
    hipLaunchKernelGGL(adaptive_emit_kernel, dim3(blocks_of(f.pixels, 256)), dim3(256), 0, stream, f);
}

void launch_adaptive_compose(const AdaptiveFrame& f, hipStream_t stream) {
    if (f.pixels <= 0) return;
    hipLaunchKernelGGL(adaptive_compose_kernel, dim3(blocks_of(f.pixels, kComposeThreads)), dim3(kComposeThreads), 0, stream, f);
}

}  // namespace nwe
