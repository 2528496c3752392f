// The multi-level adaptive frame (include/nwe.h, nwe_render_adaptive_levels): nested lattices from a coarse spacing down to k, a
// render pass per level for the cells whose corners disagree, whole pixels only behind the finest level, the rest interpolated in
// the coarsest flat cell that holds it.  Plain HIP, no MFMA here: the networks run in the render kernels, on the pixel lists this
// unit writes, between its stages.  A translation unit of its own: every other code object keeps the kernels it had - the scan
// below is a second copy of nwe_adaptive.hip's for that reason.  The lattice arithmetic is nwe_plan.h's.
#include "nwe_host.h"

namespace nwe {

// a + (b - a) * f: three fp32 operations, each rounded on its own (adaptive_lerp of nwe_adaptive.hip; -ffp-contract=off here as well)
__device__ __forceinline__ float levels_lerp(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), f)); }

// Pixel p of the call: its pose and its local row and column
struct LevelsPixel { int pose, r, w; };
__device__ __forceinline__ LevelsPixel levels_pixel(const AdaptiveLevelsFrame& f, int p) {
    const int per_pose = f.h[0].len * f.w[0].len;
    LevelsPixel x;
    x.pose = p / per_pose;
    const int rem = p - x.pose * per_pose;
    x.r = rem / f.w[0].len; x.w = rem - x.r * f.w[0].len;
    return x;
}
__device__ __forceinline__ int levels_pixel_at(const AdaptiveLevelsFrame& f, int pose, int r, int w) { return (pose * f.h[0].len + r) * f.w[0].len + w; }
__device__ __forceinline__ int levels_cell_at(const AdaptiveLevelsFrame& f, int l, int pose, int ci, int cj) {
    return (pose * f.h[l].cells + ci) * f.w[l].cells + cj;
}

// lattice.  One thread per pixel of the level 0 lattice, in the order [pose][i][j], which ascends: its pixel and that pixel's slot.
__global__ void __launch_bounds__(256) adaptive_levels_lattice_kernel(AdaptiveLevelsFrame f, int lattice) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lattice) return;
    const int per_pose = f.h[0].n * f.w[0].n;
    const int pose = t / per_pose, rem = t - pose * per_pose;
    const int i = rem / f.w[0].n, j = rem - i * f.w[0].n;
    const int p = levels_pixel_at(f, pose, adaptive_entry(f.h[0], i), adaptive_entry(f.w[0], j));
    f.list[t] = p;
    f.slot[p] = t;
}

// cells.  One thread per cell of level l: inactive unless l == 0 or its parent is busy; an active cell is busy unless every pair
// of its corners agrees (adaptive_cells_kernel's rule: !(|a - b| <= tol), a NaN difference is busy).  The corners are found by
// pixel, in whatever pass rendered them; the busy cells are counted with one atomic per wave at the most.
__global__ void __launch_bounds__(256) adaptive_levels_cells_kernel(AdaptiveLevelsFrame f, int l) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const AdaptiveAxis &h = f.h[l], &w = f.w[l];
    const int per_pose = h.cells * w.cells;
    bool busy = false;
    if (t < f.n_poses * per_pose) {
        const int pose = t / per_pose, rem = t - pose * per_pose;
        const int ci = rem / w.cells, cj = rem - ci * w.cells;
        bool active = true;
        if (l > 0) {
            const int pi = adaptive_cell(f.h[l - 1], adaptive_entry(h, ci)), pj = adaptive_cell(f.w[l - 1], adaptive_entry(w, cj));
            active = f.state[l - 1][levels_cell_at(f, l - 1, pose, pi, pj)] == kAdaptiveBusy;
        }
        uint8_t state = kAdaptiveInactive;
        if (active) {
            const int i1 = min(ci + 1, h.n - 1), j1 = min(cj + 1, w.n - 1);
            const int h0 = adaptive_entry(h, ci), h1 = adaptive_entry(h, i1), w0 = adaptive_entry(w, cj), w1 = adaptive_entry(w, j1);
            const int c[4] = {f.slot[levels_pixel_at(f, pose, h0, w0)], f.slot[levels_pixel_at(f, pose, h0, w1)],
                              f.slot[levels_pixel_at(f, pose, h1, w0)], f.slot[levels_pixel_at(f, pose, h1, w1)]};
            bool flat = c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[3] >= 0;   // by the rule they are rendered; never read in front of the outputs
            if (flat) {
                float v[4][5];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q][0] = f.c_rgb[(int64_t)c[q] * 3]; v[q][1] = f.c_rgb[(int64_t)c[q] * 3 + 1]; v[q][2] = f.c_rgb[(int64_t)c[q] * 3 + 2];
                    v[q][3] = f.c_acc[c[q]]; v[q][4] = f.c_depth[c[q]];
                }
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = p + 1; q < 4; ++q)
#pragma unroll
                        for (int e = 0; e < 5; ++e) flat = flat && fabsf(__fsub_rn(v[p][e], v[q][e])) <= (e < 4 ? f.tol_rgb : f.tol_depth);
            }
            state = flat ? kAdaptiveFlat : kAdaptiveBusy;
            busy = !flat;
        }
        f.state[l][t] = state;
    }
    const unsigned long long votes = __ballot(busy);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(f.words + 2 * l + 1, (uint32_t)__popcll(votes));
}

// mark.  One thread per pixel: whether it belongs to pass l + 1 - not rendered yet, on the lattice of level l + 1 (behind the finest
// level: any pixel), and in the closed rectangle of a busy cell of level l.  The cells whose rectangle holds the pixel are its own
// and, where it lies on the lattice row (column) that opens that cell, the one before it (adaptive_kinds_kernel): four at the most.
// A member's slot becomes kLevelsMember until emit gives it its place.
constexpr int32_t kLevelsMember = -2;
__global__ void __launch_bounds__(256) adaptive_levels_mark_kernel(AdaptiveLevelsFrame f, int l) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= f.pixels) return;
    bool member = false;
    if (f.slot[p] < 0) {
        const LevelsPixel x = levels_pixel(f, p);
        if (l == f.levels - 1 || (adaptive_on_lattice(f.h[l + 1], x.r) && adaptive_on_lattice(f.w[l + 1], x.w))) {
            const AdaptiveAxis &h = f.h[l], &w = f.w[l];
            const int ci = adaptive_cell(h, x.r), cj = adaptive_cell(w, x.w);
            const int ci0 = ci > 0 && adaptive_entry(h, ci) == x.r ? ci - 1 : ci;
            const int cj0 = cj > 0 && adaptive_entry(w, cj) == x.w ? cj - 1 : cj;
            const uint8_t* state = f.state[l] + (int64_t)x.pose * h.cells * w.cells;
            for (int i = ci0; i <= ci; ++i)
                for (int j = cj0; j <= cj; ++j) member = member || state[i * w.cells + j] == kAdaptiveBusy;
        }
        if (member) f.slot[p] = kLevelsMember;
    }
    f.counts[p] = member ? 1u : 0u;
}

// scan.  adaptive_scan_kernel of nwe_adaptive.hip, copied: one workgroup, counts[] becomes its exclusive scan in place, tile by tile
// of kLevelsScanThreads elements with the running sum carried in a register every thread holds; *total = the sum (at most 2^24).
constexpr int kLevelsScanThreads = 1024;
__global__ void __launch_bounds__(kLevelsScanThreads) adaptive_levels_scan_kernel(uint32_t* __restrict__ counts, int count, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[kLevelsScanThreads / 64];
    __shared__ uint32_t s_tile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (int base = 0; base < count; base += kLevelsScanThreads) {   // block-uniform trip count: the barriers are met by every thread
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
            const uint32_t w = lane < kLevelsScanThreads / 64 ? s_wave[lane] : 0u;
            uint32_t wi = w;
#pragma unroll
            for (int off = 1; off < kLevelsScanThreads / 64; off <<= 1) {
                const uint32_t up = __shfl_up(wi, off);
                if (lane >= off) wi += up;
            }
            if (lane < kLevelsScanThreads / 64) s_wave[lane] = wi - w;   // exclusive over the waves
            if (lane == kLevelsScanThreads / 64 - 1) s_tile = wi;
        }
        __syncthreads();
        if (i < count) counts[i] = carry + s_wave[wave] + incl - v;
        carry += s_tile;
        __syncthreads();   // s_wave and s_tile are rewritten by the next tile
    }
    if (tid == 0) *total = carry;
}

// emit.  One thread per pixel: a member of the pass goes to its place in the list - counts[p] < the members <= the list's room
// (AdaptiveLevelsPlan::list) - and its slot is its place in the compact outputs, first + counts[p] < pixels.
__global__ void __launch_bounds__(256) adaptive_levels_emit_kernel(AdaptiveLevelsFrame f, int first) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= f.pixels) return;
    if (f.slot[p] == kLevelsMember) {
        const int at = (int)f.counts[p];
        f.list[at] = p;
        f.slot[p] = first + at;
    }
}

// compose.  One thread per pixel of the call, one wave per workgroup (the flags and each level's interpolated count take one atomic
// per wave at the most): a pixel with a slot is copied from the compact outputs, one without walks the levels to its first flat
// own cell and is mixed from the slots of that cell's corners - along w on the top and on the bottom pair, then along h.
constexpr int kLevelsComposeThreads = 64;
__global__ void __launch_bounds__(kLevelsComposeThreads) adaptive_levels_compose_kernel(AdaptiveLevelsFrame f) {
    const int p = blockIdx.x * kLevelsComposeThreads + threadIdx.x;
    uint32_t flags = p == 0 ? *f.render_flags & (NWE_FLAG_RGB | NWE_FLAG_DEPTH | NWE_FLAG_ACC) : 0u;
    int at_level = -1;   // of an interpolated pixel
    if (p < f.pixels) {
        const LevelsPixel x = levels_pixel(f, p);
        const int c = f.slot[p];
        float v[5];   // r, g, b, depth, acc
        uint8_t kind, level = 0;
        if (c >= 0) {
            for (int i = 1; i <= f.levels; ++i) level += c >= f.base[i] ? 1 : 0;   // its pass
            kind = level == 0 ? 0 : 1;
            v[0] = f.c_rgb[(int64_t)c * 3]; v[1] = f.c_rgb[(int64_t)c * 3 + 1]; v[2] = f.c_rgb[(int64_t)c * 3 + 2];
            v[3] = f.c_depth[c]; v[4] = f.c_acc[c];
        } else {
            kind = 2;
            int l = 0;
            for (; l < f.classified - 1; ++l)
                if (f.state[l][levels_cell_at(f, l, x.pose, adaptive_cell(f.h[l], x.r), adaptive_cell(f.w[l], x.w))] == kAdaptiveFlat) break;
            const AdaptiveAxis h = f.h[l], w = f.w[l];
            const int ci = adaptive_cell(h, x.r), cj = adaptive_cell(w, x.w);
            const int i1 = min(ci + 1, h.n - 1), j1 = min(cj + 1, w.n - 1);
            const int h0 = adaptive_entry(h, ci), h1 = adaptive_entry(h, i1), w0 = adaptive_entry(w, cj), w1 = adaptive_entry(w, j1);
            const float fy = h1 == h0 ? 0.f : __fdiv_rn((float)(x.r - h0), (float)(h1 - h0));
            const float fx = w1 == w0 ? 0.f : __fdiv_rn((float)(x.w - w0), (float)(w1 - w0));
            // by the rule the corners of a classified cell are rendered; never read in front of the outputs
            const int c00 = max(f.slot[levels_pixel_at(f, x.pose, h0, w0)], 0), c01 = max(f.slot[levels_pixel_at(f, x.pose, h0, w1)], 0);
            const int c10 = max(f.slot[levels_pixel_at(f, x.pose, h1, w0)], 0), c11 = max(f.slot[levels_pixel_at(f, x.pose, h1, w1)], 0);
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                const float* src = e < 3 ? f.c_rgb + e : e == 3 ? f.c_depth : f.c_acc;
                const int step = e < 3 ? 3 : 1;
                const float top = levels_lerp(src[(int64_t)c00 * step], src[(int64_t)c01 * step], fx);
                const float bottom = levels_lerp(src[(int64_t)c10 * step], src[(int64_t)c11 * step], fx);
                v[e] = levels_lerp(top, bottom, fy);
            }
            flags |= ((bad(v[0]) || bad(v[1]) || bad(v[2])) ? NWE_FLAG_RGB : 0) | (bad(v[3]) ? NWE_FLAG_DEPTH : 0) | (bad(v[4]) ? NWE_FLAG_ACC : 0);
            level = (uint8_t)l;
            at_level = l;
        }
        if (f.rgb) { f.rgb[(int64_t)p * 3] = v[0]; f.rgb[(int64_t)p * 3 + 1] = v[1]; f.rgb[(int64_t)p * 3 + 2] = v[2]; }
        if (f.depth) f.depth[p] = v[3];
        if (f.acc) f.acc[p] = v[4];
        if (f.kind) f.kind[p] = kind;
        if (f.level) f.level[p] = level;
    }
    for (int l = 0; l < f.classified; ++l) {   // launch-uniform trip count
        const unsigned long long votes = __ballot(at_level == l);
        if (threadIdx.x == 0 && votes) atomicAdd(f.interp + l, (uint32_t)__popcll(votes));
    }
    if (f.flags) {   // one atomic per wave at the most
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) flags |= __shfl_xor(flags, off);
        if (threadIdx.x == 0 && flags) atomicOr(f.flags, flags);
    }
}

static unsigned blocks_of(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

void launch_adaptive_levels_lattice(const AdaptiveLevelsFrame& f, int lattice, hipStream_t stream) {
    if (lattice <= 0) return;
    hipLaunchKernelGGL(adaptive_levels_lattice_kernel, dim3(blocks_of(lattice, 256)), dim3(256), 0, stream, f, lattice);
}

void launch_adaptive_levels_classify(const AdaptiveLevelsFrame& f, int l, int first, hipStream_t stream) {
    if (f.pixels <= 0) return;
    hipLaunchKernelGGL(adaptive_levels_cells_kernel, dim3(blocks_of((int64_t)f.n_poses * f.h[l].cells * f.w[l].cells, 256)), dim3(256), 0, stream, f, l);
    hipLaunchKernelGGL(adaptive_levels_mark_kernel, dim3(blocks_of(f.pixels, 256)), dim3(256), 0, stream, f, l);
    hipLaunchKernelGGL(adaptive_levels_scan_kernel, dim3(1), dim3(kLevelsScanThreads), 0, stream, f.counts, f.pixels, f.words + 2 * l);
    hipLaunchKernelGGL(adaptive_levels_emit_kernel, dim3(blocks_of(f.pixels, 256)), dim3(256), 0, stream, f, first);
}

void launch_adaptive_levels_compose(const AdaptiveLevelsFrame& f, hipStream_t stream) {
    if (f.pixels <= 0) return;
    hipLaunchKernelGGL(adaptive_levels_compose_kernel, dim3(blocks_of(f.pixels, kLevelsComposeThreads)), dim3(kLevelsComposeThreads), 0, stream, f);
}

}  // namespace nwe
