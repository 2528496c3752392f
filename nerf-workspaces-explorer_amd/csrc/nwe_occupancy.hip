// The kernels of nwe_build_occupancy (include/nwe.h): the probe points of a chunk of cells, their sigma reduced to the grid's
// bits, the dilation.  A translation unit of its own: the code object of nwe_abi.hip keeps the kernels it had.
#include "nwe_host.h"

namespace nwe {

// Probe point j = (jx * probes + jy) * probes + jz of cell `first + c`: along an axis ((float)i + ((float)j + 0.5f) / probes) *
// step + lo, every operation rounded to fp32 on its own.  points: [n_cells * probes^3, 3], cell-major.
__global__ void occ_probe_points_kernel(OccBuild b, int64_t first, int n_cells, float* __restrict__ points) {
    const int per_cell = b.probes * b.probes * b.probes;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_cells * per_cell) return;
    const int64_t cell = first + i / per_cell;
    const int j = (int)(i % per_cell);
    const int idx[3] = {(int)(cell / ((int64_t)b.res[1] * b.res[2])), (int)((cell / b.res[2]) % b.res[1]), (int)(cell % b.res[2])};
    const int sub[3] = {j / (b.probes * b.probes), (j / b.probes) % b.probes, j % b.probes};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f = __fadd_rn((float)idx[c], __fdiv_rn(__fadd_rn((float)sub[c], 0.5f), (float)b.probes));
        points[i * 3 + c] = __fadd_rn(__fmul_rn(f, b.step[c]), b.lo[c]);
    }
}

// One thread per cell of the chunk: occupied if any of its probes^3 values is > threshold or not finite; an occupied cell's
// bit is set with an atomic OR (32 cells share a word, and so do the networks and the chunks of a build).
__global__ void occ_reduce_bits_kernel(const float* __restrict__ sigma, int64_t first, int n_cells, int per_cell, float threshold,
                                       uint32_t* __restrict__ bits) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    bool occupied = false;
    for (int j = 0; j < per_cell; ++j) {
        const float v = sigma[(int64_t)c * per_cell + j];
        occupied = occupied || v > threshold || bad(v);
    }
    const int64_t cell = first + c;
    if (occupied) atomicOr(bits + (cell >> 5), 1u << (cell & 31));
}

// One step of the dilation with the 3 x 3 x 3 box: a cell of dst is occupied if any cell of src within one cell of it, inside
// the grid, is.  One thread per word of dst, which it alone writes.
__global__ void occ_dilate_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int rx, int ry, int rz, int64_t n_cells) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w * 32 >= n_cells) return;
    uint32_t word = 0;
    for (int bit = 0; bit < 32; ++bit) {
        const int64_t cell = w * 32 + bit;
        if (cell >= n_cells) break;
        const int ix = (int)(cell / ((int64_t)ry * rz)), iy = (int)((cell / rz) % ry), iz = (int)(cell % rz);
        bool occupied = false;
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    const int x = ix + dx, y = iy + dy, z = iz + dz;
                    if (x < 0 || x >= rx || y < 0 || y >= ry || z < 0 || z >= rz) continue;
                    const int64_t n = ((int64_t)x * ry + y) * rz + z;
                    occupied = occupied || ((src[n >> 5] >> (n & 31)) & 1u);
                }
        if (occupied) word |= 1u << bit;
    }
    dst[w] = word;
}

void launch_occ_probe_points(const OccBuild& b, int64_t first, int n_cells, float* points, hipStream_t stream) {
    const int64_t n_points = (int64_t)n_cells * b.probes * b.probes * b.probes;
    hipLaunchKernelGGL(occ_probe_points_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, stream, b, first, n_cells, points);
}

void launch_occ_reduce_bits(const float* sigma, int64_t first, int n_cells, int per_cell, float threshold, uint32_t* bits, hipStream_t stream) {
    hipLaunchKernelGGL(occ_reduce_bits_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, stream, sigma, first, n_cells, per_cell,
                       threshold, bits);
}

void launch_occ_dilate(const uint32_t* src, uint32_t* dst, const int* res, hipStream_t stream) {
    const int64_t cells = (int64_t)res[0] * res[1] * res[2], words = (cells + 31) / 32;
    hipLaunchKernelGGL(occ_dilate_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, src, dst, res[0], res[1], res[2], cells);
}

}  // namespace nwe
