// Packets of 8x4 pixel blocks: which pixel a ray index of a blocked call names.  Plain C++, no device API: the planner
// (nwe_plan.cpp) and the render kernels (nwe_mfma_render_item.h) compile this one function, and nwe_debug_packet_pixels
// (include/nwe.h) hands it to the tests.
//
// A ray packet is 32 consecutive ray indices, and the hollow path of mlp_eval pays where all 32 rays of a packet have no density
// at a sample.  Density is a property of space, so a compact set of pixels is hollow more often than a 32x1 strip of an image
// row.  In a blocked call (plan_call: CallPlan::blocks) ray index j of the call therefore names pixel pi(j) of the call's
// [pose][row][column] raster, and pi maps every aligned group of 32 indices onto one block of 8 columns x 4 rows:
//   a band = 4 image rows = 4 W indices; inside a band, index r belongs to block r / 32 (blocks left to right) and is pixel
//   in = r % 32 of it, row in >> 3 and column in & 7 of the block.
// The rows rendered per pose are a multiple of 4, so a band never straddles two poses, and W is a multiple of 8, so a block
// never straddles two bands.  pi is a bijection of [0, n_rays) onto itself; no output depends on which rays share a packet.
#pragma once

#ifdef __HIPCC__
#define NWE_HOST_DEVICE __host__ __device__
#else
#define NWE_HOST_DEVICE
#endif

namespace nwe {

constexpr int kBlockW = 8, kBlockH = 4;   // kBlockW * kBlockH == kRaysPerWave (nwe_plan.h asserts it)

// RenderArgs::ray_cols of a blocked launch carries this bit (a pinhole call reads no ray table, so nothing else reads the word)
constexpr int kPacketBlocksBit = 1 << 30;

NWE_HOST_DEVICE inline bool packet_blocks_fit(int rows, int W) { return rows > 0 && W > 0 && rows % kBlockH == 0 && W % kBlockW == 0; }

// pi(j) for a frame W pixels wide; j < 2^31 (the ABI's bound on the rays of a call)
NWE_HOST_DEVICE inline int packet_block_pixel(int j, int W) {
    const int band_rays = kBlockH * W;
    const int r = j % band_rays;
    const int block = r / (kBlockW * kBlockH), in = r % (kBlockW * kBlockH);
    return j - r + (in / kBlockW) * W + block * kBlockW + in % kBlockW;
}

}  // namespace nwe
