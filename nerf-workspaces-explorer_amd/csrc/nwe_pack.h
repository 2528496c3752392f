// The plain descriptors of a packed network, shared with the launchers (nwe_host.h), and the host-side weight packers of
// both kernels: pure arithmetic, plain C++ without HIP (nwe_pack.cpp).
#pragma once
#include <stdint.h>
#include <vector>

namespace nwe {

// ---- fp32 kernel: transposed weights Wt[k][n] + bias in one float blob ------------------------
struct LayerF32 {
    int K, N;
    int64_t wt_off, b_off;  // float offsets into the blob
};
struct NetF32 {
    const float* blob;
    int D, W, in_xyz, in_dir, skip;
    LayerF32 pts[16];
    LayerF32 views, feature, alpha, rgb;
    LayerF32 output;     // use_view_dirs=False (in_dir == 0): _output_linear [out_ch, W] instead of the four heads
    int out_ch;
};
constexpr int kMaxDepth = 16;

// ---- MFMA kernel: a stream of 1-KiB tiles in consumption order (DESIGN.md "weight stream") -----
struct NetMfma {
    const uint8_t* stream;  // device: 1-KiB tiles, (hi, lo) per k-step, chunk after chunk
    const float* bias;      // device: 32 floats per chunk (tile row i -> bias of the weight row it holds); folded: then W/32 + 1 dot
                            // rows (the weights of _alpha_linear in the row order of the last trunk layer's tiles, and its bias)
    int n_tiles, n_chunks;
    float inv_scale;        // weights are stored multiplied by 1/inv_scale (a power of two)
    int D, W, skip;
    int form;               // Form: which formulation of the network the stream holds
    int colour_skip;        // set per launch, never packed (nwe_debug_set_colour_skip): the lean kernels may leave out the colour layers
                            // of a wave's evaluation whose 32 rays all have sigma <= 0 (mlp_eval: the hollow path)
};
constexpr int kTileBytes = 1024;

// The three formulations the MFMA kernel is instantiated for (template argument FORM of nwe_mfma_kernels.h; the shapes: nwe_mfma_shapes.h).
enum Form {
    kFormReference = 0,     // every layer of nerf_model.py:45-76 as a tile of the stream (selectable for comparison)
    kFormFolded = 1,        // the product path: _feature_linear multiplied into the view layer at pack time, _alpha_linear a dot product
    kFormNoViewDirs = 2     // use_view_dirs=False (nerf_model.py:41-43,78-79): trunk, then the rows rgb_raw(3), sigma_raw of _output_linear
};

struct NetShape {
    int D = 0, W = 0, in_xyz = 0, in_dir = 0, skip = -1, out_ch = 0;   // out_ch: use_view_dirs=False (in_dir == 0), rows of _output_linear
};

// What the packers make of a network, all of it in host memory (f32.blob stays null: the device side is the caller's).
struct Packed {
    std::vector<float> blob;       // fp32 kernel: per layer Wt[k][n] then bias
    NetF32 f32 = {};               // fp32 kernel: the layers' offsets into the blob
    std::vector<uint8_t> stream;   // MFMA kernel: 1-KiB tiles in consumption order
    std::vector<float> bias_tab;   // MFMA kernel: 32 floats per chunk, then (folded) the dot rows of _alpha_linear
    int n_chunks = 0;              // chunks of the stream = bias rows in front of the dot rows
    float w_scale = 1.f;           // power of two the packed weights are multiplied by
    bool colour_finite = false;    // folded MFMA stream: every value the colour layers hold AS PACKED is finite - the folded view layer
                                   // formed in fp64 with its gamma(d) columns and the rgb head, scaled and rounded to fp16, and both
                                   // biases rounded to fp32.  Then a sample of zero weight contributes 0 x (finite colour) = 0 whatever
                                   // its colour is, the condition of the hollow path (mlp_eval).  Not part of stream or bias table.
};

// w[i], b[i]: layer i as [out, in] and [out]; D trunk layers, then views, feature, alpha, rgb or (in_dir == 0) _output_linear
void pack_f32(Packed& p, const NetShape& n, const float* const* w, const float* const* b);
void pack_mfma(Packed& p, const NetShape& n, int form, const float* const* w, const float* const* b);   // form: Form
int64_t algo_flops(const NetShape& n);

}  // namespace nwe
