// MFMA render kernel (NWE_PREC_F16X3 / NWE_PREC_F16X1) for gfx950.
//
// The whole path of nerf/inference/nerf_replica_inference_handler.py:203-277 in one launch: rays,
// coarse depths, gamma(x)/gamma(d), coarse MLP, compositing, inverse-CDF importance sampling + merge,
// fine MLP, compositing.  Nothing but the per-ray results reaches HBM.
//
// Work decomposition:
//   * a packet = 32 rays (lane&31 = ray, both lane halves carry the ray state) whose samples are walked in
//     lock step; a 256-thread workgroup = 4 waves sharing one weight stream, either four packets (one per
//     wave) or one packet with its samples dealt to the four waves (render_mfma_kernel, SPLIT).
//   * the MLP is evaluated transposed, H_out^T[feature, ray] = W[feature, k] . H_in^T[k, ray], with
//     v_mfma_f32_32x32x16_f16: A = weight tile (from LDS), B = activations.  The 32x32 result has the
//     ray on the lane and the features in the 16 registers, which is exactly the B-operand layout of
//     the next layer (k order permuted; the packer permutes the weight columns to match), so
//     activations never leave the register file between layers.
//   * fp32-grade results from fp16 MFMA: every operand is split x = hi + lo (both fp16) and
//     W.x ~= Whi.xhi + Wlo.xhi + Whi.xlo, three MFMAs into one fp32 accumulator.  Weights are scaled
//     by a power of two at pack time so that their lo halves are fp16-normal; activation lo halves may
//     be fp16-subnormal (absolute error <= 3e-8), which the matrix core honours (nwe_selftest).
//   * weights stream from L2 through two LDS buffers with LDS-DMA (global_load_lds_dwordx4), one chunk
//     = one 32-row tile of a layer (hi/lo tile per 16-wide k-step), issued one chunk ahead, piece by
//     piece between the MFMAs of the current tile.
//   * one wave per SIMD: the wave's own instruction issue is the scarce resource next to the matrix
//     pipe, so everything around the MFMAs is kept to a handful of instructions per MFMA and placed
//     statically in the gaps between them: the epilogue of tile t (bias, ReLU, hi/lo split) runs in
//     stages between the MFMAs of tile t+1 (EpiPlan), LDS-DMA addressing is scalar and each piece has a
//     gap of its own (DmaPlan), the A fragments are read three k-steps ahead.
//   * template switches of render_mfma_kernel: X3 (three split products / single fp16 product), SPLIT (one packet per
//     workgroup, samples dealt to the waves), FORM (nwe_host.h: kFormFolded = _feature_linear multiplied into the view layer by
//     the packer and _alpha_linear a dot product, the product path - "FOLD" below; kFormReference = every layer a tile of the
//     stream; kFormNoViewDirs = trunk + _output_linear), LEAN (only rgb / depth / acc of pinhole views: every other pointer
//     compile-time null, no register spills).
// The templates live in nwe_mfma_config.h (shared types, tuning switches), nwe_mfma_epilogue.h, nwe_mfma_stream.h,
// nwe_mfma_eval.h and nwe_mfma_render.h (the render kernels, their variants and the one launcher) and nwe_mfma_query.h;
// nwe_mfma_inst.hip instantiates them for the shapes of nwe_mfma_shapes.h, one translation unit per group of shapes and kernel
// variant (in parallel; the Makefile generates the units), nwe_kernel_mfma.hip plans the launches and dispatches through one
// table of the shapes.
#pragma once
#include "nwe_mfma_render.h"
#include "nwe_mfma_shapes.h"
