// The one list of network shapes (W, D, SKIP, FORM) the MFMA kernel is built for.  The explicit instantiations
// (nwe_mfma_inst.hip, compiled once per group and kernel variant so that the units build in parallel) and the dispatcher's
// table, which mfma_supported() and every lookup read (nwe_kernel_mfma.hip), are generated from it: a shape is supported
// exactly if it is instantiated.
// Instantiated shapes: width 128 or 256, even depth 4 / 6 / 8 with the reference's skip connection (after layer 4 where
// that layer exists and feeds another trunk layer, nerf_model.py:13,58-59; none for depth 4), 63/27-wide encodings.
// The reference formulation (kFormReference) exists for the two BASELINE shapes only.
#pragma once

#define NWE_SHAPES_A(X) X(256, 8, 4, kFormFolded)   // the headline shape
#define NWE_SHAPES_B(X) X(256, 8, 4, kFormReference) X(256, 4, -1, kFormFolded)
#define NWE_SHAPES_C(X) X(256, 6, 4, kFormFolded) X(128, 4, -1, kFormReference)
#define NWE_SHAPES_D(X) X(128, 8, 4, kFormFolded) X(128, 6, 4, kFormFolded) X(128, 4, -1, kFormFolded)
// networks without view directions
#define NWE_SHAPES_E(X) X(256, 8, 4, kFormNoViewDirs) X(128, 4, -1, kFormNoViewDirs) X(128, 6, 4, kFormNoViewDirs)
#define NWE_SHAPES_F(X) X(256, 6, 4, kFormNoViewDirs) X(256, 4, -1, kFormNoViewDirs) X(128, 8, 4, kFormNoViewDirs)
#ifdef NWE_ONLY_HEADLINE   // diagnostic builds hold the first entry only
#define NWE_SHAPES(X) NWE_SHAPES_A(X)
#else
#define NWE_SHAPES(X) NWE_SHAPES_A(X) NWE_SHAPES_B(X) NWE_SHAPES_C(X) NWE_SHAPES_D(X) NWE_SHAPES_E(X) NWE_SHAPES_F(X)
#endif

// What an instantiation unit compiles for a shape and a variant (Variant, nwe_mfma_render.h), and what the dispatcher declares:
// the launcher, and with it the shape's kernels of that variant.  Empty where the shape does not have the variant.
#define NWE_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, VARIANT_) \
    template void launch_one<W_, D_, SKIP_, FORM_, VARIANT_>(RenderArgs, const NetMfma&, const NetMfma&, bool, bool, int64_t, int64_t, hipStream_t);
#define NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, VARIANT_) extern NWE_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, VARIANT_)
// The launcher of the shape's two query kernels (nwe_query_points: run_network at arbitrary points; three-pass / single-pass):
// a shape is queryable exactly if it renders.
#define NWE_SHAPE_QUERY_LAUNCHER(W_, D_, SKIP_, FORM_) \
    template void launch_one_query<W_, D_, SKIP_, FORM_>(QueryArgs, const NetMfma&, bool, unsigned, hipStream_t);
#define NWE_EXTERN_SHAPE_QUERY_LAUNCHER(W_, D_, SKIP_, FORM_) extern NWE_SHAPE_QUERY_LAUNCHER(W_, D_, SKIP_, FORM_)
// ... and of their counted forms (nwe_render_sparse_async: the point count is read on the device), in units of their own
#define NWE_SHAPE_QUERY_COUNTED_LAUNCHER(W_, D_, SKIP_, FORM_) \
    template void launch_one_query_counted<W_, D_, SKIP_, FORM_>(QueryArgs, const NetMfma&, const uint32_t*, bool, unsigned, hipStream_t);
#define NWE_EXTERN_SHAPE_QUERY_COUNTED_LAUNCHER(W_, D_, SKIP_, FORM_) extern NWE_SHAPE_QUERY_COUNTED_LAUNCHER(W_, D_, SKIP_, FORM_)
