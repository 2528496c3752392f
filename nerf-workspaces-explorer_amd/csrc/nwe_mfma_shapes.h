// The one list of network shapes (W, D, SKIP, FORM) the MFMA kernel is built for.  The explicit instantiations
// (nwe_mfma_inst_*.hip, one group each so that they compile in parallel), the dispatcher's declarations and lookup and
// mfma_supported() (nwe_kernel_mfma.hip) are all generated from it: a shape is supported exactly if it is instantiated.
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

// What an instantiation file compiles for a shape, and what the dispatcher declares: the launcher, and with it the shape's
// eight kernels (three-pass / single-pass, packets / sample-split, lean / full).
#define NWE_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_) \
    template void launch_one<W_, D_, SKIP_, FORM_>(RenderArgs, const NetMfma&, const NetMfma&, bool, bool, int64_t, int64_t, hipStream_t);
#define NWE_EXTERN_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_) extern NWE_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_)
// The launcher of the shape's four terminating kernels (early ray termination; lean, three-pass / single-pass, packets / sample
// split), in instantiation files of their own (nwe_mfma_inst_term_*.hip, the same groups).  Empty for kFormReference.
#define NWE_SHAPE_TERM_LAUNCHER(W_, D_, SKIP_, FORM_) \
    template void launch_one_term<W_, D_, SKIP_, FORM_>(RenderArgs, const NetMfma&, const NetMfma&, bool, bool, int64_t, int64_t, hipStream_t);
#define NWE_EXTERN_SHAPE_TERM_LAUNCHER(W_, D_, SKIP_, FORM_) extern NWE_SHAPE_TERM_LAUNCHER(W_, D_, SKIP_, FORM_)
// The launcher of the shape's four sharing kernels (shared coarse pass: producer and consumer are one instantiation; lean,
// three-pass / single-pass, packets / sample split), in files of their own (nwe_mfma_inst_share_*.hip).  Empty for kFormReference.
#define NWE_SHAPE_SHARE_LAUNCHER(W_, D_, SKIP_, FORM_) \
    template void launch_one_share<W_, D_, SKIP_, FORM_>(RenderArgs, const NetMfma&, const NetMfma&, bool, bool, int64_t, int64_t, hipStream_t);
#define NWE_EXTERN_SHAPE_SHARE_LAUNCHER(W_, D_, SKIP_, FORM_) extern NWE_SHAPE_SHARE_LAUNCHER(W_, D_, SKIP_, FORM_)
// The launcher of the shape's two tail kernels (a hybrid plan's split items in the packets launch's tail; lean, three-pass /
// single-pass, each holding both decompositions), in files of their own (nwe_mfma_inst_tail_*.hip).
#define NWE_SHAPE_TAIL_LAUNCHER(W_, D_, SKIP_, FORM_) \
    template void launch_one_tail<W_, D_, SKIP_, FORM_>(RenderArgs, const NetMfma&, const NetMfma&, bool, bool, int64_t, int64_t, hipStream_t);
#define NWE_EXTERN_SHAPE_TAIL_LAUNCHER(W_, D_, SKIP_, FORM_) extern NWE_SHAPE_TAIL_LAUNCHER(W_, D_, SKIP_, FORM_)
// The launcher of the shape's two query kernels (nwe_query_points: run_network at arbitrary points; three-pass / single-pass),
// in files of their own (nwe_mfma_inst_query_*.hip, the same groups): a shape is queryable exactly if it renders.
#define NWE_SHAPE_QUERY_LAUNCHER(W_, D_, SKIP_, FORM_) \
    template void launch_one_query<W_, D_, SKIP_, FORM_>(QueryArgs, const NetMfma&, bool, unsigned, hipStream_t);
#define NWE_EXTERN_SHAPE_QUERY_LAUNCHER(W_, D_, SKIP_, FORM_) extern NWE_SHAPE_QUERY_LAUNCHER(W_, D_, SKIP_, FORM_)
