// The explicit instantiations of the MFMA kernels: ONE unit of them per compilation, chosen on the command line (Makefile).
//   -DNWE_INST_GROUP=NWE_SHAPES_A ... _F   the group of shapes (nwe_mfma_shapes.h)
//   -DNWE_INST_VARIANT=kVariantPlain | kVariantTerm | kVariantShare | kVariantOcc | kVariantTail | kVariantList   the render kernels of that variant, or
//   -DNWE_INST_QUERY                       the query kernels, or
//   -DNWE_INST_QUERY_COUNTED               their counted forms (units of their own: the query units hold what they held)
//   -DNWE_ONE_KERNEL=true|false            instead of all three: the headline kernel alone, folded or not (`make one`)
#include "nwe_mfma_kernels.h"
#include "nwe_mfma_query.h"

namespace nwe {
#if defined(NWE_ONE_KERNEL)
template __global__ void render_mfma_kernel<256, 8, 4, true, false, NWE_ONE_KERNEL, true>(RenderArgs, NetMfma, NetMfma);
#elif defined(NWE_INST_QUERY)
NWE_INST_GROUP(NWE_SHAPE_QUERY_LAUNCHER)
#elif defined(NWE_INST_QUERY_COUNTED)
NWE_INST_GROUP(NWE_SHAPE_QUERY_COUNTED_LAUNCHER)
#else
#define NWE_INST(W_, D_, SKIP_, FORM_) NWE_SHAPE_LAUNCHER(W_, D_, SKIP_, FORM_, NWE_INST_VARIANT)
NWE_INST_GROUP(NWE_INST)
#endif
}  // namespace nwe
