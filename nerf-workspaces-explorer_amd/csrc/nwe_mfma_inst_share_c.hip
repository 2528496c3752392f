// Instantiations of the MFMA render kernel with the shared coarse pass, group C of nwe_mfma_shapes.h.
#include "nwe_mfma_kernels.h"

namespace nwe {
NWE_SHAPES_C(NWE_SHAPE_SHARE_LAUNCHER)
}  // namespace nwe
