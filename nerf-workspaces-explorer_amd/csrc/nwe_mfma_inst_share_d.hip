// Instantiations of the MFMA render kernel with the shared coarse pass, group D of nwe_mfma_shapes.h.
#include "nwe_mfma_kernels.h"

namespace nwe {
NWE_SHAPES_D(NWE_SHAPE_SHARE_LAUNCHER)
}  // namespace nwe
