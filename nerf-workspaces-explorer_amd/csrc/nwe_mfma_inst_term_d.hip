// Instantiations of the MFMA render kernel with early ray termination, group D of nwe_mfma_shapes.h.
#include "nwe_mfma_kernels.h"

namespace nwe {
NWE_SHAPES_D(NWE_SHAPE_TERM_LAUNCHER)
}  // namespace nwe
