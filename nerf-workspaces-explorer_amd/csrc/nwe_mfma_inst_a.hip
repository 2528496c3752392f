// Instantiations of the MFMA render kernel, group A of nwe_mfma_shapes.h.
#include "nwe_mfma_kernels.h"

namespace nwe {
NWE_SHAPES_A(NWE_SHAPE_LAUNCHER)
}  // namespace nwe
