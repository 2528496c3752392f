// Instantiations of the MFMA tail kernel (split items in the packets launch's tail), group A of nwe_mfma_shapes.h.
#include "nwe_mfma_kernels.h"

namespace nwe {
NWE_SHAPES_A(NWE_SHAPE_TAIL_LAUNCHER)
}  // namespace nwe
