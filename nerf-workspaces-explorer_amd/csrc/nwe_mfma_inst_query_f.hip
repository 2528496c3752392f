// Instantiations of the MFMA query kernel (run_network at arbitrary points), group F of nwe_mfma_shapes.h.
#include "nwe_mfma_query.h"
#include "nwe_mfma_shapes.h"

namespace nwe {
NWE_SHAPES_F(NWE_SHAPE_QUERY_LAUNCHER)
}  // namespace nwe
