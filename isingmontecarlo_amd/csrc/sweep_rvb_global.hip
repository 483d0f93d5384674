// Instantiations of sse::sweep_kernel<16, 4, MODE, 0, SSE_PASSES_RVB_G>: the RVB sweep alone with its per-variable tables (constant-op
// starts and positions, variables without constant ops, variable -> sub-variable, edge -> boundary-bond entry) in a per-replica HBM
// scratch (DevBatch::rvb_tbl) instead of LDS — any model, whatever its size or its number of constant ops (ISINGMC_CFG_RVB_GLOBAL_TABLES).
// Two bond decodes: the LDS edge table (MODE 1) and the general 16-byte records (every other model: the host allocates the records of every
// bond-table row in every mode, the +-J decode's batches included).
#include "sse_sweep.hip.h"
namespace sse {
hipError_t launch_rvb_global(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    if (!B.rvb_tbl || c.W != 16 || c.K != 4 || c.passes != SSE_PASSES_RVB_G) return hipErrorInvalidValue;
    if (c.mode == SSE_MODE_LDS_EDGES) return launch_one<16, 4, SSE_MODE_LDS_EDGES, 0, SSE_PASSES_RVB_G>(c, B, A);
    return launch_one<16, 4, SSE_MODE_GENERAL, 0, SSE_PASSES_RVB_G>(c, B, A);
}
} // namespace sse
