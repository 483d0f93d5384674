// Instantiations of sse::sweep_kernel<16, 4, MODE, 0, SSE_PASSES_RVB_G>: the RVB sweep alone with its per-variable tables (constant-op
// starts and positions, variables without constant ops, variable -> sub-variable, edge -> boundary-bond entry) in a per-replica HBM
// scratch (DevBatch::rvb_tbl) instead of LDS — any model, whatever its size or its number of constant ops (ISINGMC_CFG_RVB_GLOBAL_TABLES).
// Two bond decodes: the LDS edge table (MODE 1) and the general 16-byte records (every other model: the host allocates the records of every
// bond-table row in every mode, the +-J decode's batches included).
#include "sse_device.hip.h"
namespace sse {
size_t rvb_global_lds_words(uint32_t N, uint32_t nwords, uint32_t ledges, uint32_t areas) {
    (void)N; // (Lds<16>::carve with the tables in HBM: the bit arrays, round buffers, misc, chunk counters and edge table; then rvb_carve<16, true>)
    const size_t o_cur = (size_t)nwords * 2 + 4 * 16 + 16 + 2 * SSE_MAX_CHUNKS + ledges;
    return o_cur + 2 + rvb_global_fixed_words() + (size_t)areas * SSE_RVB_SLOT_WORDS;
}
hipError_t launch_rvb_global(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    if (!B.rvb_tbl || c.W != 16 || c.K != 4 || c.passes != SSE_PASSES_RVB_G) return hipErrorInvalidValue;
    if (c.mode == SSE_MODE_LDS_EDGES) return launch_one<16, 4, SSE_MODE_LDS_EDGES, 0, SSE_PASSES_RVB_G>(c, B, A);
    return launch_one<16, 4, SSE_MODE_GENERAL, 0, SSE_PASSES_RVB_G>(c, B, A);
}
} // namespace sse
