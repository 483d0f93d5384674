// Instantiations of sse::sweep_fast_kernel (sse_fast.hip.h): the diagonal-pass launch of the headline geometry.
#include "sse_fast.hip.h"
#include "sse_launch.h"
namespace sse {
template <int K, int PHASE, bool F64>
static hipError_t launch_fast_one(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    return launch_lds(sweep_fast_kernel<K, PHASE, F64>, dim3(B.R), dim3(256), c.lds_bytes, c.stream, B, A);
}
uint32_t fast_max_vars() { return SSE_FAST_MAX_VARS; }
hipError_t launch_sweep_fast(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    if (c.W != 4 || c.mode != SSE_MODE_LDS_EDGES) return hipErrorInvalidValue;
    // the integer acceptance rule equals the oracle's f64 expressions while the cutoff stays within SSE_ACCEPT_MAX_DEN; a batch
    // that can grow beyond it keeps the f64 rounds
    const bool f64 = B.cap > SSE_ACCEPT_MAX_DEN;
    if (c.K == 4) {
        if (f64) return c.phase ? launch_fast_one<4, 1, true>(c, B, A) : launch_fast_one<4, 0, true>(c, B, A);
        return c.phase ? launch_fast_one<4, 1, false>(c, B, A) : launch_fast_one<4, 0, false>(c, B, A);
    }
    if (c.K == 2) return f64 ? launch_fast_one<2, 0, true>(c, B, A) : launch_fast_one<2, 0, false>(c, B, A);
    return hipErrorInvalidValue;
}
} // namespace sse
