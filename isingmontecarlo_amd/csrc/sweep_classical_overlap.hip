// Launcher of the classical overlap kernel (sse_classical_overlap.hip.h).
#include "sse_classical_overlap.hip.h"
namespace sse {
hipError_t launch_classical_overlaps(hipStream_t stream, const CmcDev &D, const CmcPtDev &P, const CmcOvDev &O, int32_t *q_row, int32_t *ql_row) {
    const uint64_t items = (uint64_t)O.G * O.P * P.T;
    if (O.K < 2u || items == 0u || (uint64_t)O.G * O.K != P.C || (uint64_t)P.C * P.T != D.R || items > CMC_OV_MAX_ITEMS || !O.hq || !O.hl) return hipErrorInvalidValue;
    hipLaunchKernelGGL(classical_overlap_kernel, dim3((uint32_t)((items + CMC_OV_WAVES - 1u) / CMC_OV_WAVES)), dim3(64u * CMC_OV_WAVES), 0, stream, D, P, O, q_row, ql_row);
    return hipGetLastError();
}
} // namespace sse
