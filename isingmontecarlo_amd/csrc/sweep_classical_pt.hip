// Launcher of the classical tempering kernel (sse_classical_pt.hip.h).
#include "sse_classical_pt.hip.h"
namespace sse {
hipError_t launch_classical_tempering(hipStream_t stream, const CmcDev &D, const CmcPtDev &P, uint64_t pt_step, double *energy_row, int32_t *mag_row) {
    if (P.T < 2u || P.C == 0u || (uint64_t)P.C * P.T != D.R) return hipErrorInvalidValue;
    const uint32_t waves = P.T < CMC_PT_MAX_WAVES ? P.T : CMC_PT_MAX_WAVES;
    hipLaunchKernelGGL(classical_tempering_kernel, dim3(P.C), dim3(64u * waves), 0, stream, D, P, pt_step, energy_row, mag_row);
    return hipGetLastError();
}
} // namespace sse
