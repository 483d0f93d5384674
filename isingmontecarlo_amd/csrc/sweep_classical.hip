// Launchers of the classical Monte Carlo kernels (sse_classical.hip.h).
#include "sse_classical.hip.h"
#include "sse_launch.h" // launch_lds, lds_bytes_of
#include "lds_plan.h"
namespace sse {
hipError_t launch_classical_steps(hipStream_t stream, const CmcDev &D, const CmcCarve &C, const CmcStepArgs &A) {
    if (C.W == 0u || C.W > 4u || D.R == 0u) return hipErrorInvalidValue;
    // per-replica couplings run the variant compiled for them: the shared-coupling kernel is the one it always was
    return launch_lds((D.T.flags & CMC_T_PER_REPLICA) ? classical_steps_per_replica_kernel : classical_steps_kernel, dim3((D.R + C.W - 1u) / C.W), dim3(C.W * 64u), lds_bytes_of(C.words), stream, D, C, A);
}
hipError_t launch_classical_energies(hipStream_t stream, const CmcDev &D, double *out) {
    hipLaunchKernelGGL(classical_energies_kernel, dim3(D.R), dim3(64), 0, stream, D, out);
    return hipGetLastError();
}
hipError_t launch_classical_init_state(hipStream_t stream, const CmcDev &D, uint32_t N) {
    hipLaunchKernelGGL(classical_init_state_kernel, dim3(D.R), dim3(64), 0, stream, D, N);
    return hipGetLastError();
}
} // namespace sse
