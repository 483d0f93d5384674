// Launcher of the classical cluster-move kernel (sse_classical_icm.hip.h).
#include "sse_classical_icm.hip.h"
#include "sse_launch.h" // launch_lds
#include "lds_plan.h"   // lds_bytes_of
namespace sse {
hipError_t launch_classical_icm(hipStream_t stream, const CmcDev &D, const CmcPtDev &P, const CmcOvDev &O, const CmcIcmDev &I, uint64_t pt_step) {
    const CmcIcmCarve &C = I.C;
    if (O.K < 2u || I.M != cmc_icm_pairs(O.K) || I.t_first >= I.t_last || I.t_last > P.T || (uint64_t)O.G * O.K != P.C || (uint64_t)P.C * P.T != D.R) return hipErrorInvalidValue;
    if (C.W == 0u || C.W > CMC_ICM_MAX_WAVES || C.nwords != D.nwords || C.wave_words != cmc_icm_wave_words(D.T.N) || C.words != C.W * C.wave_words) return hipErrorInvalidValue;
    if (!I.moves || !I.empty || !I.size_sum) return hipErrorInvalidValue;
    const uint64_t items = (uint64_t)O.G * I.M * (I.t_last - I.t_first), grid = (items + C.W - 1u) / C.W;
    if (items == 0u || grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return launch_lds(classical_icm_kernel, dim3((uint32_t)grid), dim3(64u * C.W), lds_bytes_of(C.words), stream, D, P, O, I, pt_step);
}
} // namespace sse
