// Launches of the sample-record kernels (sse_observe.hip.h): bit series of two-valued observables and their autocorrelations.
#include "sse_observe.hip.h"
namespace sse {
hipError_t launch_record_series(hipStream_t stream, const uint32_t *rec, uint32_t R, uint32_t nwords, uint32_t T, const ObsGroups &G, uint32_t *out) {
    const size_t lds = 4 * obs_series_lds_words(nwords);
    return launch_lds(record_series_kernel, dim3((T + OBS_TILE - 1) / OBS_TILE, R), dim3(OBS_SERIES_WAVES * 64), lds, stream, rec, R, nwords, T, G, out);
}
hipError_t launch_bit_autocorr(hipStream_t stream, const uint32_t *series, uint32_t R, uint32_t ngroups, uint32_t T, double *out) {
    const size_t lds = 4 * (obs_autocorr_lds_words(T) + 2);
    // OBS_LAGS lags per lane: whole waves for a quarter of the lags while the series is short, one pass per 4096 lags when it is long
    uint32_t threads = ((T + OBS_LAGS - 1u) / OBS_LAGS + 63u) / 64u * 64u;
    if (threads > OBS_MAX_THREADS) threads = OBS_MAX_THREADS;
    return launch_lds(bit_autocorr_kernel, dim3(R), dim3(threads), lds, stream, series, ngroups, T, out);
}
} // namespace sse
