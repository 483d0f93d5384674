// Instantiations of sse::cluster_kernel (sse_cluster.hip.h): the cluster-update launch of the headline geometry.
#include "../../include/isingmc_hip.h"
#include "sse_cluster.hip.h"
#include "sse_launch.h"
namespace sse {
template <int K, bool HL, int PHASE>
static hipError_t launch_cluster_one(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    return launch_lds(cluster_kernel<K, HL, PHASE>, dim3(B.R), dim3(SSE_CLW * 64), c.lds_bytes, c.stream, B, A);
}
// (PHASE = 1, the data-preparation symbol, exists for K = 4 only)
template <int K, bool HL>
static hipError_t launch_cluster_phase(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    if constexpr (K == 4) if (c.phase) return launch_cluster_one<K, HL, 1>(c, B, A);
    return launch_cluster_one<K, HL, 0>(c, B, A);
}
size_t cluster_lds_words(uint32_t N, uint32_t nwords, uint32_t Nb, uint32_t ufcap, bool has_long) { ClLds L; L.carve(N, nwords, Nb, ufcap, has_long); return L.end; }
bool cluster_ids_fit(uint32_t N, uint32_t S, uint32_t ufcap) { return cl_ids_fit(N, S, ufcap); }
uint32_t cluster_max_vars() { return SSE_CL_MAX_VARS; }
hipError_t launch_cluster(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    if (c.mode != SSE_MODE_LDS_EDGES || B.N > SSE_CL_MAX_VARS || !(A.domask & SSE_DO_CLUSTER)) return hipErrorInvalidValue;
    const bool hl = B.has_long != 0u;
    if (c.K == 4) return hl ? launch_cluster_phase<4, true>(c, B, A) : launch_cluster_phase<4, false>(c, B, A);
    if (c.K == 2) return hl ? launch_cluster_phase<2, true>(c, B, A) : launch_cluster_phase<2, false>(c, B, A);
    return hipErrorInvalidValue;
}
} // namespace sse

// Host-only audit of the kernel's LDS layout (include/isingmc_hip.h): ClLds::carve, the words of the launch, the gate, the root list.
extern "C" int isingmc_plan_cluster_lds(uint32_t N, uint32_t nwords, uint32_t Nb, uint32_t has_long, uint32_t ufcap, uint32_t S, uint32_t out[13]) {
    if (!out || N == 0 || N > SSE_CL_MAX_VARS || nwords < (N + 31) / 32) return ISINGMC_EINVAL;
    sse::ClLds L;
    L.carve(N, nwords, Nb, ufcap, has_long != 0u);
    out[0] = L.o_tab; out[1] = L.o_state; out[2] = L.o_touch; out[3] = L.o_misc; out[4] = L.o_chn; out[5] = L.o_chtr;
    out[6] = L.o_ent; out[7] = L.o_frozen; out[8] = L.o_froot; out[9] = L.o_parent;
    out[10] = L.end;
    out[11] = sse::cl_ids_fit(N, S, ufcap) ? 1u : 0u;
    out[12] = sse::cl_list_cap(N, S);
    return ISINGMC_OK;
}
// ... and, of the same carve, the queues of parked unions: word offset, words, entries per wave
extern "C" int isingmc_plan_cluster_queue(uint32_t N, uint32_t nwords, uint32_t Nb, uint32_t has_long, uint32_t ufcap, uint32_t out[3]) {
    if (!out || N == 0 || N > SSE_CL_MAX_VARS || nwords < (N + 31) / 32) return ISINGMC_EINVAL;
    sse::ClLds L;
    L.carve(N, nwords, Nb, ufcap, has_long != 0u);
    out[0] = L.o_queue; out[1] = SSE_CL_QUEUE_WORDS; out[2] = SSE_CL_QCAP;
    return ISINGMC_OK;
}
