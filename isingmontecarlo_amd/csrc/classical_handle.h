// classical_handle.h — what the two host files of classical Monte Carlo share (classical.hip: creation, time steps, accessors;
// classical_pt.hip: tempering): the handle, the host form of the graph tables, the config check and the step loop of the sequential
// rule.  Internal: the C ABI is include/isingmc_hip.h.
#pragma once
#include "../../include/isingmc_hip.h"
#include "classical_launch.h"
#include "hip_host.h"

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

// the graph tables of classical_rule.h on the host
struct CmcHostTables {
    std::vector<uint32_t> row, ent, edges;
    std::vector<double> jv, bias, cum;
    std::vector<uint8_t> jcode;       // per-replica couplings: [R] rows of 4 cmc_code_words(E) bytes (codes) ...
    std::vector<double> jr, totalw_r; // ... or [R][2E] doubles; [R] totals of the per-replica running sums
    uint32_t N = 0, E = 0, flags = 0;
    double totalw = 0.0;
    CmcTables view() const {
        return CmcTables{N, E, flags, (uint32_t)jv.size(), row.data(), ent.data(), jv.data(), bias.empty() ? nullptr : bias.data(), edges.data(),
                         cum.empty() ? nullptr : cum.data(), totalw, jcode.empty() ? nullptr : jcode.data(), jr.empty() ? nullptr : jr.data(),
                         totalw_r.empty() ? nullptr : totalw_r.data()};
    }
    // 0: the batch shares its couplings, 1: per-replica codes into a batch-wide dictionary, 2: per-replica doubles
    uint32_t coupling_format() const { return !(flags & CMC_T_PER_REPLICA) ? 0u : (flags & CMC_T_COMPACT) ? 1u : 2u; }
    // the first chain of T slots (of R) whose coupling rows are not all bitwise equal, or CMC_NONE
    uint32_t first_mixed_chain(uint32_t R, uint32_t T) const;
};

// tempering (isingmc_classical_pt_attach): every array is allocated once at its largest size, R entries
struct CmcPtHandle {
    bool attached = false;
    sse::CmcPtDev dev{};
    double *d_betas = nullptr;
    uint64_t step = 0;
    std::vector<double> betas;
};

// overlaps between copies (isingmc_classical_overlap_attach): the histograms live from attach to detach
struct CmcOvHandle {
    bool attached = false;
    sse::CmcOvDev dev{};
    DevBuf hq, hl;                     // the blocks behind dev.hq / dev.hl
    size_t hq_count = 0, hl_count = 0; // entries of the two histograms
};

// cluster moves between copies (isingmc_classical_icm_attach): the counts live from attach to detach
struct CmcIcmHandle {
    bool attached = false;
    sse::CmcIcmDev dev{};
    DevBuf counts;    // the block behind dev.moves / dev.empty / dev.size_sum: [3][G][M][T]
    size_t count = 0; // entries of one of the three, G M T
};

struct isingmc_classical {
    sse::CmcDev dev{};
    sse::CmcCarve carve{};
    CmcHostTables host;
    uint32_t flags = 0;
    int device = 0;
    uint32_t lds_bytes = 0; // the LDS of one workgroup of the device
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    double *d_beta = nullptr, *d_energy = nullptr;
    CmcPtHandle pt;
    CmcOvHandle ov;
    CmcIcmHandle icm;
    std::vector<DevBuf> allocs;
    mutable std::string err;
};

// count zeroed elements of device memory that live as long as the handle
template <typename T>
static int cmc_alloc(isingmc_classical *g, T **p, size_t count) {
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    DevBuf q;
    if (const hipError_t e = q.alloc(bytes)) { g->err = std::string("hipMalloc(&q, bytes): ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    HIP_TRY(g, hipMemset(q.as<void>(), 0, bytes));
    *p = q.as<T>();
    g->allocs.push_back(std::move(q));
    return ISINGMC_OK;
}
// ... a copy of v (at least one element is allocated)
template <typename T>
static int cmc_upload(isingmc_classical *g, const T **p, const std::vector<T> &v) {
    DevBuf q;
    if (const hipError_t e = q.alloc(std::max<size_t>(v.size(), 1) * sizeof(T))) { g->err = std::string("hipMalloc(&q, bytes): ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    if (!v.empty()) HIP_TRY(g, hipMemcpy(q.as<void>(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *p = q.as<T>();
    g->allocs.push_back(std::move(q));
    return ISINGMC_OK;
}

// a replica's state as bytes on the host, with the marks of the worm next to them
struct CmcHostState {
    uint8_t *s, *mark;
    bool get(uint32_t v) const { return s[v] != 0; }
    void flip(uint32_t v) { s[v] ^= 1u; mark[v] ^= 1u; }
    bool marked(uint32_t v) const { return mark[v] != 0; }
    void unmark(uint32_t v) { mark[v] = 0; }
};
// the move counts of a step as the launches resolve them
struct CmcHostMoves { uint32_t nspin, nedge, nworm, kinds; };

// classical.hip
int cmc_refuse(int rc, const std::string &why); // the error text of a call without a handle
int cmc_check_config(const isingmc_classical_config *cfg);
void cmc_build_tables(const isingmc_classical_config *cfg, CmcHostTables &H);
// t time steps of replica `replica` (its global index; g is the view of its local index) by the sequential rule: state [N] bytes,
// mark [N] zeroed scratch, *epoch advanced, ctr [8] added to
void cmc_host_replica_steps(const CmcGraphMem &g, uint64_t seed, uint32_t replica, uint64_t t, double beta, const CmcHostMoves &m, uint8_t *state,
                            uint8_t *mark, uint64_t *epoch, uint64_t *ctr);
