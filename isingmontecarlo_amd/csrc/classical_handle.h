// classical_handle.h — the handle of classical Monte Carlo and its device memory, for the two host files that call the HIP runtime
// (classical.hip: creation, time steps, accessors; classical_pt.hip: the three attachments and the device rounds).  What needs no
// device (tables, checks, plans, the sequential rule) is classical_host.h.  Internal: the C ABI is include/isingmc_hip.h.
#pragma once
#include "classical_host.h"
#include "hip_host.h"

#include <utility>

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
