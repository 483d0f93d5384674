// batch.hip.h — the batch behind the C ABI (include/isingmc_hip.h) as the host-side translation units share it: create.hip (creation),
// driver.hip (the sweep driver), isingmc_hip.hip (the accessors), pt.hip (parallel tempering) and record.hip (the sample record).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>
#include "../../include/isingmc_hip.h"
#include "hip_host.h"
#include "lds_plan.h"
#include "sse_batch.h"

// The launch geometry and modes a batch runs with: the part of plan_batch()'s choice that is read after isingmc_create.  Later calls
// only re-size lds_words (size_lds) and may give up rvb_split (prepare()).
struct BatchGeometry {
    uint32_t W = 8, K = 4, mode = sse::SSE_MODE_GENERAL; // mode: SSE_MODE_* (bond decode / where the per-variable tables live)
    uint32_t W_off = 0;                 // waves per replica of the off-diagonal launches; 0 = decide per launch (16 when its tables fit in LDS)
    bool w8_ok = false;                 // an 8-wave off-diagonal geometry without LDS union-find fits (and the row stride allows it)
    size_t lds_words_pm_diag = 0;       // +-J decode: LDS of the diagonal launch with its per-wave spin bytes in LDS (0 = they do not fit: mode 4 there too)
    size_t lds_words_diag = 0, lds_words_fast = 0; // LDS words of the diagonal launch: general kernel, trimmed kernel
    bool fast_diag = false;             // the diagonal-pass launch uses sse_fast.hip.h (headline geometry: LDS edge tables, 4 waves, N <= 4096)
    bool lean_cluster = false;          // cluster (+ free spins + sampling) launches use sse_cluster.hip.h when their ids fit its LDS union-find
    bool defer = false;                 // ... leaving its flips as one byte per slot for the next (trimmed) diagonal launch to apply
    size_t lds_words_rvb = 0;           // LDS words of a general launch that runs an RVB sweep
    bool rvb_global = false;            // ISINGMC_CFG_RVB_GLOBAL_TABLES: every RVB sweep is a launch of its own with the tables in HBM (SSE_PASSES_RVB_G)
    bool rvb_split = false;             // RVB sweeps run as a growth launch + a main launch (sse_rvb_split.hip.h) instead of the fused kernel
    uint32_t rvb_main_W = 4;            // waves per replica of that main launch
    size_t lds_words = 0;               // LDS words of the general launch (its union-find ids: DevBatch::lds_ufcap)
    bool fused_launch = false;          // ISINGMC_CFG_FUSED_LAUNCH: whole timesteps in one kernel (no diagonal-only launches)
    size_t lds_total_words = 0;         // all of a workgroup's LDS
    uint32_t uf_ids_limit = 0;          // the caller's test limit on the ids of the LDS union-find
};

struct isingmc_batch : BatchGeometry {
    sse::DevBatch dev{};
    uint32_t last_W_off = 0;
    uint64_t steps_per_launch = 0;
    uint32_t acc_rows = 0;
    uint32_t rvb_updates = 0;
    uint32_t *d_acc_row = nullptr;
    DevBuf acc;                         // the accumulator table behind dev.acc: [acc_rows][8], replaced by isingmc_set_accumulator_rows
    bool acc_follow_slots = false;      // the caller passed the tempering slots as accumulator rows: isingmc_pt_step keeps row = slot
    uint32_t max_ntrans = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;
    uint32_t last_launches = 0;
    bool last_lean = false;             // the last cluster launch used the dedicated kernel
    bool pending = false;               // some replicas' strings in HBM may still wait for their flip bytes (DevBatch::pend says which)
    const double *beta_dev = nullptr;   // isingmc_pt_timesteps: per-replica betas already on the device (used when the caller passes none)
    bool last_rvb_split = false;        // the last RVB sweep ran as a growth launch + a main launch
    bool last_rvb_global = false;       // ... as a launch with its tables in HBM
    std::vector<hipEvent_t> evpool;     // per-launch events of the split path (bounded, see run())
    float pass_ms[3] = {0.f, 0.f, 0.f}; // [0] diagonal-only launches, [1] all other launches of the last run, [2] of those: the RVB-sweep launches
    uint32_t pass_launches[3] = {0, 0, 0};
    double offset = 0.0;
    std::vector<double> offsets;        // per-replica energy offsets (ISINGMC_CFG_PER_REPLICA_J), else empty
    bool per_replica_J = false;
    bool generic = false;               // built from isingmc_interaction matrices
    bool generic_sym = false;           // ... all of them symmetric under a global spin flip (cluster updates allowed)
    std::vector<double> mats_host;      // [Nb][16] in | out<<2
    std::vector<sse::BondRec> bonds_host;
    double *d_beta = nullptr;
    uint32_t *d_out = nullptr;
    uint32_t *d_vstate = nullptr;
    uint8_t *d_ok = nullptr;
    std::vector<DevBuf> allocs;         // what lives as long as the batch (dalloc)
    DevBuf rvb_prod, rvb_tbl;           // the blocks behind dev.rvb_prod / dev.rvb_tbl (driver.hip allocates them on first use)
    mutable std::string err;
    struct PtState *pt = nullptr;       // native parallel tempering (isingmc_pt_*, pt.hip)
    std::vector<uint32_t> ham_row_host; // [R] bond-table row of each local replica (tempering between different Hamiltonians), empty = identity
    // sample record (isingmc_record_*, record.hip): [rec_cap][R][nwords] words, rows 0 .. rec_count - 1 written; empty = none attached
    DevBuf rec;
    uint32_t rec_cap = 0, rec_count = 0;
    // scratch of the record's observables, grown on demand: observable groups, bit series [R][ngroups][Tw], autocorrelations [R][T]
    DevBuf obs_groups, obs_series, obs_out;
    // scratch of the imaginary-time folds (isingmc_itime_groups, isingmc_bond_counts), grown on demand: results, groups, variable -> groups lists
    DevBuf itime_buf;
};

namespace sse {

// the LDS questions of lds_plan.h asked of a batch
inline bool is_tg(const isingmc_batch *b) { return is_tg(b->mode); }
inline bool is_pm(const isingmc_batch *b) { return is_pm(b->mode); }
inline uint32_t lds_edges(const isingmc_batch *b) { return lds_edges(b->mode, b->dev); }
inline LdsNeeds lds_needs(const isingmc_batch *b) { return {b->dev, b->mode, b->lds_total_words, b->uf_ids_limit, b->max_ntrans}; }
inline LdsPlan plan_lds(const isingmc_batch *b, uint32_t W) { return plan_lds(lds_needs(b), W); }

// count elements of device memory that live as long as the batch, or in `owner` (whose previous block is freed)
template <typename T>
int dalloc(isingmc_batch *b, T **p, size_t count, bool zero = true, DevBuf *owner = nullptr) {
    const size_t bytes = (count ? count : 1) * sizeof(T);
    DevBuf q;
    if (const hipError_t e = q.alloc(bytes)) { b->err = std::string("hipMalloc(&q, bytes): ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    if (zero) HIP_TRY(b, hipMemset(q.as<void>(), 0, bytes));
    *p = q.as<T>();
    if (owner) *owner = std::move(q); else b->allocs.push_back(std::move(q));
    return ISINGMC_OK;
}

// The observable groups of a call (group g = group_vars[group_start[g] .. group_start[g + 1])): non-empty groups of variables below N
inline int check_groups(isingmc_batch *b, const char *prefix, uint32_t ngroups, const uint32_t *group_start, const uint32_t *group_vars, uint32_t N) {
    const char *why = nullptr;
    if (group_start[0] != 0u) why = ": group_start[0] must be 0";
    for (uint32_t g = 0; !why && g < ngroups; ++g)
        if (group_start[g + 1] <= group_start[g]) why = ": every observable group needs at least one variable";
    for (uint32_t k = 0; !why && k < group_start[ngroups]; ++k)
        if (group_vars[k] >= N) why = ": group variable out of range";
    if (!why) return ISINGMC_OK;
    b->err = std::string(prefix) + why;
    return ISINGMC_EINVAL;
}

int ensure_materialized(isingmc_batch *b);   // driver.hip: apply the flip bytes that replicas' strings still wait for
hipError_t record_append(isingmc_batch *b);  // record.hip: the p = 0 states of a sampled step go to the sample record
void pt_free(isingmc_batch *b);              // pt.hip: release the tempering state, if any
int pt_rows_are_slots(isingmc_batch *b, uint32_t nrows, const uint32_t *rows, bool *yes); // pt.hip: are these accumulator rows the replicas' tempering slots?

} // namespace sse
