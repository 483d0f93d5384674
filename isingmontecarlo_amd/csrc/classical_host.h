// classical_host.h — the device-free half of classical Monte Carlo's host code (classical_host.hip): the host form of the graph tables,
// the config check, the launch plans, the argument checks of the ladder, the groups and the window, and what a run of rounds is
// given.  classical_handle.h adds the handle on top for classical.hip and classical_pt.hip.  Nothing here calls the HIP runtime or a
// launcher: the unit links into a program without either (tests/test_classical_host_sanitized_cpu.py).  Internal: the C ABI is
// include/isingmc_hip.h.
#pragma once
#include "../../include/isingmc_hip.h"
#include "classical_launch.h" // the carve types and the inline plans

#include <algorithm>
#include <string>
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
    // the first chain of T slots (of R) whose coupling rows are not all bitwise equal, or CMC_NONE
    uint32_t first_mixed_chain(uint32_t R, uint32_t T) const;
};

int cmc_refuse(int rc, const std::string &why); // sets the error text of a call without a handle (this thread's) ...
const char *cmc_last_refusal();                 // ... and reads it: what isingmc_classical_last_error(NULL) returns
int cmc_check_config(const isingmc_classical_config *cfg);
void cmc_build_tables(const isingmc_classical_config *cfg, CmcHostTables &H);
// checks, tables and the launch plan: everything isingmc_classical_create decides before it touches a device
int cmc_plan_config(const isingmc_classical_config *cfg, uint32_t lds_bytes, CmcHostTables &H, sse::CmcCarve &C);
// the eight slots of isingmc_classical_plan / isingmc_classical_launch_plan, the four of isingmc_classical_icm_plan / _icm_launch_plan
void cmc_plan_slots(const sse::CmcCarve &C, uint32_t table_flags, uint32_t out[8]);
void cmc_icm_plan_slots(const sse::CmcIcmCarve &C, uint32_t lds_bytes, uint32_t out[4]);

// One run of rounds, as the isingmc_classical_pt_run* entries (on the device: classical_pt.hip) and their isingmc_classical_host_pt_run*
// twins (on the CPU) describe it: where the series go (null: not recorded) and which phases a round has behind its steps.  What every
// entry is given comes first, in the entries' own order, so that an entry initialises the struct from its arguments.
struct CmcRounds {
    uint64_t rounds, steps;
    uint32_t nspin, nedge, nworm, kinds;
    double *energy_out;                          // a row a round: [C][T]
    int32_t *mag_out;                            // [C][T]
    int32_t *q_out = nullptr, *ql_out = nullptr; // [G][P][T], with the measurement only
    bool overlaps = false, cluster_moves = false; // the overlaps are measured (needs groups); the cluster moves run behind the measurement (needs a window)
};

// What the attach calls and the CPU rounds ask of a ladder (classical_pt_rule.h), of the batch as groups of copies
// (classical_overlap_rule.h; and the sizes that follow) and of a window of cluster moves (classical_icm_rule.h; t_last = 0 means T).
// Every error is reachable without a device; `why` is its text.
struct CmcOvShape {
    uint32_t K, G, P;
    uint64_t items;            // G P T
    size_t hq_count, hl_count; // entries of the histograms
};
int cmc_check_pt_args(uint32_t R, uint32_t replica_offset, uint32_t ntemps, const double *betas, std::string &why);
int cmc_check_pt_couplings(const CmcHostTables &H, uint32_t R, uint32_t ntemps, std::string &why);
int cmc_check_overlap_args(const CmcHostTables &H, uint32_t R, uint32_t replica_offset, uint32_t T, uint32_t K, CmcOvShape &S, std::string &why);
int cmc_check_icm_window(uint32_t T, uint32_t &t_first, uint32_t &t_last, std::string &why);
std::string cmc_icm_too_large(uint32_t lds_bytes); // the refusal of a model whose bit sets exceed LDS
