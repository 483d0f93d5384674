// classical_launch.h — the host-facing interface of the classical Monte Carlo kernels (sse_classical.hip.h, unit sweep_classical.hip):
// what a launch is given, the LDS carve that the kernel lays its LDS out with and the host sizes the launch by, and the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "classical_rule.h"

namespace sse {

struct CmcDev {
    CmcTables T;        // the graph tables in global memory (shared by the batch; with CMC_T_PER_REPLICA the couplings are per replica)
    uint32_t R, nwords; // replicas; state words per replica
    uint32_t *state;    // [R][nwords] bit v of word v >> 5
    uint64_t *epoch;    // [R] time steps taken
    uint64_t *counters; // [R][8] (classical_rule.h: CMC_C_*)
    uint32_t *err;      // [R] sticky error flags: a flagged replica is skipped
    uint32_t seed_lo, seed_hi, replica_offset;
};
struct CmcStepArgs {
    uint64_t t;
    const double *beta; // [R]
    uint32_t nspin, nedge, nworm, kinds, serial;
};

// The LDS of classical_steps_kernel in words.  Per wave (= per replica of the workgroup), from word 0: the state bits [nwords], then
// one stamp byte per variable [ceil(N / 4)].  Behind the waves' areas the graph tables that fit, in the order row starts, row entries,
// couplings, biases, edge list, cumulative weights (the order in which they pay: a move reads its rows more often than anything
// else); a table that does not fit, or any table with force_global, is read from global memory (offset CMC_NONE).  Tables of doubles
// start on even words.
// Per-replica couplings (CMC_T_PER_REPLICA).  The code bytes are a per-wave item like the state: code_words = cmc_code_words(E) words
// for each of the W waves (wave w's at o_jcode + w code_words), for all waves or for none, placed behind the row entries and before the
// dictionary (a move reads one code per row entry).  The doubles of the other format and the per-replica cumulative weights are read
// from global memory always (cmc_global_only): their bits are in `has` and never in `in_lds`.
enum { CMC_L_ROW = 1, CMC_L_ENT = 2, CMC_L_JV = 4, CMC_L_BIAS = 8, CMC_L_EDGES = 16, CMC_L_CUM = 32, CMC_L_JREP = 64 };
struct CmcCarve {
    uint32_t W, wave_words, o_stamp; // a wave's area: wave_words words at wave * wave_words, its stamps o_stamp words in
    uint32_t o_row, o_ent, o_jv, o_bias, o_edges, o_cum;
    uint32_t in_lds, has;            // CMC_L_* of the tables in LDS / of the tables the model has
    uint32_t words;                  // the dynamic LDS of the launch
    uint32_t o_jcode, code_words;    // the waves' code bytes (CMC_NONE: in global memory, or no codes); words of one wave's codes
};
__host__ __device__ inline uint32_t cmc_wave_words(uint32_t N) { return (N + 31u) / 32u + (N + 3u) / 4u; }
__host__ __device__ inline uint32_t cmc_edge_words(const CmcTables &T) { return (T.flags & CMC_T_EDGE16) ? T.E : 2u * T.E; }
// force: CMC_FORCE_GLOBAL every table is read from global memory, CMC_FORCE_GLOBAL_CODES the per-replica code bytes are (both for
// tests and A-B timing)
enum { CMC_FORCE_GLOBAL = 1, CMC_FORCE_GLOBAL_CODES = 2 };
inline CmcCarve cmc_carve(const CmcTables &T, uint32_t W, size_t total_words, uint32_t force) {
    const bool force_global = (force & CMC_FORCE_GLOBAL) != 0u;
    CmcCarve c{};
    c.W = W; c.wave_words = cmc_wave_words(T.N); c.o_stamp = (T.N + 31u) / 32u;
    size_t o = (size_t)W * c.wave_words;
    auto place = [&](uint32_t bit, size_t words, bool dbl, bool present, bool global_only = false) {
        if (!present) return (uint32_t)CMC_NONE;
        c.has |= bit;
        const size_t at = dbl ? (o + 1) & ~(size_t)1 : o;
        if (force_global || global_only || at + words > total_words) return (uint32_t)CMC_NONE;
        c.in_lds |= bit; o = at + words;
        return (uint32_t)at;
    };
    const bool per_replica = (T.flags & CMC_T_PER_REPLICA) != 0u, codes = per_replica && (T.flags & CMC_T_COMPACT) != 0u;
    c.code_words = codes ? cmc_code_words(T.E) : 0u;
    c.o_row = place(CMC_L_ROW, (size_t)T.N + 1, false, true);
    c.o_ent = place(CMC_L_ENT, 2 * (size_t)T.E, false, true);
    c.o_jcode = place(CMC_L_JREP, (size_t)W * c.code_words, false, per_replica, !codes || (force & CMC_FORCE_GLOBAL_CODES) != 0u);
    c.o_jv = place(CMC_L_JV, 2 * (size_t)T.njv, true, !per_replica || codes);
    c.o_bias = place(CMC_L_BIAS, 2 * (size_t)T.N, true, (T.flags & CMC_T_BIAS) != 0u);
    c.o_edges = place(CMC_L_EDGES, cmc_edge_words(T), false, true);
    c.o_cum = place(CMC_L_CUM, 2 * (size_t)T.E, true, (T.flags & CMC_T_CUM) != 0u, per_replica);
    c.words = (uint32_t)o;
    return c;
}
// the tables of a model that no launch keeps in LDS
inline uint32_t cmc_global_only(const CmcTables &T, uint32_t force) {
    if (!(T.flags & CMC_T_PER_REPLICA)) return 0u;
    const bool codes_in_lds = (T.flags & CMC_T_COMPACT) != 0u && !(force & CMC_FORCE_GLOBAL_CODES);
    return (codes_in_lds ? 0u : (uint32_t)CMC_L_JREP) | ((T.flags & CMC_T_CUM) ? (uint32_t)CMC_L_CUM : 0u);
}
// The launch of a model: the most waves per workgroup of 4, 2, 1 with every table in LDS (every table that a launch can keep there:
// cmc_global_only); when no count does that, the most waves whose own areas (state bits and stamps) fit, with the tables that still fit.
// W = 0: the areas of a single wave exceed LDS.
inline CmcCarve cmc_plan(const CmcTables &T, size_t total_words, uint32_t force) {
    const uint32_t counts[3] = {4, 2, 1};
    if (!(force & CMC_FORCE_GLOBAL))
        for (uint32_t W : counts) {
            const CmcCarve c = cmc_carve(T, W, total_words, force);
            if (c.in_lds == (c.has & ~cmc_global_only(T, force)) && c.words <= total_words) return c;
        }
    for (uint32_t W : counts)
        if ((size_t)W * cmc_wave_words(T.N) <= total_words) return cmc_carve(T, W, total_words, force);
    CmcCarve none{};
    return none;
}
// the most variables whose per-wave areas fit (what ISINGMC_ENOTIMPL names)
inline uint32_t cmc_max_vars(size_t total_words) {
    uint32_t lo = 0, hi = CMC_MAX_VARS;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (cmc_wave_words(mid) <= total_words) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// sweep_classical.hip
hipError_t launch_classical_steps(hipStream_t stream, const CmcDev &D, const CmcCarve &C, const CmcStepArgs &A);
hipError_t launch_classical_energies(hipStream_t stream, const CmcDev &D, double *out);
hipError_t launch_classical_init_state(hipStream_t stream, const CmcDev &D, uint32_t N);

// The tempering launch (classical_pt_rule.h; sse_classical_pt.hip.h, unit sweep_classical_pt.hip): R = C T slots, all in global memory
#define CMC_PT_MAX_WAVES 16u // a workgroup has min(T, 16) waves: the energy of a slot is a chain of dependent loads, which only more waves hide
struct CmcPtDev {
    uint32_t T, C;                // temperatures per chain, chains
    const double *betas;          // [T] the ladder
    uint32_t *temp_of, *slot_at;  // [R] temperature of a slot; slot (within its chain) at a temperature
    double *beta_slot;            // [R] betas[temp_of[r]]: what the next steps launch reads
    double *energy;               // [R] by slot, of the latest round
    int32_t *mag;                 // [R]
    uint64_t *attempts, *accepts; // [C][T - 1]
};
// one tempering step of every chain at step number pt_step; energy_row / mag_row: [C][T] by temperature, or null
hipError_t launch_classical_tempering(hipStream_t stream, const CmcDev &D, const CmcPtDev &P, uint64_t pt_step, double *energy_row, int32_t *mag_row);

// The overlap launch (classical_overlap_rule.h; sse_classical_overlap.hip.h, unit sweep_classical_overlap.hip): G groups of K copies,
// P = K (K - 1) / 2 pairs a group, one wave per item (g, p, t)
#define CMC_OV_MAX_ITEMS 0x80000000ull // G P T at most: four items a workgroup keep the grid inside 2^31
struct CmcOvDev {
    uint32_t K, G, P; // copies a group, groups, pairs a group
    uint64_t *hq;     // [G][P][T][N + 1] by the differing variables nq
    uint64_t *hl;     // [G][P][T][E + 1] by the differing edges nl
};
// one measurement of every item with the maps as they stand; q_row / ql_row: [G][P][T], or null.  The histograms gain one count each.
hipError_t launch_classical_overlaps(hipStream_t stream, const CmcDev &D, const CmcPtDev &P, const CmcOvDev &O, int32_t *q_row, int32_t *ql_row);

// The cluster-move launch (classical_icm_rule.h; sse_classical_icm.hip.h, unit sweep_classical_icm.hip): one wave per item (g, m, t)
// of the window, W waves a workgroup.  The LDS of classical_icm_kernel in words: per wave, from word wave * wave_words, three bit sets
// of nwords words each: d (the differing variables), the cluster, the frontier.  Nothing else lives in LDS: rows and entries are read
// from global memory, where the batch shares them.
struct CmcIcmCarve {
    uint32_t W, nwords, wave_words; // waves a workgroup; words of one bit set; a wave's area (3 nwords)
    uint32_t words;                 // the dynamic LDS of the launch
};
__host__ __device__ inline uint32_t cmc_icm_wave_words(uint32_t N) { return 3u * ((N + 31u) / 32u); }
inline CmcIcmCarve cmc_icm_carve(uint32_t N, uint32_t W) { return CmcIcmCarve{W, (N + 31u) / 32u, cmc_icm_wave_words(N), W * cmc_icm_wave_words(N)}; }
// the most waves a workgroup of 4, 2, 1 whose areas fit; W = 0: the area of a single wave exceeds LDS
inline CmcIcmCarve cmc_icm_plan(uint32_t N, size_t total_words) {
    const uint32_t counts[3] = {4, 2, 1};
    for (uint32_t W : counts)
        if ((size_t)W * cmc_icm_wave_words(N) <= total_words) return cmc_icm_carve(N, W);
    return CmcIcmCarve{};
}
// the most variables whose single-wave area fits (what ISINGMC_ENOTIMPL names)
inline uint32_t cmc_icm_max_vars(size_t total_words) {
    uint32_t lo = 0, hi = CMC_MAX_VARS;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (cmc_icm_wave_words(mid) <= total_words) lo = mid; else hi = mid - 1;
    }
    return lo;
}
struct CmcIcmDev {
    uint32_t t_first, t_last, M;        // the window of ladder indices; pairs a group, K / 2
    CmcIcmCarve C;
    uint64_t *moves, *empty, *size_sum; // [G][M][T] each
};
// the cluster moves of every item of the window at step number pt_step, with the maps as they stand
hipError_t launch_classical_icm(hipStream_t stream, const CmcDev &D, const CmcPtDev &P, const CmcOvDev &O, const CmcIcmDev &I, uint64_t pt_step);

} // namespace sse
