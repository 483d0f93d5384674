// sse_classical.hip.h — classical Ising Monte Carlo for gfx950 (GraphState, src/classical/graph.rs; the rule: classical_rule.h).
//
// One wave64 owns one replica for a whole call of t time steps; a workgroup of W waves holds W replicas and one copy of the graph
// tables (CmcCarve: in LDS where they fit, otherwise read from global memory, where all replicas share them in L2).  A wave keeps its
// replica's state as bits in LDS and one stamp byte per variable.
//
// Spin and edge steps.  Lane l of a batch holds move base + l of the step (its Philox words are drawn once).  The lanes from the
// first uncommitted one, p, evaluate their moves side by side against the committed state.  The lanes that accept stamp their sites
// with l + 1 (the smallest stamp wins).  Lane l's decision is final exactly when no stamp below l + 1 lies on a variable it read: its
// own site or sites and every neighbour in their rows; a rejected earlier lane writes no stamp and disturbs nobody.  With d the first
// lane that is not final, the lanes p .. d - 1 are committed (LDS bit flips), the stamps are cleared and the round repeats from
// p = d.  Lane p is always final (no active lane is earlier), so every round commits at least one move; the lanes before d saw the
// state that the sequential rule shows them (by induction over the lanes: the accepted moves before them touch nothing they read), so
// the result is the sequential one, move for move.
// Worm steps are the cold path: lane 0 walks (cmc_worm), with the stamp bytes as the marks of the flipped variables.
//
// Per-replica couplings (CMC_T_PER_REPLICA) are a variant of their own at compile time, classical_steps_per_replica_kernel: the
// kernel of a batch that shares its couplings carries none of it.  There a wave stages its own replica's code bytes into its LDS area
// (word copies: a row of codes is whole words) when the plan puts them there, and otherwise reads its codes, or its doubles, from
// global memory; the tables are indexed by the local replica, the Philox stream by the global one.  Everything else is shared.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "classical_launch.h"
#include "sse_core.hip.h" // philox4x32_10, lds_raw, sse_ballot

namespace sse {

// the graph tables, each in LDS or in global memory.  PR: the view of one replica of a batch with per-replica couplings
struct CmcNoReplica {};
struct CmcReplicaDev {
    uint32_t o_jcode;     // the wave's code bytes in LDS (word offset), or CMC_NONE
    const uint8_t *jcode; // the replica's rows in global memory (cmc_graph_mem)
    const double *jr, *cum_r;
    double totalw_r;
};
template <bool PR> struct CmcGraphDevT {
    const CmcTables &T;
    const CmcCarve &C;
    typename std::conditional<PR, CmcReplicaDev, CmcNoReplica>::type P;
    __device__ __forceinline__ uint32_t N() const { return T.N; }
    __device__ __forceinline__ uint32_t E() const { return T.E; }
    __device__ __forceinline__ uint32_t row(uint32_t v) const { return C.o_row != CMC_NONE ? LDSW(C.o_row, v) : T.row[v]; }
    __device__ __forceinline__ uint32_t ent(uint32_t k) const { return C.o_ent != CMC_NONE ? LDSW(C.o_ent, k) : T.ent[k]; }
    __device__ __forceinline__ double dbl(uint32_t off, const double *g, uint32_t i) const {
        return off != CMC_NONE ? *reinterpret_cast<const double *>(&lds_raw[off + 2u * i]) : g[i];
    }
    __device__ __forceinline__ uint32_t nbr(uint32_t k) const { return ent(k) & CMC_NBR_MASK; }
    __device__ __forceinline__ double J(uint32_t k) const {
        if constexpr (PR) {
            if (!(T.flags & CMC_T_COMPACT)) return P.jr[k];
            return dbl(C.o_jv, T.jv, P.o_jcode != CMC_NONE ? (uint32_t)LDSB(P.o_jcode, k) : (uint32_t)P.jcode[k]);
        } else return dbl(C.o_jv, T.jv, (T.flags & CMC_T_COMPACT) ? ent(k) >> 24 : k);
    }
    __device__ __forceinline__ double bias(uint32_t v) const { return (T.flags & CMC_T_BIAS) ? dbl(C.o_bias, T.bias, v) : 0.0; }
    __device__ __forceinline__ uint32_t edge_word(uint32_t i) const { return C.o_edges != CMC_NONE ? LDSW(C.o_edges, i) : T.edges[i]; }
    __device__ __forceinline__ void edge(uint32_t e, uint32_t &a, uint32_t &b) const {
        if (T.flags & CMC_T_EDGE16) { const uint32_t w = edge_word(e); a = w & 0xFFFFu; b = w >> 16; }
        else { a = edge_word(2u * e); b = edge_word(2u * e + 1u); }
    }
    __device__ __forceinline__ bool importance() const { return (T.flags & CMC_T_CUM) != 0u; }
    __device__ __forceinline__ double cum(uint32_t e) const {
        if constexpr (PR) return P.cum_r[e]; else return dbl(C.o_cum, T.cum, e);
    }
    __device__ __forceinline__ double totalw() const {
        if constexpr (PR) return P.totalw_r; else return T.totalw;
    }
};
using CmcGraphDev = CmcGraphDevT<false>;
// a wave's state bits and stamp bytes.  flip() is for one lane at a time (the worm): it toggles the variable's mark too
struct CmcStateDev {
    uint32_t o_state, o_stamp;
    __device__ __forceinline__ bool get(uint32_t v) const { return ((LDSW(o_state, v >> 5) >> (v & 31u)) & 1u) != 0u; }
    __device__ __forceinline__ void flip(uint32_t v) { LDSW(o_state, v >> 5) ^= 1u << (v & 31u); LDSB(o_stamp, v) ^= 1u; }
    __device__ __forceinline__ bool marked(uint32_t v) const { return LDSB(o_stamp, v) != 0u; }
    __device__ __forceinline__ void unmark(uint32_t v) { LDSB(o_stamp, v) = 0u; }
    __device__ __forceinline__ uint32_t stamp(uint32_t v) const { return LDSB(o_stamp, v); }
};
struct CmcDrawDev {
    uint32_t k0, k1, replica, epoch_lo, epoch_hi24;
    __device__ __forceinline__ uint4 words(uint32_t tag, uint32_t index) const { return philox4x32_10(index, epoch_lo, replica, (tag << 24) | epoch_hi24, k0, k1); }
    __device__ __forceinline__ uint32_t operator()(uint32_t tag, uint32_t index, int) const { return words(tag, index).x; } // word 0
};

// is a stamp of an earlier lane on v?  (stamp 0 = none: 0 - 1 wraps to the largest value)
__device__ __forceinline__ bool cmc_stamped_before(const CmcStateDev &s, uint32_t v, uint32_t lane) { return (uint32_t)(s.stamp(v) - 1u) < lane; }
template <class G> __device__ __forceinline__ bool cmc_row_stamped_before(const G &g, const CmcStateDev &s, uint32_t v, uint32_t lane) {
    bool hit = cmc_stamped_before(s, v, lane);
    for (uint32_t k = g.row(v), end = g.row(v + 1u); k < end; ++k) hit |= cmc_stamped_before(s, g.nbr(k), lane);
    return hit;
}
// lower the stamp of v to `mine` (several lanes of one store instruction may have written v: any one of them stays)
__device__ __forceinline__ bool cmc_stamp_lower(const CmcStateDev &s, uint32_t v, uint32_t mine) {
    if (LDSB(s.o_stamp, v) <= mine) return false;
    LDSB(s.o_stamp, v) = (uint8_t)mine;
    return true;
}

// nmoves spin (edge_step = false) or edge moves of one step; returns the number accepted
template <class G>
__device__ __forceinline__ uint32_t cmc_moves(const G &g, CmcStateDev &s, const CmcDrawDev &draw, double beta, uint32_t nmoves, bool edge_step,
                                              bool serial, int lane) {
    uint32_t accepted = 0;
    for (uint32_t base = 0; base < nmoves; base += 64u) {
        const uint32_t nb = nmoves - base < 64u ? nmoves - base : 64u;
        const bool mine = (uint32_t)lane < nb;
        uint32_t a = 0, b = CMC_NONE, uword = 0;
        if (mine) {
            const uint4 w = draw.words(SSE_TAG_CLASSICAL, cmc_index_move(base + (uint32_t)lane));
            uword = w.y;
            if (edge_step) g.edge(cmc_pick_edge(g, w.x), a, b); else a = cmc_range(w.x, g.N());
        }
        uint32_t p = 0;
        while (p < nb) {
            const bool active = mine && (serial ? (uint32_t)lane == p : (uint32_t)lane >= p);
            bool acc = false;
            if (active) acc = cmc_should_flip(beta, edge_step ? cmc_edge_de(g, s, a, b) : cmc_spin_de(g, s, a), uword);
            uint32_t d = p + 1u;
            if (!serial) {
                const uint32_t stamp = (uint32_t)lane + 1u;
                if (acc) { LDSB(s.o_stamp, a) = (uint8_t)stamp; if (edge_step) LDSB(s.o_stamp, b) = (uint8_t)stamp; }
                SSE_WAVE_FENCE();
                for (;;) { // the smallest stamp wins a variable that several lanes accepted on
                    bool again = false;
                    if (acc) { again = cmc_stamp_lower(s, a, stamp); if (edge_step) again |= cmc_stamp_lower(s, b, stamp); }
                    SSE_WAVE_FENCE();
                    if (!sse_any(again)) break;
                }
                bool disturbed = false;
                if (active && (uint32_t)lane > p) {
                    disturbed = cmc_row_stamped_before(g, s, a, (uint32_t)lane);
                    if (edge_step) disturbed |= cmc_row_stamped_before(g, s, b, (uint32_t)lane);
                }
                const uint64_t nonfinal = sse_ballot(disturbed);
                d = nonfinal ? (uint32_t)__builtin_ctzll(nonfinal) : nb;
                SSE_WAVE_FENCE();
                if (acc) { LDSB(s.o_stamp, a) = 0u; if (edge_step) LDSB(s.o_stamp, b) = 0u; }
            }
            const bool commit = acc && (uint32_t)lane < d;
            if (commit) { // the committed lanes flip different variables (a later one on the same variable would be disturbed)
                atomicXor(&LDSW(s.o_state, a >> 5), 1u << (a & 31u));
                if (edge_step) atomicXor(&LDSW(s.o_state, b >> 5), 1u << (b & 31u));
            }
            accepted += (uint32_t)popc64(sse_ballot(commit));
            SSE_WAVE_FENCE();
            p = d;
        }
    }
    return accepted;
}

template <bool PR> __device__ __forceinline__ void cmc_steps(const CmcDev &D, const CmcCarve &C, const CmcStepArgs &A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * C.W + (uint32_t)wave;
    // the graph tables that live in LDS, staged by the whole workgroup (waves without a replica help and leave behind the barrier)
    const CmcTables &T = D.T;
    const uint32_t nthreads = C.W * 64u;
    if (C.o_row != CMC_NONE) for (uint32_t i = threadIdx.x; i < T.N + 1u; i += nthreads) LDSW(C.o_row, i) = T.row[i];
    if (C.o_ent != CMC_NONE) for (uint32_t i = threadIdx.x; i < 2u * T.E; i += nthreads) LDSW(C.o_ent, i) = T.ent[i];
    if (C.o_edges != CMC_NONE) for (uint32_t i = threadIdx.x, n = cmc_edge_words(T); i < n; i += nthreads) LDSW(C.o_edges, i) = T.edges[i];
    const uint32_t *jv = reinterpret_cast<const uint32_t *>(T.jv), *bias = reinterpret_cast<const uint32_t *>(T.bias), *cum = reinterpret_cast<const uint32_t *>(T.cum);
    if (C.o_jv != CMC_NONE) for (uint32_t i = threadIdx.x; i < 2u * T.njv; i += nthreads) LDSW(C.o_jv, i) = jv[i];
    if (C.o_bias != CMC_NONE) for (uint32_t i = threadIdx.x; i < 2u * T.N; i += nthreads) LDSW(C.o_bias, i) = bias[i];
    if (C.o_cum != CMC_NONE) for (uint32_t i = threadIdx.x; i < 2u * T.E; i += nthreads) LDSW(C.o_cum, i) = cum[i];
    CmcStateDev s;
    s.o_state = (uint32_t)wave * C.wave_words; s.o_stamp = s.o_state + C.o_stamp;
    const bool live = r < D.R && D.err[r < D.R ? r : 0u] == 0u;
    if (live) {
        for (uint32_t i = lane; i < D.nwords; i += 64u) LDSW(s.o_state, i) = D.state[(size_t)r * D.nwords + i];
        for (uint32_t i = lane; i < C.wave_words - C.o_stamp; i += 64u) LDSW(s.o_stamp, i) = 0u;
    }
    CmcGraphDevT<PR> g{T, C, {}};
    if constexpr (PR) { // the tables of the local replica r; its code bytes into the wave's own words (a row is code_words whole words)
        if (live) {
            const CmcGraphMem m = cmc_graph_mem(T, r);
            g.P = CmcReplicaDev{C.o_jcode != CMC_NONE ? C.o_jcode + (uint32_t)wave * C.code_words : (uint32_t)CMC_NONE, m.jcode, m.jr, m.cum_r, m.totalw_r};
            if (g.P.o_jcode != CMC_NONE) {
                const uint32_t *codes = reinterpret_cast<const uint32_t *>(m.jcode);
                for (uint32_t i = lane; i < C.code_words; i += 64u) LDSW(g.P.o_jcode, i) = codes[i];
            }
        }
    }
    __syncthreads();
    if (!live) return;
    const double beta = A.beta[r];
    const uint32_t nspin = cmc_default_moves(A.nspin, T.N / 2u), nedge = cmc_default_moves(A.nedge, T.E / 2u), nworm = cmc_default_moves(A.nworm, 1u);
    uint64_t epoch = D.epoch[r];
    uint64_t ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    CmcDrawDev draw;
    draw.k0 = D.seed_lo; draw.k1 = D.seed_hi; draw.replica = D.replica_offset + r;
    for (uint64_t step = 0; step < A.t; ++step, ++epoch) {
        draw.epoch_lo = (uint32_t)epoch; draw.epoch_hi24 = (uint32_t)(epoch >> 32) & 0xFFFFFFu;
        const uint32_t kind = cmc_step_kind(A.kinds, draw);
        if (kind == 0u) {
            ctr[CMC_C_SPIN] += nspin;
            ctr[CMC_C_SPIN_ACC] += cmc_moves(g, s, draw, beta, nspin, false, A.serial != 0u, lane);
        } else if (kind == 1u) {
            ctr[CMC_C_EDGE] += nedge;
            ctr[CMC_C_EDGE_ACC] += cmc_moves(g, s, draw, beta, nedge, true, A.serial != 0u, lane);
        } else {
            if (lane == 0) {
                uint32_t ndraw = 0;
                for (uint32_t i = 0; i < nworm; ++i) cmc_worm(g, s, beta, A.kinds != CMC_KINDS_WORM_NO_DOUBLES, draw, &ndraw, ctr);
            }
            SSE_WAVE_FENCE();
        }
    }
    SSE_WAVE_FENCE();
    for (uint32_t i = lane; i < D.nwords; i += 64u) D.state[(size_t)r * D.nwords + i] = LDSW(s.o_state, i);
    if (lane == 0) {
        D.epoch[r] = epoch;
        for (int i = 0; i < 8; ++i) D.counters[(size_t)r * 8u + i] += ctr[i];
    }
}

__global__ __launch_bounds__(256) void classical_steps_kernel(CmcDev D, CmcCarve C, CmcStepArgs A) { cmc_steps<false>(D, C, A); }
__global__ __launch_bounds__(256) void classical_steps_per_replica_kernel(CmcDev D, CmcCarve C, CmcStepArgs A) { cmc_steps<true>(D, C, A); }

// get_energy (graph.rs:430-447), one wave per replica: the lanes share the variables and their sums are added across the wave
__global__ __launch_bounds__(64) void classical_energies_kernel(CmcDev D, double *out) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const CmcGraphMem g = cmc_graph_mem(D.T, r);
    struct Bits {
        const uint32_t *w;
        __device__ bool get(uint32_t v) const { return ((w[v >> 5] >> (v & 31u)) & 1u) != 0u; }
    } s{D.state + (size_t)r * D.nwords};
    double e = 0.0;
    for (uint32_t v = lane; v < D.T.N; v += 64u) e = e + cmc_energy_of(g, s, v) + (s.get(v) ? -g.bias(v) : g.bias(v));
    for (int o = 32; o > 0; o >>= 1) e += __shfl_down(e, o, 64);
    if (lane == 0) out[r] = e;
}

// make_random_spin_state (graph.rs:451-453) exactly as isingmc_create draws it: one fair bit per variable, tag INIT, epoch 0
__global__ void classical_init_state_kernel(CmcDev D, uint32_t N) {
    const uint32_t r = blockIdx.x;
    CmcDrawDev draw;
    draw.k0 = D.seed_lo; draw.k1 = D.seed_hi; draw.replica = D.replica_offset + r; draw.epoch_lo = 0u; draw.epoch_hi24 = 0u;
    for (uint32_t i = threadIdx.x; i < D.nwords; i += blockDim.x) {
        uint32_t w = 0;
        for (uint32_t j = 0; j < 32u && i * 32u + j < N; ++j) w |= (draw.words(SSE_TAG_INIT, i * 32u + j).x >> 31) << j;
        D.state[(size_t)r * D.nwords + i] = w;
    }
}

} // namespace sse
