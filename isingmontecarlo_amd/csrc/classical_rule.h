// classical_rule.h — the moves of classical Ising Monte Carlo (GraphState, src/classical/graph.rs), once: the packed graph tables, the
// random stream of a time step, the energy differences, the acceptance test, the edge choice and the whole worm move.
//
// Three consumers: classical_steps_kernel (sse_classical.hip.h: one wave per replica, graph tables in LDS or in global memory),
// isingmc_classical_host_steps (classical_host.hip: the sequential rule on the CPU) and the table builder of isingmc_classical_create.  The
// functions are templates over a graph accessor G and a state accessor S, so the same arithmetic reads plain arrays on the host and LDS
// on the device:
//   G: N(), E(), row(v) (start of v's row; row(N) = entries), nbr(k), J(k) (neighbour and coupling of row entry k), bias(v),
//      edge(e, a, b), importance(), cum(e), totalw()
//   S: get(v), flip(v) (a flip also toggles v's mark), marked(v), unmark(v)
// A step of replica r at epoch e draws from the Philox stream (index, e_lo, r, tag << 24 | e_hi24) keyed by the seed (sse_format.h):
// a draw is any  uint32_t draw(uint32_t tag, uint32_t index, int word).
// Plain inline functions, no device code: hipcc compiles them for the kernel, a host C++ compiler takes the header as it is.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/sse_format.h" // SSE_HD, SSE_TAG_CLASSICAL, SSE_TAG_CLASSICAL_WORM

// ---- the graph tables ----
// binding_mat (graph.rs:69-78) as a CSR: variable v's row is entries row[v] .. row[v + 1], (neighbour, J) sorted by neighbour with a
// stable sort in edge order; multi-edges stay separate entries.  An entry is  neighbour | code << 24 : with CMC_T_COMPACT the model has
// at most 256 distinct couplings and jv[code] is the entry's J; otherwise code = 0 and jv[k] is the J of entry k.  (This is the batch
// that shares its couplings; CMC_T_PER_REPLICA below.)
#define CMC_MAX_VARS (1u << 24)
#define CMC_NBR_MASK 0xFFFFFFu
#define CMC_T_COMPACT 1u // jv is a dictionary of the distinct couplings
#define CMC_T_EDGE16 2u  // N <= 65536: an edge is one word a | b << 16 (otherwise two words a, b)
#define CMC_T_BIAS 4u    // some bias is non-zero (otherwise bias is null: all zero)
#define CMC_T_CUM 8u     // edge importance sampling: cum[e] = J_0 + .. + J_e, totalw = cum[E - 1] (graph.rs:320-336)
// Per-replica couplings (disorder realisations on one topology): the code bits of every entry are 0 and the couplings are a table of
// their own, indexed by (local replica r, row entry k); both entries of edge e carry J[r][e].  With CMC_T_COMPACT the batch has at most
// 256 distinct couplings over all R E values: jv is their dictionary (order of first appearance, r-major) and jcode holds one byte per
// entry, in rows of cmc_code_words(E) words (the bytes behind 2E are 0).  Otherwise jr holds one double per entry and jv is empty.
// With CMC_T_CUM the running sums are per replica as well: cum [R][E], totalw_r [R].
#define CMC_T_PER_REPLICA 16u
#define CMC_NONE 0xFFFFFFFFu
struct CmcTables {
    uint32_t N, E, flags, njv; // njv: entries of jv
    const uint32_t *row;       // [N + 1]
    const uint32_t *ent;       // [2E]
    const double *jv;          // [njv]
    const double *bias;        // [N] or null
    const uint32_t *edges;     // [E] or [2E]
    const double *cum;         // [E] ([R][E] per replica) or null
    double totalw;
    const uint8_t *jcode;      // [R][4 cmc_code_words(E)] or null
    const double *jr;          // [R][2E] or null
    const double *totalw_r;    // [R] or null
};
SSE_HD inline uint32_t cmc_code_words(uint32_t E) { return (2u * E + 3u) / 4u; } // the words of one replica's code bytes
// what a time step draws its kind from (isingmc_classical_timesteps `kinds`)
#define CMC_KINDS_ALL 0u   // spin, edge or worm steps, as do_time_step draws them (:364-365)
#define CMC_KINDS_BASIC 1u // only_basic_moves: spin or edge steps
#define CMC_KINDS_SPIN 2u  // every step a spin step, an edge step, a worm step (with doubles, as do_time_step runs them) ...
#define CMC_KINDS_EDGE 3u
#define CMC_KINDS_WORM 4u
#define CMC_KINDS_WORM_NO_DOUBLES 5u // ... or a worm step with allow_doubles = false
#define CMC_KINDS_COUNT 6u
// counters [8]: attempted and accepted moves per kind, worm failures, worm path entries
enum { CMC_C_SPIN = 0, CMC_C_SPIN_ACC = 1, CMC_C_EDGE = 2, CMC_C_EDGE_ACC = 3, CMC_C_WORM = 4, CMC_C_WORM_ACC = 5, CMC_C_WORM_FAIL = 6, CMC_C_WORM_PATH = 7 };

// the graph accessor over tables in plain memory: the view of one replica (cmc_graph_mem).  J(k), cum(e) and totalw() are the only
// places that know the coupling format
struct CmcGraphMem {
    CmcTables T;
    const uint8_t *jcode; // the replica's codes / doubles (per-replica couplings), its running sums and their total
    const double *jr, *cum_r;
    double totalw_r;
    SSE_HD uint32_t N() const { return T.N; }
    SSE_HD uint32_t E() const { return T.E; }
    SSE_HD uint32_t row(uint32_t v) const { return T.row[v]; }
    SSE_HD uint32_t nbr(uint32_t k) const { return T.ent[k] & CMC_NBR_MASK; }
    SSE_HD double J(uint32_t k) const {
        if (T.flags & CMC_T_PER_REPLICA) return (T.flags & CMC_T_COMPACT) ? T.jv[jcode[k]] : jr[k];
        return T.jv[(T.flags & CMC_T_COMPACT) ? T.ent[k] >> 24 : k];
    }
    SSE_HD double bias(uint32_t v) const { return (T.flags & CMC_T_BIAS) ? T.bias[v] : 0.0; }
    SSE_HD void edge(uint32_t e, uint32_t &a, uint32_t &b) const {
        if (T.flags & CMC_T_EDGE16) { a = T.edges[e] & 0xFFFFu; b = T.edges[e] >> 16; }
        else { a = T.edges[2 * e]; b = T.edges[2 * e + 1]; }
    }
    SSE_HD bool importance() const { return (T.flags & CMC_T_CUM) != 0u; }
    SSE_HD double cum(uint32_t e) const { return cum_r[e]; }
    SSE_HD double totalw() const { return totalw_r; }
};
// the view of local replica r (with shared couplings every r gives the same view)
SSE_HD inline CmcGraphMem cmc_graph_mem(const CmcTables &T, uint32_t r) {
    if (!(T.flags & CMC_T_PER_REPLICA)) return CmcGraphMem{T, nullptr, nullptr, T.cum, T.totalw};
    const bool cum = (T.flags & CMC_T_CUM) != 0u;
    return CmcGraphMem{T, T.jcode ? T.jcode + (size_t)r * 4u * cmc_code_words(T.E) : nullptr, T.jr ? T.jr + (size_t)r * 2u * T.E : nullptr,
                       cum ? T.cum + (size_t)r * T.E : nullptr, cum ? T.totalw_r[r] : 0.0};
}

// ---- the random stream ----
SSE_HD inline uint32_t cmc_range(uint32_t word, uint32_t n) { return (uint32_t)(((uint64_t)word * (uint64_t)n) >> 32); } // __umulhi
SSE_HD inline double cmc_u01(uint32_t word) { return (double)word * (1.0 / 4294967296.0); }                             // [0, 1)
// Portable Philox4x32-10 for the host (the kernel draws the same integers with sse_core.hip.h's philox4x32_10)
struct CmcHostDraw {
    uint32_t k0, k1, replica, epoch_lo, epoch_hi24;
    uint32_t operator()(uint32_t tag, uint32_t index, int word) const {
        uint32_t c[4] = {index, epoch_lo, replica, (tag << 24) | epoch_hi24}, ka = k0, kb = k1;
        for (int i = 0; i < 10; ++i) {
            const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
            const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ ka, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ kb;
            c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
            ka += 0x9E3779B9u; kb += 0xBB67AE85u;
        }
        return c[word];
    }
};
#define CMC_INDEX_KIND 0u
SSE_HD inline uint32_t cmc_index_move(uint32_t i) { return 1u + i; } // word 0: the site or edge choice, word 1: the acceptance uniform
// the kind of a step, 0 spin, 1 edge, 2 worm (do_time_step, :364-365); forced kinds draw nothing
template <class Draw> SSE_HD inline uint32_t cmc_step_kind(uint32_t kinds, Draw draw) {
    if (kinds >= CMC_KINDS_SPIN) return kinds == CMC_KINDS_SPIN ? 0u : kinds == CMC_KINDS_EDGE ? 1u : 2u;
    return cmc_range(draw(SSE_TAG_CLASSICAL, CMC_INDEX_KIND, 0), kinds == CMC_KINDS_BASIC ? 2u : 3u);
}
// None of the reference's Option arguments (:361-363)
SSE_HD inline uint32_t cmc_default_moves(uint32_t given, uint32_t def) { return given == CMC_NONE ? (def ? def : 1u) : given; }

// ---- one move ----
// should_flip (:339-347)
SSE_HD inline bool cmc_should_flip(double beta, double de, uint32_t word) {
    if (de > 0.0) return cmc_u01(word) < exp(-beta * de);
    return true;
}
// delta_e (:155-176): in row order from 0.0, entries whose neighbour is `omit` left out (CMC_NONE: none)
template <class G, class S> SSE_HD inline double cmc_delta_e(const G &g, const S &s, uint32_t v, uint32_t omit) {
    const bool sv = s.get(v);
    double de = 0.0;
    for (uint32_t k = g.row(v), end = g.row(v + 1); k < end; ++k) {
        const uint32_t u = g.nbr(k);
        if (u == omit) continue;
        de += -2.0 * g.J(k) * (sv == s.get(u) ? 1.0 : -1.0);
    }
    return de;
}
template <class G, class S> SSE_HD inline double cmc_bias_e(const G &g, const S &s, uint32_t v) { return 2.0 * g.bias(v) * (s.get(v) ? 1.0 : -1.0); }
// do_spin_flip (:91-119)
template <class G, class S> SSE_HD inline double cmc_spin_de(const G &g, const S &s, uint32_t v) { return cmc_delta_e(g, s, v, CMC_NONE) + cmc_bias_e(g, s, v); }
// do_edge_flip (:122-153)
template <class G, class S> SSE_HD inline double cmc_edge_de(const G &g, const S &s, uint32_t a, uint32_t b) {
    return (cmc_delta_e(g, s, a, b) + cmc_bias_e(g, s, a)) + (cmc_delta_e(g, s, b, a) + cmc_bias_e(g, s, b));
}
// the edge of an edge move (:131-141): uniform, or by weight: the number of cumulative weights strictly below p = u * totalw
template <class G> SSE_HD inline uint32_t cmc_pick_edge(const G &g, uint32_t word) {
    if (!g.importance()) return cmc_range(word, g.E());
    const double p = cmc_u01(word) * g.totalw();
    uint32_t lo = 0, hi = g.E() - 1u; // cum[E - 1] = totalw > p: the answer is at most E - 1
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (g.cum(mid) < p) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// ---- the worm move (do_worm_flip, :179-318) ----
// A WormMove: Single(a) has b = CMC_NONE, Double(a, b) flips both.
struct CmcWormMove { uint32_t a, b; };
SSE_HD inline bool cmc_near(double x) { return fabs(x) < DBL_EPSILON; }
template <class G, class S> SSE_HD inline double cmc_worm_de(const G &g, const S &s, CmcWormMove m) { // the closure delta_e (:191-199)
    if (m.b == CMC_NONE) return cmc_delta_e(g, s, m.a, CMC_NONE);
    const double de = cmc_delta_e(g, s, m.a, m.b);
    return de + cmc_delta_e(g, s, m.b, m.a);
}
// The candidates of a path step in the reference's order (:214-242): for each neighbour ov of sel_var in row order (but last_index),
// Single(ov), then with doubles Double(ov, oov) over ov's row (but sel_var), ov pretended flipped.  visit(move, de) sees each one
// whose de is near 0 or near -starting_e; it returns true to stop the walk.
template <class G, class S, class Visit>
SSE_HD inline void cmc_worm_candidates(const G &g, S &s, uint32_t sel_var, uint32_t last_index, double starting_e, bool allow_doubles, Visit visit) {
    for (uint32_t k = g.row(sel_var), end = g.row(sel_var + 1); k < end; ++k) {
        const uint32_t ov = g.nbr(k);
        if (ov == last_index) continue;
        const double de = cmc_delta_e(g, s, ov, CMC_NONE);
        if (cmc_near(de) || cmc_near(de + starting_e)) { if (visit(CmcWormMove{ov, CMC_NONE}, de)) return; }
        if (!allow_doubles) continue;
        bool stop = false;
        s.flip(ov);
        for (uint32_t k2 = g.row(ov), end2 = g.row(ov + 1); k2 < end2 && !stop; ++k2) {
            const uint32_t oov = g.nbr(k2);
            if (oov == ov || oov == sel_var) continue;
            const double de2 = cmc_delta_e(g, s, oov, CMC_NONE) + de;
            if (cmc_near(de2) || cmc_near(de2 + starting_e)) stop = visit(CmcWormMove{ov, oov}, de2);
        }
        s.flip(ov); // return to normal
        if (stop) return;
    }
}
// One worm.  The candidate stack is not stored: a first walk counts the candidates near 0 (nzero), those near -starting_e (nres)
// and whether one of the latter is not also near 0 (any_resolve: then only the resolving ones stay, :243-245); a second walk stops at
// the chosen one.  The path is not stored either: its last move, its length and the marks that S::flip toggles are enough, because
// sort + remove_doubles (:297-298) leaves exactly the variables flipped an odd number of times: those that are marked.
// Draws (tag WORM, index *ndraw counted through the whole step, word 0) in program order: the start variable, one per path step that
// has candidates, and the final acceptance when the field energy is positive (should_flip draws nothing otherwise).
// S must come with no marks and is left with none.
template <class G, class S, class Draw>
SSE_HD inline void cmc_worm(const G &g, S &s, double beta, bool allow_doubles, Draw draw, uint32_t *ndraw, uint64_t *ctr) {
    const uint32_t N = g.N();
    const uint32_t start = cmc_range(draw(SSE_TAG_CLASSICAL_WORM, (*ndraw)++, 0), N);
    CmcWormMove sel{start, CMC_NONE};
    uint32_t last_index = start;
    uint64_t len = 1;
    const double starting_e = cmc_delta_e(g, s, start, CMC_NONE);
    s.flip(start);
    bool failed = false;
    for (;;) {
        const uint32_t sel_var = sel.b == CMC_NONE ? sel.a : sel.b;
        uint32_t nzero = 0, nres = 0;
        bool any_resolve = false;
        cmc_worm_candidates(g, s, sel_var, last_index, starting_e, allow_doubles, [&](CmcWormMove, double de) {
            const bool res = cmc_near(de + starting_e);
            if (cmc_near(de)) ++nzero; else any_resolve = true;
            if (res) ++nres;
            return false;
        });
        const uint32_t n = any_resolve ? nres : nzero;
        CmcWormMove ov;
        double de;
        if (n) {
            uint32_t left = cmc_range(draw(SSE_TAG_CLASSICAL_WORM, (*ndraw)++, 0), n);
            ov = CmcWormMove{CMC_NONE, CMC_NONE}; de = 0.0;
            cmc_worm_candidates(g, s, sel_var, last_index, starting_e, allow_doubles, [&](CmcWormMove m, double d) {
                if (any_resolve ? !cmc_near(d + starting_e) : !cmc_near(d)) return false;
                if (left--) return false;
                ov = m; de = d;
                return true;
            });
        } else { // no options: turn around, undo the last move (:253-262)
            ov = sel.b == CMC_NONE ? sel : CmcWormMove{sel.b, sel.a};
            de = cmc_worm_de(g, s, ov);
        }
        ++len;
        s.flip(ov.a);
        if (ov.b != CMC_NONE) s.flip(ov.b);
        last_index = ov.b == CMC_NONE ? sel_var : ov.a; // (:272-276)
        sel = ov;
        if (cmc_near(de + starting_e)) break; // back at the initial energy
        if (len > N) { failed = true; break; } // path getting too long
    }
    ctr[CMC_C_WORM] += 1; ctr[CMC_C_WORM_PATH] += len;
    bool keep = false;
    if (!failed) { // the energy change from the longitudinal fields, over the net-flipped variables in increasing order (:300-311)
        double total_he = 0.0;
        for (uint32_t v = 0; v < N; ++v) if (s.marked(v)) total_he += cmc_bias_e(g, s, v);
        keep = total_he > 0.0 ? cmc_should_flip(beta, total_he, draw(SSE_TAG_CLASSICAL_WORM, (*ndraw)++, 0)) : true;
    } else ctr[CMC_C_WORM_FAIL] += 1;
    if (keep) ctr[CMC_C_WORM_ACC] += 1;
    for (uint32_t v = 0; v < N; ++v) if (s.marked(v)) { if (!keep) s.flip(v); s.unmark(v); }
}

// get_energy (:430-447)
template <class G, class S> SSE_HD inline double cmc_energy_of(const G &g, const S &s, uint32_t v) {
    double total_e = 0.0;
    for (uint32_t k = g.row(v), end = g.row(v + 1); k < end; ++k) total_e += g.J(k) * (s.get(v) == s.get(g.nbr(k)) ? 1.0 : -1.0) / 2.0;
    return total_e; // the caller adds: acc + total_e + (s_v ? -bias : bias)
}
