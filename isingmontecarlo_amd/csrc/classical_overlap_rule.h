// classical_overlap_rule.h — the overlaps between copies of one realisation under classical tempering (classical_pt_rule.h), once: the
// layout of a batch as groups of copies, the pair of slots an item compares, and the two counts every overlap is made of.
//
// Layout.  Tempering is attached: the batch is C chains of T temperatures.  With ncopies = K >= 2, consecutive chains form G = C / K
// groups; group g holds the chains g K .. g K + K - 1, K independent copies of one realisation (moves are keyed by the replica index
// and swaps by the chain index, so the copies share nothing but their couplings).  The pairs of a group are (a, b) with
// 0 <= a < b < K, a-major then b; p is the pair's index, P = K (K - 1) / 2.  The global group index is (replica_offset / T + g K) / K,
// so C and replica_offset / T are multiples of K: a batch split over handles at whole groups measures the same thing.  With per-replica
// couplings the K chains of a group hold bit-identical coupling rows (+0 and -0 differ); with shared couplings every grouping is valid.
//
// What a round measures, after its time steps and before its swaps (the moment of the E and M series).  For group g, pair p = (a, b)
// and temperature t, A is the slot of chain g K + a that holds t, (g K + a) T + slot_at[(g K + a) T + t], B the same for chain
// g K + b, and d = state(A) xor state(B).
//   nq: the set bits of d among the N variables, 0 .. N.  The spin overlap is Q = N - 2 nq = sum_v sigma_v^A sigma_v^B.
//   nl: the edges e = 0 .. E - 1 of the edge list, by g.edge(e, i, j), with d_i != d_j, 0 .. E.  The link overlap is
//       QL = E - 2 nl = sum_e (sigma_i sigma_j)^A (sigma_i sigma_j)^B.  Every entry of the edge list counts once, multi-edges apiece,
//       and the value of J does not matter (zero couplings count too).
// Outputs: the series overlap[round][g][p][t] = Q and link_overlap[round][g][p][t] = QL (int32), and the histograms
// hq[g][p][t][nq] (N + 1 bins) and hl[g][p][t][nl] (E + 1 bins) (uint64), +1 per measured round.  Sticky error flags of slots do not
// alter the measurement.  Everything is an integer.
// Three consumers: classical_overlap_kernel (sse_classical_overlap.hip.h), isingmc_classical_host_pt_run_overlaps (classical_host.hip)
// and the tests.  Plain inline functions, no device code: hipcc compiles them for the kernel, a host C++ compiler takes the header as
// it is.
#pragma once
#include <stdint.h>
#include "classical_rule.h"

SSE_HD inline uint64_t cmc_ov_pairs(uint32_t K) { return (uint64_t)K * (K - 1u) / 2u; }
// the copies (a, b) of pair p: a-major then b
SSE_HD inline void cmc_ov_pair(uint32_t K, uint32_t p, uint32_t &a, uint32_t &b) {
    a = 0u;
    for (uint32_t row = K - 1u; p >= row; p -= row, --row) ++a; // row: the pairs that start with a
    b = a + 1u + p;
}
// the slot of chain `chain` that holds temperature t
SSE_HD inline uint32_t cmc_ov_slot(const uint32_t *slot_at, uint32_t T, uint32_t chain, uint32_t t) { return chain * T + slot_at[chain * T + t]; }
// the item (g, p, t) of a flat index, t fastest
SSE_HD inline void cmc_ov_item(uint64_t item, uint32_t P, uint32_t T, uint32_t &g, uint32_t &p, uint32_t &t) {
    t = (uint32_t)(item % T);
    p = (uint32_t)((item / T) % P);
    g = (uint32_t)(item / T / P);
}

// d = A xor B, bit by bit
template <class S> SSE_HD inline bool cmc_ov_differ(const S &A, const S &B, uint32_t v) { return A.get(v) != B.get(v); }
// the share of nq of one of `stride` workers: the variables first, first + stride, ...
template <class S> SSE_HD inline uint32_t cmc_ov_count_spins(uint32_t N, const S &A, const S &B, uint32_t first, uint32_t stride) {
    uint32_t n = 0;
    for (uint32_t v = first; v < N; v += stride) n += cmc_ov_differ(A, B, v) ? 1u : 0u;
    return n;
}
// the share of nl: the edges first, first + stride, ...
template <class G, class S> SSE_HD inline uint32_t cmc_ov_count_links(const G &g, const S &A, const S &B, uint32_t first, uint32_t stride) {
    uint32_t n = 0;
    for (uint32_t e = first; e < g.E(); e += stride) {
        uint32_t i, j;
        g.edge(e, i, j);
        n += cmc_ov_differ(A, B, i) != cmc_ov_differ(A, B, j) ? 1u : 0u;
    }
    return n;
}
SSE_HD inline int32_t cmc_ov_overlap(uint32_t total, uint32_t differing) { return (int32_t)total - 2 * (int32_t)differing; } // Q of (N, nq), QL of (E, nl)
