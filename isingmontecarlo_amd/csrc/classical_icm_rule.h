// classical_icm_rule.h — isoenergetic cluster moves (Houdayer moves) between copies of one realisation under classical tempering,
// once: the pairs of a round, the item a wave or a loop iteration works on, the draw of the seed variable, and the cluster.
//
// Layout.  Tempering and overlaps are attached: the batch is G groups of K copies (chains) of T temperatures, as
// classical_overlap_rule.h defines them.  Cluster moves are attached with a window t_first <= t < t_last of ladder indices; outside
// the window nothing happens and nothing is counted.
//
// Pairs of a round.  M = K / 2 pairs (rounded down) and o = pt_step % K: pair m is the copies a = (o + 2 m) mod K and
// b = (o + 2 m + 1) mod K.  The pairs of a round are disjoint; K = 3 leaves one copy idle each round and rotates, K = 4 alternates
// partners.  An item is (g, m, t), t fastest, over the window's temperatures only.  A and B are the slots of the chains g K + a and
// g K + b that hold t (cmc_ov_slot).
//
// The move of an item.  d = state(A) xor state(B), nq its population count.  nq = 0: the item counts as empty and nothing moves.
// Otherwise one Philox word is drawn from the counter (index = m T + t, step_lo, global group index, SSE_TAG_CLASSICAL_ICM << 24 |
// step_hi24) keyed by the seed (step = pt_step; the global group index is classical_overlap_rule.h's), k = cmc_range(word, nq), and the
// seed variable is the k-th set bit of d in increasing variable order.  The cluster is the connected component of the seed in the
// subgraph induced on {v : d_v = 1} by the rows of the graph's CSR: every entry of the edge list connects, whatever its J (zero
// couplings and multi-edges included; no coupling is read).  Every variable of the cluster is flipped in A and in B.
//
// What the move leaves alone: epochs, move counters, maps and each replica's Philox stream; d, and with it Q and QL; E_A + E_B, biases
// included (s^A = -s^B on the cluster, and a cluster has no edge to a differing variable outside it).
// Counts per item, uint64 [G][M][T] each, cumulative: moves, empty, size_sum (cluster sizes added up).
// Place in a round: the steps, then the overlap measurement when it is on, then the cluster moves, then the tempering step, whose E
// and M are therefore those after the moves.
// Three consumers: classical_icm_kernel (sse_classical_icm.hip.h), isingmc_classical_host_pt_run_icm (classical_host.hip) and the tests.
// Plain inline functions, no device code: hipcc compiles them for the kernel, a host C++ compiler takes the header as it is.
#pragma once
#include <stdint.h>
#include "classical_overlap_rule.h"

SSE_HD inline uint32_t cmc_icm_pairs(uint32_t K) { return K / 2u; }
// the copies (a, b) of pair m in the round of step number pt_step
SSE_HD inline void cmc_icm_pair(uint32_t K, uint64_t pt_step, uint32_t m, uint32_t &a, uint32_t &b) {
    const uint32_t o = (uint32_t)(pt_step % K);
    a = (o + 2u * m) % K;
    b = (o + 2u * m + 1u) % K;
}
// the item (g, m, t) of a flat index over the window, t fastest
SSE_HD inline void cmc_icm_item(uint64_t item, uint32_t M, uint32_t t_first, uint32_t t_last, uint32_t &g, uint32_t &m, uint32_t &t) {
    const uint32_t Tw = t_last - t_first;
    t = t_first + (uint32_t)(item % Tw);
    m = (uint32_t)((item / Tw) % M);
    g = (uint32_t)(item / Tw / M);
}
// where the counts of item (g, m, t) are: the arrays span every temperature
SSE_HD inline size_t cmc_icm_count_index(uint32_t M, uint32_t T, uint32_t g, uint32_t m, uint32_t t) { return ((size_t)g * M + m) * T + t; }
// the counter of an item's draw: c[0] .. c[3] (the key is the seed)
SSE_HD inline void cmc_icm_counter(uint32_t T, uint64_t pt_step, uint32_t group, uint32_t m, uint32_t t, uint32_t c[4]) {
    c[0] = m * T + t;
    c[1] = (uint32_t)pt_step;
    c[2] = group;
    c[3] = (SSE_TAG_CLASSICAL_ICM << 24) | ((uint32_t)(pt_step >> 32) & 0xFFFFFFu);
}
// the position of the k-th set bit of w (k = 0: the lowest); w has more than k set bits
SSE_HD inline uint32_t cmc_icm_nth_bit(uint32_t w, uint32_t k) {
    for (; k; --k) w &= w - 1u;
    uint32_t p = 0;
    while (!((w >> p) & 1u)) ++p;
    return p;
}

// The sequential form, for the host: diff [N] bytes holds d; the seed is the rank-th variable with diff != 0 (rank < nq); mark [N]
// comes zeroed and leaves with 1 on the cluster; stack [N] is scratch.  Returns the size of the cluster.
template <class G> inline uint32_t cmc_icm_grow(const G &g, const uint8_t *diff, uint32_t rank, uint8_t *mark, uint32_t *stack) {
    uint32_t seed = 0;
    for (uint32_t left = rank;; ++seed)
        if (diff[seed] && left-- == 0u) break;
    uint32_t top = 0, size = 1;
    mark[seed] = 1u;
    stack[top++] = seed;
    while (top) {
        const uint32_t v = stack[--top];
        for (uint32_t k = g.row(v), end = g.row(v + 1u); k < end; ++k) {
            const uint32_t u = g.nbr(k);
            if (!diff[u] || mark[u]) continue;
            mark[u] = 1u;
            stack[top++] = u;
            ++size;
        }
    }
    return size;
}
