// classical_pt_rule.h — replica exchange for batches of classical replicas (GraphState), once: the layout of a batch as chains of
// temperatures, the energy and magnetisation of a slot in a fixed order of additions, the acceptance test of a pair and one
// tempering step of a chain.  The decision stream and the walk over the two pair sets are pt_rule.h's, unchanged.
//
// Layout.  A batch of R replicas is C chains of T temperatures, R = C T, slot r = c T + i.  betas[T] is one ladder shared by all
// chains (finite, any order, equal neighbours allowed).  temp_of[r] is the temperature index that slot r holds, slot_at[c T + t] its
// inverse; initially temp_of[c T + i] = i.  A swap exchanges temperature labels: states, epochs, move counters and each replica's
// Philox stream (keyed by replica_offset + r) never move.  The global chain index is replica_offset / T + c.
//
// Energy of a slot, bit for bit (the order of classical_energies_kernel).  Lane l of 64 folds
//     e = e + cmc_energy_of(g, s, v) + (s_v ? -bias_v : bias_v)      over v = l, l + 64, ..., from 0.0,
// then a tree over the offsets o = 32, 16, .., 1 adds p[l] += p[l + o] for l < o; the energy is p[0].  Every term of cmc_energy_of is
// J (+-1) / 2, which is exact, so the bits depend only on the order of the additions.  The magnetisation M = sum_v (2 s_v - 1) is an
// int32 from population counts and is exact.
//
// One round: every slot takes `steps` time steps at betas[temp_of[r]]; E and M of every slot are computed (a recorded series holds
// them by temperature, series[round][c][temp_of[r]], before the round's swaps); every chain takes one tempering step at the handle's
// step number pt_step; pt_step increments.
// Three consumers: classical_tempering_kernel (sse_classical_pt.hip.h), isingmc_classical_host_pt_run (classical_host.hip) and the tests.
// Plain inline functions, no device code: hipcc compiles them for the kernel, a host C++ compiler takes the header as it is.
#pragma once
#include <math.h>
#include <stdint.h>
#include "classical_rule.h"
#include "pt_rule.h"

#define CMC_PT_LANES 64u

// ---- energy and magnetisation ----
// the fold of lane `lane` over its variables
template <class G, class S> SSE_HD inline double cmc_pt_lane_energy(const G &g, const S &s, uint32_t lane) {
    double e = 0.0;
    for (uint32_t v = lane; v < g.N(); v += CMC_PT_LANES) e = e + cmc_energy_of(g, s, v) + (s.get(v) ? -g.bias(v) : g.bias(v));
    return e;
}
// the whole sum on one thread: the 64 folds, then the tree
template <class G, class S> inline double cmc_pt_energy(const G &g, const S &s) {
    double p[CMC_PT_LANES];
    for (uint32_t l = 0; l < CMC_PT_LANES; ++l) p[l] = cmc_pt_lane_energy(g, s, l);
    for (uint32_t o = CMC_PT_LANES / 2u; o > 0u; o >>= 1)
        for (uint32_t l = 0; l < o; ++l) p[l] += p[l + o];
    return p[0];
}
template <class G, class S> inline int32_t cmc_pt_magnetization(const G &g, const S &s) {
    int32_t up = 0;
    for (uint32_t v = 0; v < g.N(); ++v) up += s.get(v) ? 1 : 0;
    return 2 * up - (int32_t)g.N();
}

// ---- the acceptance test ----
// The pair (t, t + 1): e_t is the energy of the slot that holds temperature t, u uniform in [0, 1).  No case split: a non-negative
// exponent gives a value >= 1 > u.
SSE_HD inline bool cmc_pt_accept(double beta_t, double beta_t1, double e_t, double e_t1, double u) {
    return exp((beta_t - beta_t1) * (e_t - e_t1)) > u;
}

// ---- one tempering step ----
// One chain's share of the arrays: betas [T]; temp_of, slot_at and energy from the chain's first slot ([T]; temp_of and energy are
// indexed by the slot within the chain, slot_at holds such slots); attempts and accepts [T - 1] (either may be null).
struct CmcPtChainView {
    uint32_t T;
    const double *betas;
    uint32_t *temp_of, *slot_at;
    const double *energy;
    uint64_t *attempts, *accepts;
};
// An attempt on the pair (t, t + 1) with the uniform u.  The pairs of a phase are disjoint: their attempts touch different entries.
SSE_HD inline bool cmc_pt_attempt(const CmcPtChainView &c, uint32_t t, double u) {
    const uint32_t a = c.slot_at[t], b = c.slot_at[t + 1u];
    const bool acc = cmc_pt_accept(c.betas[t], c.betas[t + 1u], c.energy[a], c.energy[b], u); // energies belong to slots
    if (c.attempts) c.attempts[t] += 1u;
    if (acc) {
        c.slot_at[t] = b; c.slot_at[t + 1u] = a;
        c.temp_of[a] = t + 1u; c.temp_of[b] = t;
        if (c.accepts) c.accepts[t] += 1u;
    }
    return acc;
}
// The step of chain k (its global index) at step number pt_step, on one thread
template <class Draw> inline void cmc_pt_chain_step(uint64_t seed, uint64_t pt_step, uint32_t k, const CmcPtChainView &c, Draw draw) {
    const PtChain pc = pt_chain(seed, pt_step, k);
    const bool a_first = pt_a_first(pc, draw);
    for (int phase = 0; phase < 2; ++phase)
        pt_walk_phase(pc, a_first, phase, 0u, c.T - 1u, draw, [&](uint32_t t, double u) { cmc_pt_attempt(c, t, u); });
}

// is temp_of [R] a permutation of 0 .. T - 1 within every chain?
inline bool cmc_pt_is_permutation(const uint32_t *temp_of, uint32_t R, uint32_t T, uint8_t *seen /* [T] scratch */) {
    for (uint32_t c = 0; c < R / T; ++c) {
        for (uint32_t t = 0; t < T; ++t) seen[t] = 0;
        for (uint32_t i = 0; i < T; ++i) {
            const uint32_t t = temp_of[c * T + i];
            if (t >= T || seen[t]) return false;
            seen[t] = 1;
        }
    }
    return true;
}
