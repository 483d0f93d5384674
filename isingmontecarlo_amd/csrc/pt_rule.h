// pt_rule.h — the swap rule of a tempering step (TemperingContainer::tempering_step, tempering_container.rs:121-149; swap_on_chunks
// :241-302), once: the decision stream, the acceptance test and the walk of one chain through one phase.
//
// A step of chain k draws from the Philox stream (index, step_lo, k, SSE_TAG_PT << 24 | step_hi24) keyed by the seed: index 0 is the
// order coin (gen_bool(0.5), :140: which of the two pair sets goes first), index 1 + t the uniform of the pair (t, t + 1).  Set a holds
// the pairs with even t, set b those with odd t (make_first/second_subgraphs, :83-99); a phase visits one set in increasing t.
// Three consumers (pt.hip): isingmc_pt_decide (a whole ladder on the host), pt_decide_kernel (one thread per chain) and
// isingmc_pt_plan_phase (one rank's share of a phase).  The kernel draws with sse_core.hip.h's philox4x32_10 (gfx950 builtins), the
// host with pt_philox_word below: the same integers, so the draw is a parameter of the walk.
// Plain inline functions: hipcc compiles them for the kernel, a host C++ compiler for tests/test_pt_rule_cpu.py (no HIP header needed).
#pragma once
#include <stdint.h>
#include "../../include/sse_format.h" // SSE_TAG_PT

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_RULE_FN __host__ __device__ inline
#else
#define PT_RULE_FN inline
#endif

// ---- the decision stream ----
struct PtChain { uint32_t step_lo, chain, tag_step_hi, key0, key1; }; // counter words 1..3 and the key; word 0 is the index
PT_RULE_FN PtChain pt_chain(uint64_t seed, uint64_t step, uint32_t chain) {
    return {(uint32_t)step, chain, (SSE_TAG_PT << 24) | (uint32_t)((step >> 32) & 0xFFFFFFu), (uint32_t)seed, (uint32_t)(seed >> 32)};
}
#define PT_INDEX_COIN 0u
PT_RULE_FN uint32_t pt_index_pair(uint32_t t) { return 1u + t; }
PT_RULE_FN bool pt_coin(uint32_t word) { return (word >> 31) != 0u; }                       // true: set a goes first
PT_RULE_FN double pt_uniform(uint32_t word) { return (double)word * (1.0 / 4294967296.0); } // [0, 1)

// Portable Philox4x32-10, first output word (control logic on the host, not the sweep path)
PT_RULE_FN uint32_t pt_philox_word(const PtChain &c, uint32_t index) {
    uint32_t c0 = index, c1 = c.step_lo, c2 = c.chain, c3 = c.tag_step_hi, k0 = c.key0, k1 = c.key1;
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
struct PtHostDraw { PT_RULE_FN uint32_t operator()(const PtChain &c, uint32_t index) const { return pt_philox_word(c, index); } };
// a draw is any  uint32_t draw(const PtChain &, uint32_t index)  that returns the first Philox word of that counter
template <class Draw> PT_RULE_FN bool pt_a_first(const PtChain &c, Draw draw) { return pt_coin(draw(c, PT_INDEX_COIN)); }

// ---- the acceptance test ----
// f64::powi as Rust lowers it (compiler-rt __powidf2): squaring sequence, reciprocal for negative exponents.  Multiplications
// and one division only: the host and the device give the same bits (as does the oracle, which multiplies in the same order)
PT_RULE_FN double pt_powi(double x, int64_t n) {
    uint64_t m = n < 0 ? (uint64_t)(-n) : (uint64_t)n;
    double r = 1.0;
    while (m) { if (m & 1u) r *= x; x *= x; m >>= 1; }
    return n < 0 ? 1.0 / r : r;
}
// The swap test of a pair of neighbouring temperatures t, t + 1 (swap_on_chunks, tempering_container.rs:296-298): the walker at t
// holds n_a ops, the one at t + 1 n_b; rel = the product of their relative weights under each other's Hamiltonian (1 when the
// Hamiltonians are equal: a multiplication by 1.0 changes no bit); u uniform in [0, 1)
PT_RULE_FN bool pt_accept(double beta_t, double beta_t1, uint32_t n_a, uint32_t n_b, double rel, double u) {
    return pt_powi(beta_t / beta_t1, (int64_t)n_b - (int64_t)n_a) * rel > u;
}

// ---- the walk ----
// does the pair (t, t + 1) belong to `phase` (0, 1) of a chain whose coin said a_first?
PT_RULE_FN bool pt_in_phase(bool a_first, int phase, uint32_t t) { return ((t & 1u) == 0u) == ((phase == 0) ? a_first : !a_first); }
// One phase of one chain over the pairs (t, t + 1), t_begin <= t < t_end, in increasing t: attempt(t, u) with the pair's uniform u.
// Pairs of a phase are disjoint, so attempt may swap the two walkers at once.
template <class Draw, class Attempt>
PT_RULE_FN void pt_walk_phase(const PtChain &c, bool a_first, int phase, uint32_t t_begin, uint32_t t_end, Draw draw, Attempt attempt) {
    for (uint32_t t = t_begin + (pt_in_phase(a_first, phase, t_begin) ? 0u : 1u); t < t_end; t += 2) attempt(t, pt_uniform(draw(c, pt_index_pair(t))));
}
