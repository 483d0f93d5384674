// sse_classical_icm.hip.h — the cluster-move launch of classical tempering for gfx950 (the rule: classical_icm_rule.h).
//
// One wave per item (g, m, t) of the window, t fastest, W = 4, 2 or 1 waves per workgroup (CmcIcmCarve), ceil(items / W) workgroups.
// A wave whose item is past the end leaves as a whole.  A wave keeps three bit sets of nwords words in its own LDS area: d, the cluster
// and the frontier.
//   d and nq: the lanes stride over the words of both states, XOR them (the bits behind N masked in the last word) and count bits.
//   The seed: the k-th set bit of d, by a wave prefix sum of the words' population counts, 64 words a trip with a running total.
//   Growth: lane l takes the frontier words l, l + 64, ... (an atomic exchange with 0 takes a word's bits), walks the rows of their
//   variables in global memory and ORs every newly reached d-variable into the cluster and into the frontier with LDS atomics.  Bits
//   that arrive in a word after its exchange stay for the next pass.  The loop ends after a pass in which no lane took a bit: no one
//   added one either.  The cluster is a set, so the order of expansion does not show.
//   Apply: the lanes stride over the words and XOR the cluster into both states; lane 0 adds to the item's three counts with a plain
//   load, add and store (every item owns its counts, and launches are ordered by their stream).
// The trip count of the growth loop differs from wave to wave, so there is no workgroup barrier anywhere: every LDS word belongs to
// one wave, whose LDS operations execute in order; SSE_WAVE_FENCE keeps the compiler from moving them across the phases.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "classical_icm_rule.h"
#include "classical_launch.h"
#include "sse_core.hip.h" // philox4x32_10, lds_raw, sse_ballot

namespace sse {

#define CMC_ICM_MAX_WAVES 4u

__global__ __launch_bounds__(64 * CMC_ICM_MAX_WAVES) void classical_icm_kernel(CmcDev D, CmcPtDev P, CmcOvDev O, CmcIcmDev I, uint64_t pt_step) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t item = (uint64_t)blockIdx.x * I.C.W + wave;
    if (wave >= I.C.W || item >= (uint64_t)O.G * I.M * (I.t_last - I.t_first)) return; // the whole wave
    uint32_t grp, m, t, a, b;
    cmc_icm_item(item, I.M, I.t_first, I.t_last, grp, m, t);
    cmc_icm_pair(O.K, pt_step, m, a, b);
    const uint32_t ra = cmc_ov_slot(P.slot_at, P.T, grp * O.K + a, t), rb = cmc_ov_slot(P.slot_at, P.T, grp * O.K + b, t);
    uint32_t *A = D.state + (size_t)ra * D.nwords, *B = D.state + (size_t)rb * D.nwords;
    const uint32_t N = D.T.N, nw = I.C.nwords;
    const uint32_t o_d = wave * I.C.wave_words, o_cl = o_d + nw, o_fr = o_cl + nw;
    const size_t at = cmc_icm_count_index(I.M, P.T, grp, m, t);

    uint32_t nq = 0;
    for (uint32_t j = lane; j < nw; j += 64u) {
        uint32_t d = A[j] ^ B[j];
        if (j == nw - 1u && (N & 31u)) d &= (1u << (N & 31u)) - 1u;
        LDSW(o_d, j) = d; LDSW(o_cl, j) = 0u; LDSW(o_fr, j) = 0u;
        nq += __popc(d);
    }
    for (int o = 32; o > 0; o >>= 1) nq += __shfl_xor(nq, o, 64);
    if (nq == 0u) { // (one value for the wave)
        if (lane == 0u) I.empty[at] = I.empty[at] + 1u;
        return;
    }
    uint32_t c[4];
    cmc_icm_counter(P.T, pt_step, (D.replica_offset / P.T + grp * O.K) / O.K, m, t, c);
    const uint32_t k = cmc_range(philox4x32_10(c[0], c[1], c[2], c[3], D.seed_lo, D.seed_hi).x, nq);
    SSE_WAVE_FENCE();

    // the k-th set bit of d: 64 words a trip, `before` the bits of the trips so far
    uint32_t seed = 0;
    for (uint32_t base = 0, before = 0; base < nw; base += 64u) {
        const uint32_t j = base + lane, w = j < nw ? LDSW(o_d, j) : 0u, cnt = __popc(w);
        uint32_t incl = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= (uint32_t)o) incl += up;
        }
        const uint32_t first = before + incl - cnt; // the rank of the word's lowest set bit
        const bool mine = cnt != 0u && first <= k && k < first + cnt;
        const uint64_t hit = sse_ballot(mine);
        if (hit) { // (one lane)
            uint32_t v = 0;
            if (mine) v = j * 32u + cmc_icm_nth_bit(w, k - first);
            seed = __shfl(v, __builtin_ctzll(hit), 64);
            break;
        }
        before += __shfl(incl, 63, 64);
    }
    if (lane == 0u) {
        LDSW(o_cl, seed >> 5) = 1u << (seed & 31u);
        LDSW(o_fr, seed >> 5) = 1u << (seed & 31u);
    }
    SSE_WAVE_FENCE();

    for (;;) { // growth: a pass over the frontier words
        bool took = false;
        for (uint32_t j = lane; j < nw; j += 64u) {
            if (LDSW(o_fr, j) == 0u) continue;
            uint32_t f = atomicExch(&LDSW(o_fr, j), 0u);
            took |= f != 0u;
            while (f) {
                const uint32_t v = j * 32u + (uint32_t)__builtin_ctz(f);
                f &= f - 1u;
                for (uint32_t e = D.T.row[v], end = D.T.row[v + 1u]; e < end; ++e) {
                    const uint32_t u = D.T.ent[e] & CMC_NBR_MASK, bit = 1u << (u & 31u);
                    if (!(LDSW(o_d, u >> 5) & bit)) continue;
                    if (!(atomicOr(&LDSW(o_cl, u >> 5), bit) & bit)) atomicOr(&LDSW(o_fr, u >> 5), bit); // newly reached
                }
            }
        }
        SSE_WAVE_FENCE();
        if (!sse_any(took)) break;
    }

    uint32_t size = 0;
    for (uint32_t j = lane; j < nw; j += 64u) {
        const uint32_t cl = LDSW(o_cl, j);
        if (cl) { A[j] ^= cl; B[j] ^= cl; }
        size += __popc(cl);
    }
    for (int o = 32; o > 0; o >>= 1) size += __shfl_down(size, o, 64);
    if (lane == 0u) {
        I.moves[at] = I.moves[at] + 1u;
        I.size_sum[at] = I.size_sum[at] + size;
    }
}

} // namespace sse
