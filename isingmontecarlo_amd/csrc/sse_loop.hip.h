// sse_loop.hip.h — the directed-loop update (sse::sweep_kernel, sse_sweep.hip.h, and the trimmed diagonal kernel, sse_fast.hip.h).
#pragma once
#include "sse_core.hip.h"

namespace sse {

// Directed loop.  Reference: LoopUpdater::make_loop_update_with_rng (qmc_traits/directed_loop.rs:103-171)
// and loop_body (:217-301).  One loop per call; the walk itself is sequential (thread 0), the two things the
// reference does with linked lists are done cooperatively by the whole workgroup:
//   get_nth_p (:76-87, an O(n) list walk)        -> tile-wise ballot/popcount rank search
//   get_next/previous_p_for_rel_var (:51-54)     -> tile-wise search along the worldline direction
// Returns the number of vertices visited.
template <int W, bool CL, bool PM = false>
__device__ __forceinline__ uint32_t loop_pass(const DevBatch &B, const Lds<W> &L, uint32_t r, const Rng &rng, uint32_t M, int n, uint32_t &gr,
                              uint32_t &err) {
    constexpr int NT = W * 64;
    constexpr int U = 4; // independent loads in flight per thread during searches
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6); // scalar: keeps per-wave control flow uniform
    uint32_t *ops = B.ops + (size_t)r * B.stride;
    if (n == 0) return 0u;
    const uint4 o0 = rng.draw(SSE_TAG_LOOP, 0u);
    const uint32_t nth = __umulhi(o0.x, (uint32_t)n);
    // ---- start vertex: the nth occupied slot in p order.  The per-chunk occupancy kept by the diagonal pass
    // names the chunk; only that chunk is scanned (sub-tiles of U*NT slots, wave-major inside) ----
    uint32_t cbase = 0, qbeg = 0, qend = M;
    {
        const uint32_t used = (M + B.CH - 1) / B.CH;
        for (uint32_t c = 0; c < used; ++c) {
            const uint32_t cn = LDSW(L.o_chn, c);
            if (nth < cbase + cn) { qbeg = c * B.CH; qend = min(qbeg + B.CH, M); break; }
            cbase += cn;
        }
    }
    if (tid == 0) LDSW(L.o_misc, MISC_LOOP_A) = 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t q0 = qbeg; q0 < qend; q0 += U * NT) {
        uint32_t wd[U];
        uint64_t occ[U];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < U; ++j) { const uint32_t p = q0 + (uint32_t)(wave * 64 * U + j * 64 + lane); wd[j] = p < qend ? ops[p] : 0u; }
#pragma unroll
        for (int j = 0; j < U; ++j) { occ[j] = sse_ballot(wd[j] != 0u); cnt += popc64(occ[j]); }
        const int buf = gr & 1;
        if (lane == 0) LDSI(L.o_tot, buf * W + wave) = cnt;
        __syncthreads();
        gr++;
        uint32_t wbase = 0, total = 0;
#pragma unroll
        for (int w2 = 0; w2 < W; ++w2) { const uint32_t t = (uint32_t)LDSI(L.o_tot, buf * W + w2); if (w2 < wave) wbase += t; total += t; }
        uint32_t run = cbase + wbase;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const uint32_t myrank = run + popc64(occ[j] & lanemask_lt(lane));
            if (wd[j] != 0u && myrank == nth) LDSW(L.o_misc, MISC_LOOP_A) = q0 + (uint32_t)(wave * 64 * U + j * 64 + lane);
            run += popc64(occ[j]);
        }
        cbase += total;
        if (cbase > nth) break;
    }
    __syncthreads();
    const uint32_t p0 = LDSW(L.o_misc, MISC_LOOP_A);
    if (p0 == 0xFFFFFFFFu) { err = SSE_ERR_COUNT; return 0u; } // n inconsistent with the op-string
    // the word at the current vertex travels with the walk: the search below hands over the word it found together with the
    // distance (one 64-bit LDS minimum), so a vertex costs one round trip to the op-string instead of three
    const uint32_t o64 = (L.o_misc + 7u) & ~1u; // an 8-byte aligned pair inside o_misc[6, 9)
    uint32_t cur_word = ops[p0];
    uint32_t rel0, side0;
    {
        const Bd d0 = decode_bond<CL, W, PM>(B, L, sse_op_bond(cur_word));
        const uint32_t k0 = d0.c != SSE_NO_VAR ? 2u : 1u;
        rel0 = __umulhi(o0.y, k0);
        side0 = (o0.z >> 31) ? 0u : 1u; // gen() true -> Inputs (directed_loop.rs:153-157)
    }
    uint32_t p = p0, rel = rel0, side = side0, visited = 0;
    const uint32_t max_steps = 64u * M + 1024u; // the reference's loop is unbounded (directed_loop.rs:217-301); past this the replica reports ISINGMC_ELIMIT (clearable)
    bool finished = false;
    // A walk is one dependent chain (the longest of a batch's walks ends the launch), so what can be taken off the chain is: the
    // random numbers (64 steps' worth at a time, lane l of every wave holding step base + l: one Philox evaluation per 64 steps instead
    // of one per step on the single working lane), and the first search step's loads (both directions are requested before the
    // vertex update decides which one it will be: the loads fly while thread 0 computes).
    const bool spec = M > 2u * (uint32_t)(U * NT); // (the speculative rows then never reach the vertex itself, whose word is being rewritten)
    uint32_t ox = 0u;
    for (uint32_t step = 1; step <= max_steps; ++step) {
        if (((step - 1u) & 63u) == 0u) ox = rng.draw(SSE_TAG_LOOP, step + (uint32_t)lane).x;
        const uint32_t ux = (uint32_t)__builtin_amdgcn_readlane((int)ox, (int)((step - 1u) & 63u));
        uint32_t wf[U], wb[U];
        if (spec) {
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const uint32_t d = 1u + (uint32_t)(j * NT + tid);
                uint32_t qf = p + d, qb = p + M - d;
                if (qf >= M) qf -= M;
                if (qb >= M) qb -= M;
                wf[j] = ops[qf]; wb[j] = ops[qb];
            }
        }
        // ---- vertex update by thread 0 ----
        if (tid == 0) {
            const uint32_t word = cur_word;
            const Bd d = decode_bond<CL, W, PM>(B, L, sse_op_bond(word));
            const uint32_t k = d.c != SSE_NO_VAR ? 2u : 1u;
            uint32_t in_e = sse_op_in(word), out_e = sse_op_out(word);
            if (side == 0u) in_e ^= 1u << rel; else out_e ^= 1u << rel;
            double wl[4], total = 0.0;
            for (uint32_t leg = 0; leg < 2u * k; ++leg) {
                uint32_t i2 = in_e, o2 = out_e;
                if (leg < k) i2 ^= 1u << leg; else o2 ^= 1u << (leg - k);
                wl[leg] = op_weight(B, sse_op_bond(word), d, i2, o2);
                total += wl[leg];
            }
            double c = u01(ux) * total;
            uint32_t exit_leg = 2u * k - 1u;
            for (uint32_t leg = 0; leg < 2u * k; ++leg) {
                if (c < wl[leg]) { exit_leg = leg; break; }
                c -= wl[leg];
            }
            const uint32_t xside = exit_leg < k ? 0u : 1u, xrel = exit_leg < k ? exit_leg : exit_leg - k;
            if (xside == 0u) in_e ^= 1u << xrel; else out_e ^= 1u << xrel;
            ops[p] = (word & ~0xFu) | in_e | (out_e << SSE_OP_OUT_SHIFT);
            const bool closed = (p == p0 && xrel == rel0 && xside == side0);
            const uint32_t var = xrel == 0u ? d.a : d.c;
            LDSW(L.o_misc, MISC_LOOP_A) = closed ? 1u : 0u;
            LDSW(L.o_misc, MISC_LOOP_B) = var;
            LDSW(L.o_misc, MISC_LOOP_C) = xside | (xrel << 1) | ((((xside == 1u ? out_e : in_e) >> xrel) & 1u) << 2);
            LDSW(o64, 0) = 0xFFFFFFFFu; LDSW(o64, 1) = 0xFFFFFFFFu; // best (distance << 32 | word found there)
        }
        __syncthreads();
        visited++;
        if (LDSW(L.o_misc, MISC_LOOP_A)) { finished = true; break; }
        const uint32_t var = LDSW(L.o_misc, MISC_LOOP_B);
        const uint32_t info = LDSW(L.o_misc, MISC_LOOP_C);
        const uint32_t xside = info & 1u, newbit = (info >> 2) & 1u;
        const bool forward = xside == 1u;
        // ---- search the next op on worldline `var`, distance 1..M (distance M = the op itself) ----
        uint32_t found = 0xFFFFFFFFu, found_word = 0u;
        for (uint32_t d0 = 1; d0 <= M; d0 += U * NT) {
            uint32_t wd[U];
            if (spec && d0 == 1u) {
#pragma unroll
                for (int j = 0; j < U; ++j) wd[j] = forward ? wf[j] : wb[j];
            } else {
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const uint32_t d = d0 + (uint32_t)(j * NT + tid);
                    wd[j] = 0u;
                    if (d <= M) {
                        uint32_t q = forward ? p + d : p + M - d;
                        if (q >= M) q -= M;
                        wd[j] = ops[q];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                bool match = false;
                if (wd[j]) {
                    const Bd d = decode_bond<CL, W, PM>(B, L, sse_op_bond(wd[j]));
                    match = d.a == var || d.c == var;
                }
                // (a worldline holds an op every few hundred slots: a handful of lanes per step get here)
                if (match) atomicMin(reinterpret_cast<unsigned long long *>(&LDSW(o64, 0)), ((unsigned long long)(d0 + (uint32_t)(j * NT + tid)) << 32) | wd[j]);
            }
            __syncthreads();
            found = LDSW(o64, 1);
            found_word = LDSW(o64, 0);
            __syncthreads();
            if (found != 0xFFFFFFFFu) break;
        }
        if (found == 0xFFFFFFFFu) { err = SSE_ERR_COUNT; finished = true; break; }
        uint32_t q = forward ? p + found : p + M - found;
        const bool wrapped = forward ? (q >= M) : (found > p);
        if (q >= M) q -= M;
        const Bd dq = decode_bond<CL, W, PM>(B, L, sse_op_bond(found_word)); // (the op itself at distance M: the word as thread 0 just left it)
        const uint32_t nrel = dq.a == var ? 0u : 1u;
        if (wrapped && tid == 0) { // directed_loop.rs:276-288
            const uint32_t wi = var >> 5, bi = var & 31;
            LDSW(L.o_state, wi) = (LDSW(L.o_state, wi) & ~(1u << bi)) | (newbit << bi);
        }
        const uint32_t nside = xside ^ 1u;
        if (q == p0 && nrel == rel0 && nside == side0) { finished = true; break; } // :293
        p = q; rel = nrel; side = nside; cur_word = found_word;
    }
    if (!finished) err = SSE_ERR_LOOP_OPEN;
    __syncthreads();
    return visited;
}

} // namespace sse
