// Imaginary-time folds of two-valued observables and bond counts (include/isingmc_hip.h: isingmc_itime_groups, isingmc_bond_counts):
// OpContainer::itime_fold (fast_ops.rs:1296-1315) of every group observable and OpContainer::get_count (op_container.rs:129) of every
// bond, for all replicas in one launch and in exact integers.
//
// An observable is a group of variables and a flip bit as in sse_observe.hip.h; x_g(p) is its value on the propagated state BEFORE slot
// p's op.  It only changes at off-diagonal ops, so nothing is evaluated per slot: the identity of sse_itime.h turns the fold into one
// term per EVENT (an off-diagonal op's flipped variable, for every group that holds the variable).
//
// One workgroup per replica; wave w owns the 64-slot rows [w * per, (w + 1) * per).  Rows are loaded whole (the op-string rows are padded
// and hold 0 beyond the cutoff; lanes beyond the cutoff are masked all the same).
//   A  every wave xors the variables its ops flip into its own N-bit array and counts its occupied slots; bonds are counted into the
//      histogram on the way.  An exclusive prefix over the waves, from the p = 0 state, turns the arrays into the state at the start of
//      every wave's range, and the counts into the occupied slots in front of it.
//   B  every wave evaluates the groups on its start state (one bit per group: the flip bits, toggled through the list of every set
//      variable), then walks its rows again: the off-diagonal lanes look up the lists of the variables they flip, a ballot of them gives
//      the events, taken in slot order; per flipped variable the lanes run over the variable's groups (variable -> groups lists built
//      on the host), toggle the group's bit and add delta * weight into the group's two 64-bit sums in LDS.
// A variable that a group lists twice appears twice in its list: the two toggles of one instruction are serialised by the LDS atomic
// and their terms cancel, as the parity does.  No scratch, no global atomics but for a histogram that LDS does not hold.
#pragma once
#include "../../include/sse_format.h"
#include "sse_itime.h"
#include "sse_launch.h" // ItimeArgs, ItimeCarve

namespace sse {

// the bit of group g on the state words `st`
__device__ inline uint32_t itime_group_bit(const ObsGroups &G, const uint32_t *st, uint32_t g) {
    uint32_t par = G.flip ? (uint32_t)G.flip[g] : 0u;
    for (uint32_t k = G.start[g], e = G.start[g + 1]; k < e; ++k) {
        const uint32_t v = G.vars[k];
        par ^= st[v >> 5] >> (v & 31u);
    }
    return par & 1u;
}

// grid R, A.W * 64 threads, dynamic LDS itime_carve(...).words words.  CSR_LDS = A.csr_lds: the variable -> groups lists are staged in LDS
// (a template parameter so that their loads are LDS loads and not flat ones)
template <bool CSR_LDS>
__global__ void __launch_bounds__(1024)
itime_kernel(DevBatch B, ItimeArgs A) {
    extern __shared__ uint32_t it_lds[];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), W = nthr >> 6;
    const uint32_t G = A.G.ngroups, N = B.N, nwords = B.nwords, Nb = B.Nb;
    const ItimeCarve C = itime_carve(W, N, nwords, Nb, G, A.nv, A.hist_lds != 0u, CSR_LDS);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(it_lds + C.o_acc); // [0, G): all slots, [G, 2 G): occupied slots
    uint32_t *sign = it_lds + C.o_sign + wave * C.sw;
    uint32_t *masks = it_lds + C.o_mask, *mask = masks + wave * nwords;
    uint32_t *cnt = it_lds + C.o_cnt, *hist = it_lds + C.o_hist, *st0 = it_lds + C.o_st0;
    const uint32_t M = B.cutoff[r];
    const uint32_t *ops = B.ops + (size_t)r * B.stride;
    const uint32_t rows = (M + 63u) >> 6, per = (rows + W - 1u) / W;
    const uint32_t row0 = min(wave * per, rows), row1 = min(row0 + per, rows);
    uint32_t *counts = A.counts ? A.counts + (size_t)r * Nb : nullptr;

    for (uint32_t i = tid; i < C.o_st0; i += nthr) it_lds[i] = 0u;
    if (G) {
        for (uint32_t j = tid; j < nwords; j += nthr) st0[j] = B.state[(size_t)r * nwords + j];
        if (CSR_LDS) {
            for (uint32_t i = tid; i <= N; i += nthr) it_lds[C.o_vstart + i] = A.vstart[i];
            for (uint32_t i = tid; i < A.nv; i += nthr) it_lds[C.o_vgroups + i] = A.vgroups[i];
        }
    }
    __syncthreads();

    // A: flipped variables and occupied slots of the wave's range; the bond histogram
    uint32_t occ = 0;
    for (uint32_t row = row0; row < row1; ++row) {
        const uint32_t p = row * 64u + lane;
        uint32_t w = ops[p];
        if (p >= M) w = 0u;
        occ += (uint32_t)__popcll(__ballot(w != 0u));
        if (!w) continue;
        const uint32_t bond = sse_op_bond(w);
        if (bond >= Nb) continue; // (isingmc_verify reports such a string; nothing is written outside the tables here)
        if (counts) {
            if (A.hist_lds) atomicAdd(&hist[bond], 1u);
            else atomicAdd(&counts[bond], 1u);
        }
        const uint32_t f = sse_itime_flips(w);
        if (G && f) {
            const BondRec rec = B.bonds[bond]; // a bond's variables are the same in every Hamiltonian row
            const uint32_t a = rec.a_info & SSE_VAR_MASK, c = rec.c;
            if ((f & 1u) && a < N) atomicXor(&mask[a >> 5], 1u << (a & 31u));
            if ((f & 2u) && c < N) atomicXor(&mask[c >> 5], 1u << (c & 31u));
        }
    }
    if (lane == 0u) cnt[wave] = occ;
    __syncthreads();
    if (counts && A.hist_lds)
        for (uint32_t i = tid; i < Nb; i += nthr) counts[i] = hist[i];
    if (!G) return; // (uniform)

    // the state at the start of every wave's range, the occupied slots in front of it and in all
    uint32_t occ_run = 0, n = 0;
    for (uint32_t u = 0; u < W; ++u) {
        const uint32_t c = cnt[u];
        if (u < wave) occ_run += c;
        n += c;
    }
    for (uint32_t j = tid; j < nwords; j += nthr) {
        uint32_t s = st0[j];
        for (uint32_t u = 0; u < W; ++u) {
            const uint32_t t = masks[u * nwords + j];
            masks[u * nwords + j] = s;
            s ^= t;
        }
    }
    __syncthreads();

    // B: the groups on the wave's start state (their flip bits, toggled once per set variable through the variable's list), then its
    // events in slot order
    const uint32_t *vstart = CSR_LDS ? it_lds + C.o_vstart : A.vstart;
    const uint32_t *vgroups = CSR_LDS ? it_lds + C.o_vgroups : A.vgroups;
    if (row0 < row1) {
        for (uint32_t i = lane; i < C.sw; i += 64u) sign[i] = A.flip_bits ? A.flip_bits[i] : 0u;
        __builtin_amdgcn_wave_barrier(); // (one wave's LDS accesses complete in order; this keeps the compiler from moving them)
        for (uint32_t v = lane; v < N; v += 64u) {
            if (!((mask[v >> 5] >> (v & 31u)) & 1u)) continue;
            for (uint32_t k = vstart[v], e = vstart[v + 1u]; k < e; ++k) {
                const uint32_t g = vgroups[k];
                atomicXor(&sign[g >> 5], 1u << (g & 31u));
            }
        }
    }
    __syncthreads();
    for (uint32_t row = row0; row < row1; ++row) {
        const uint32_t p = row * 64u + lane;
        uint32_t w = ops[p];
        if (p >= M) w = 0u;
        const uint32_t f = sse_itime_flips(w);
        uint32_t kb[2] = {0u, 0u}, ke[2] = {0u, 0u}; // the lists of the variables this lane's op flips (empty: not flipped)
        if (f) {
            const uint32_t bond = sse_op_bond(w);
            if (bond < Nb) {
                const BondRec rec = B.bonds[bond];
                const uint32_t va = rec.a_info & SSE_VAR_MASK, vc = rec.c;
                if ((f & 1u) && va < N) { kb[0] = vstart[va]; ke[0] = vstart[va + 1u]; }
                if ((f & 2u) && vc < N) { kb[1] = vstart[vc]; ke[1] = vstart[vc + 1u]; }
            }
        }
        const unsigned long long occb = __ballot(w != 0u);
        unsigned long long evb = __ballot(f != 0u);
        while (evb) {
            const uint32_t l = (uint32_t)__builtin_ctzll(evb);
            evb &= evb - 1ull;
            const uint32_t upto = occ_run + (uint32_t)__popcll(occb & ((2ull << l) - 1ull)); // occupied slots up to and including the event's
            const long long w_all = sse_itime_behind(M, row * 64u + l), w_occ = sse_itime_occupied_behind(n, upto);
#pragma unroll
            for (uint32_t leg = 0; leg < 2u; ++leg) {
                const uint32_t b = __builtin_amdgcn_readlane(kb[leg], l), e = __builtin_amdgcn_readlane(ke[leg], l);
                for (uint32_t k = b + lane; k < e; k += 64u) {
                    const uint32_t g = vgroups[k];
                    const uint32_t before = atomicXor(&sign[g >> 5], 1u << (g & 31u)) >> (g & 31u);
                    const long long d = sse_itime_delta(before);
                    atomicAdd(&acc[g], (unsigned long long)(d * w_all));
                    atomicAdd(&acc[G + g], (unsigned long long)(d * w_occ));
                }
            }
        }
        occ_run += (uint32_t)__popcll(occb);
    }
    __syncthreads();
    for (uint32_t g = tid; g < G; g += nthr) {
        const uint32_t bit0 = itime_group_bit(A.G, st0, g);
        if (A.sum_all) A.sum_all[(size_t)r * G + g] = sse_itime_total(M, bit0, (long long)acc[g]);
        if (A.sum_occ) A.sum_occ[(size_t)r * G + g] = sse_itime_total(n, bit0, (long long)acc[G + g]);
    }
}

} // namespace sse
