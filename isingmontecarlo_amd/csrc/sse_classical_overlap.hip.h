// sse_classical_overlap.hip.h — the overlap launch of classical tempering for gfx950 (the rule: classical_overlap_rule.h).
//
// One wave per item (g, p, t), t fastest, four waves per workgroup, ceil(G P T / 4) workgroups: the items spread over every CU (one
// workgroup per chain, as the tempering launch has it, would leave most CUs idle).  A wave whose item is past the end leaves as a
// whole; there is no barrier.  Spin overlap: the lanes stride over the nwords words of both states, XOR them and count bits; the bits
// behind N are masked in the last word, and only when N is no multiple of 32.  Link overlap: the lanes stride over the E edges and read
// the two d bits from the state words.  Everything is read from global memory, one path for every N.  Lane 0 stores the two series
// values (when there is a series) and increments its own two histogram bins with a plain load, add and store: every item owns its
// histogram rows and launches are ordered by their stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "classical_launch.h"
#include "classical_overlap_rule.h"

namespace sse {

#define CMC_OV_WAVES 4u
// a slot's state words in global memory
struct CmcOvBits {
    const uint32_t *w;
    __device__ __forceinline__ bool get(uint32_t v) const { return ((w[v >> 5] >> (v & 31u)) & 1u) != 0u; }
};

__global__ __launch_bounds__(64 * CMC_OV_WAVES) void classical_overlap_kernel(CmcDev D, CmcPtDev P, CmcOvDev O, int32_t *q_row, int32_t *ql_row) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * CMC_OV_WAVES + (threadIdx.x >> 6);
    if (item >= (uint64_t)O.G * O.P * P.T) return; // the whole wave
    uint32_t grp, p, t, a, b;
    cmc_ov_item(item, O.P, P.T, grp, p, t);
    cmc_ov_pair(O.K, p, a, b);
    const uint32_t ra = cmc_ov_slot(P.slot_at, P.T, grp * O.K + a, t), rb = cmc_ov_slot(P.slot_at, P.T, grp * O.K + b, t);
    const CmcOvBits A{D.state + (size_t)ra * D.nwords}, B{D.state + (size_t)rb * D.nwords};
    const uint32_t N = D.T.N, E = D.T.E;
    uint32_t nq = 0;
    for (uint32_t j = lane; j < D.nwords; j += 64u) {
        uint32_t d = A.w[j] ^ B.w[j];
        if (j == D.nwords - 1u && (N & 31u)) d &= (1u << (N & 31u)) - 1u;
        nq += __popc(d);
    }
    uint32_t nl = cmc_ov_count_links(cmc_graph_mem(D.T, ra), A, B, lane, 64u); // the edge list is the batch's: any replica's view reads it
    for (int o = 32; o > 0; o >>= 1) { nq += __shfl_down(nq, o, 64); nl += __shfl_down(nl, o, 64); }
    if (lane == 0u) {
        if (q_row) q_row[item] = cmc_ov_overlap(N, nq);
        if (ql_row) ql_row[item] = cmc_ov_overlap(E, nl);
        uint64_t *hq = O.hq + (size_t)item * ((size_t)N + 1u) + nq, *hl = O.hl + (size_t)item * ((size_t)E + 1u) + nl;
        *hq = *hq + 1u;
        *hl = *hl + 1u;
    }
}

} // namespace sse
