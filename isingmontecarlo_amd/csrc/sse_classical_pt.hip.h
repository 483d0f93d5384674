// sse_classical_pt.hip.h — the tempering launch of classical Monte Carlo for gfx950 (the rule: classical_pt_rule.h).
//
// One workgroup per chain, of min(T, 16) waves.  Its waves stride over the chain's T slots: a wave computes the energy and the magnetisation of a slot
// from the state words in global memory, in the order the rule states (64 lane folds, then the tree), and stores them by slot; with a
// series it also stores them by the temperature the slot holds, which no one has changed yet.  After a workgroup barrier the chain's
// two phases are decided: the pairs of a phase are disjoint, so the threads take them side by side (thread j the j-th pair of the
// phase, striding by the workgroup), with a barrier between the phases.  Last, the threads write the beta of every slot for the next
// steps launch.  Everything the launch works on lives in global memory, so T is bounded by nothing but R.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "classical_launch.h"
#include "classical_pt_rule.h"
#include "sse_core.hip.h" // philox4x32_10

namespace sse {

struct CmcPtKernelDraw {
    __device__ uint32_t operator()(const PtChain &c, uint32_t index) const { return philox4x32_10(index, c.step_lo, c.chain, c.tag_step_hi, c.key0, c.key1).x; }
};
// a slot's state bits in global memory
struct CmcBitsMem {
    const uint32_t *w;
    __device__ __forceinline__ bool get(uint32_t v) const { return ((w[v >> 5] >> (v & 31u)) & 1u) != 0u; }
};

__global__ __launch_bounds__(64 * CMC_PT_MAX_WAVES) void classical_tempering_kernel(CmcDev D, CmcPtDev P, uint64_t pt_step, double *energy_row, int32_t *mag_row) {
    __shared__ uint32_t s_err;
    const uint32_t c = blockIdx.x, T = P.T, base = c * T;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    if (threadIdx.x == 0u) s_err = 0u;
    __syncthreads();
    for (uint32_t i = wave; i < T; i += nwaves) { // the wave's slots
        const uint32_t r = base + i;
        const CmcGraphMem g = cmc_graph_mem(D.T, r); // the slot's own couplings (equal along a chain when they are per replica)
        const CmcBitsMem s{D.state + (size_t)r * D.nwords};
        double e = cmc_pt_lane_energy(g, s, lane);
        for (int o = 32; o > 0; o >>= 1) e += __shfl_down(e, o, 64);
        int up = 0;
        for (uint32_t j = lane; j < D.nwords; j += 64u) {
            uint32_t w = s.w[j];
            if (j == D.nwords - 1u && (D.T.N & 31u)) w &= (1u << (D.T.N & 31u)) - 1u;
            up += __popc(w);
        }
        for (int o = 32; o > 0; o >>= 1) up += __shfl_down(up, o, 64);
        if (lane == 0u) {
            const int32_t m = 2 * up - (int32_t)D.T.N;
            const uint32_t t = P.temp_of[r];
            P.energy[r] = e; P.mag[r] = m;
            if (energy_row) energy_row[base + t] = e;
            if (mag_row) mag_row[base + t] = m;
            if (D.err[r] != 0u) atomicOr(&s_err, 1u);
        }
    }
    __syncthreads();
    if (s_err == 0u) { // a chain with a flagged slot makes no swaps
        const CmcPtChainView cv{T, P.betas, P.temp_of + base, P.slot_at + base, P.energy + base, P.attempts + (size_t)c * (T - 1u), P.accepts + (size_t)c * (T - 1u)};
        const PtChain pc = pt_chain((uint64_t)D.seed_lo | ((uint64_t)D.seed_hi << 32), pt_step, D.replica_offset / T + c);
        const CmcPtKernelDraw draw;
        const bool a_first = pt_a_first(pc, draw);
        for (int phase = 0; phase < 2; ++phase) {
            const uint32_t first = pt_in_phase(a_first, phase, 0u) ? 0u : 1u;
            for (uint32_t t = first + 2u * threadIdx.x; t + 1u < T; t += 2u * blockDim.x) cmc_pt_attempt(cv, t, pt_uniform(draw(pc, pt_index_pair(t))));
            __syncthreads(); // (uniform: s_err is one value for the workgroup)
        }
    }
    for (uint32_t i = threadIdx.x; i < T; i += blockDim.x) P.beta_slot[base + i] = P.betas[P.temp_of[base + i]];
}

} // namespace sse
