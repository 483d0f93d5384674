// sse_sweep.hip.h — sse::sweep_kernel, the general kernel that runs whole timesteps or a group of their passes, and the dispatch
// from a LaunchCfg to its instantiations (sweep_w*.hip and sweep_rvb_global.hip instantiate them).
#pragma once
#include "sse_cluster_pass.hip.h"
#include "sse_diag.hip.h"
#include "sse_launch.h"
#include "sse_loop.hip.h"
#include "sse_rvb.hip.h"

namespace sse {

// One launch = nsteps timesteps of every replica.  Reference drivers: QmcIsingGraph::timestep
// (qmc_ising.rs:644-795), Qmc::timestep (qmc_runner.rs:363-377), measurement loop
// QmcStepper::timesteps_measure_with_self (qmc_traits/qmc_stepper.rs:133-162).
// PHASE only tags the symbol (0 = measured path, 1 = data preparation) so that profilers can tell the
// two apart; the code is identical.
// PASSES selects what is compiled in: SSE_PASSES_ALL = every pass (one launch runs whole timesteps), SSE_PASSES_DIAG =
// the diagonal pass alone.  The diagonal pass needs half the registers and a quarter of the LDS of the cluster
// pass, so as its own kernel it runs at twice the occupancy (4 waves per SIMD for W <= 4); the host then issues
// two launches per timestep (driver.hip, run()).  n, cutoff, epoch, chunk counters travel through HBM.
// SSE_PASSES_OFFDIAG is the second of those launches with the diagonal and RVB code left out (fewer live scalars).
#ifndef SSE_MIN_WAVES_PER_SIMD
#define SSE_MIN_WAVES_PER_SIMD 1
#endif

template <int W, int PASSES>
constexpr int sse_waves_per_simd() {
    if (PASSES == SSE_PASSES_DIAG) return W <= 4 ? 4 : (W <= 8 ? 2 : 1);
    return W == 8 ? SSE_MIN_WAVES_PER_SIMD : (W == 6 ? 3 : (W == 4 ? 2 : 1));
}
template <int W, int K, int MODE, int PHASE, int PASSES>
__global__ __launch_bounds__(W * 64, (sse_waves_per_simd<W, PASSES>())) void sweep_kernel(DevBatch B, SweepArgs A) {
    constexpr int NT = W * 64;
    constexpr bool CL = MODE == SSE_MODE_LDS_EDGES, TG = MODE == SSE_MODE_GLOBAL_TABLES || MODE == SSE_MODE_PM_GLOBAL_TABLES;
    constexpr bool PM = MODE == SSE_MODE_PM_LDS_TABLES || MODE == SSE_MODE_PM_GLOBAL_TABLES;
    constexpr bool RG = PASSES == SSE_PASSES_RVB_G, RVB_ONLY = PASSES == SSE_PASSES_RVB || RG;
    static_assert(MODE != SSE_MODE_PM_LDS_TABLES || PASSES == SSE_PASSES_DIAG, "mode 3 is the diagonal launch of large +-J models");
    static_assert(!RG || (!TG && !PM), "RVB_G decodes bonds through the LDS edge table or the general records");
    Lds<W> L;
    L.carve(B.N, B.nwords, B.lds_ufcap, CL ? B.E : 0u, B.has_long, TG || RG, PM ? B.pm_words : 0u, MODE == SSE_MODE_PM_LDS_TABLES);
    const int tid = threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (A.only_flagged && !B.aux[r]) return; // (uniform per workgroup; the flag is cleared at the end, behind the barriers below)
    if (B.bond_stride) { // per-replica couplings: this replica's tables (B is this workgroup's private copy)
        const uint32_t hr = B.ham_row ? B.ham_row[r] : r;
        B.bonds += (size_t)hr * B.bond_stride;
        B.cumw += (size_t)hr * B.bond_stride;
        B.wtot = B.wtot_r[hr];
        if constexpr (PM) for (uint32_t i = tid; i < B.pm_words; i += NT) LDSW(L.o_signs, i) = B.pm_signs[(size_t)hr * B.pm_words + i];
    }
    for (uint32_t i = tid; i < B.nwords; i += NT) LDSW(L.o_state, i) = B.state[(size_t)r * B.nwords + i];
    if constexpr (CL)
        for (uint32_t i = tid; i < B.E; i += NT) LDSW(L.o_edges, i) = B.edges_compact[i];
    for (uint32_t i = tid; i < 2 * SSE_MAX_CHUNKS; i += NT) LDSW(L.o_chn, i) = B.chunks[(size_t)r * 2 * SSE_MAX_CHUNKS + i];
    __syncthreads();
    int n = (int)B.n[r], ntrans = (int)B.ntrans[r];
    uint32_t M = B.cutoff[r], err = B.err[r], gr = 0, last_out = 0;
    uint64_t epoch = B.epoch[r];
    const double beta = A.beta ? A.beta[r] : 0.0;
    uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0;
    for (uint64_t step = 0; step < A.nsteps; ++step) {
        if (err) break;
        if constexpr (PASSES != SSE_PASSES_OFFDIAG && !RVB_ONLY)
        if (A.domask & SSE_DO_DIAG) {
            const Rng rng = make_rng(B, r, epoch);
            if (A.domask & SSE_DO_HEATBATH) diagonal_pass<W, K, CL, true, TG, PM>(B, L, r, rng, beta, M, n, ntrans, gr);
            else diagonal_pass<W, K, CL, false, TG, PM>(B, L, r, rng, beta, M, n, ntrans, gr);
            epoch++;
            a5 += M;
            if (A.domask & SSE_DO_GROW) { // qmc_ising.rs:786, qmc_runner.rs:197
                const uint32_t want = (uint32_t)n + (uint32_t)n / 2u;
                if (want > M) { if (want > B.cap) { err = SSE_ERR_CAPACITY; break; } M = want; }
            }
        }
        if constexpr (((PASSES == SSE_PASSES_ALL || PASSES == SSE_PASSES_RVB) && !TG && !PM) || RG) // (RVB keeps its working set in LDS except under RVB_G: refused by the host for MODE 2 models without it)
        if (A.domask & SSE_DO_RVB) { // qmc_ising.rs:705-752
            const uint32_t updates = A.rvb_updates ? A.rvb_updates : (B.N + 1u) / 2u;
            last_out = rvb_pass<W, CL, RG>(B, L, r, epoch, M, updates, gr, err);
            epoch++;
            a4 += updates;
            if (err) break;
        }
        // the directed loop is one sequential walk: it runs in the small geometry of the diagonal launch
        if constexpr (PASSES != SSE_PASSES_OFFDIAG && !RVB_ONLY)
        if (A.domask & SSE_DO_LOOP) {
            const Rng rng = make_rng(B, r, epoch);
            last_out = loop_pass<W, CL, PM>(B, L, r, rng, M, n, gr, err);
            epoch++;
            a4 += last_out;
            if (err) break;
        }
        if constexpr (PASSES != SSE_PASSES_DIAG && !RVB_ONLY) {
        if (A.domask & SSE_DO_CLUSTER) {
            const Rng rng = make_rng(B, r, epoch);
            const uint32_t S_ids = (uint32_t)W * B.N + (uint32_t)ntrans;
            if constexpr (TG) last_out = cluster_pass<W, K, CL, true, true, PM>(B, L, r, rng, A.prob, M, n, ntrans, gr, err);
            else if (S_ids <= B.lds_ufcap && S_ids <= 65535u) last_out = cluster_pass<W, K, CL, false, false>(B, L, r, rng, A.prob, M, n, ntrans, gr, err);
            else last_out = cluster_pass<W, K, CL, true, false>(B, L, r, rng, A.prob, M, n, ntrans, gr, err);
            epoch++;
            a4 += (uint64_t)n;
            if (err) break;
        }
        if (A.domask & SSE_DO_FREE) {
            const Rng rng = make_rng(B, r, epoch);
            if (!(A.domask & SSE_DO_CLUSTER)) touch_scan<W, CL, PM>(B, L, r, M);
            free_spin_pass<W>(B, L, rng);
            epoch++;
        }
        if (A.sampling_freq && (A.step0 + step + 1) % A.sampling_freq == 0) {
            if (tid == 0) LDSW(L.o_misc, MISC_LOOP_A) = 0u;
            __syncthreads();
            uint32_t up = 0;
            for (uint32_t i = tid; i < B.nwords; i += NT) up += __popc(LDSW(L.o_state, i));
            for (int off = 32; off > 0; off >>= 1) up += __shfl_down(up, off);
            if ((tid & 63) == 0 && up) atomicAdd(&LDSW(L.o_misc, MISC_LOOP_A), up);
            __syncthreads();
            const long long mag = 2ll * (long long)LDSW(L.o_misc, MISC_LOOP_A) - (long long)B.N;
            a0 += (uint64_t)n; a1 += 1; a2 += (uint64_t)(mag < 0 ? -mag : mag); a3 += (uint64_t)(mag * mag); a6 += (uint64_t)ntrans;
            __syncthreads();
        }
        } // PASSES != SSE_PASSES_DIAG
    }
    __syncthreads();
    // (the directed loop of the diagonal launch can flip p=0 spins too)
        for (uint32_t i = tid; i < B.nwords; i += NT) B.state[(size_t)r * B.nwords + i] = LDSW(L.o_state, i);
    for (uint32_t i = tid; i < 2 * SSE_MAX_CHUNKS; i += NT) B.chunks[(size_t)r * 2 * SSE_MAX_CHUNKS + i] = LDSW(L.o_chn, i);
    if (tid == 0) {
        B.n[r] = (uint32_t)n; B.ntrans[r] = (uint32_t)ntrans; B.cutoff[r] = M; B.err[r] = err; B.epoch[r] = epoch;
        if (A.out_u32) A.out_u32[r] = last_out;
        uint64_t *acc = B.acc + (size_t)B.acc_row[r] * 8;
        acc[0] += a0; acc[1] += a1; acc[2] += a2; acc[3] += a3; acc[4] += a4; acc[5] += a5; acc[6] += a6;
        if (A.only_flagged) B.aux[r] = 0u;
    }
}

template <int W, int K, int MODE, int PHASE, int PASSES>
hipError_t launch_one(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    return launch_lds(sweep_kernel<W, K, MODE, PHASE, PASSES>, dim3(B.R), dim3(W * 64), c.lds_bytes, c.stream, B, A);
}
// PHASE = 1, the data-preparation symbol, exists in the default geometry K = 4 only: any other K runs PHASE = 0 whatever c.phase says
template <int W, int K, int MODE, int PASSES>
hipError_t launch_phase(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    if constexpr (K == 4) if (c.phase) return launch_one<W, K, MODE, 1, PASSES>(c, B, A);
    return launch_one<W, K, MODE, 0, PASSES>(c, B, A);
}
template <int W, int K, int MODE>
hipError_t launch_k(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    switch (c.passes) {
    case SSE_PASSES_DIAG: return launch_phase<W, K, MODE, SSE_PASSES_DIAG>(c, B, A);
    case SSE_PASSES_OFFDIAG: return launch_phase<W, K, MODE, SSE_PASSES_OFFDIAG>(c, B, A);
    case SSE_PASSES_RVB:
        if constexpr (MODE != SSE_MODE_GLOBAL_TABLES && MODE != SSE_MODE_PM_GLOBAL_TABLES) return launch_one<W, K, MODE, 0, SSE_PASSES_RVB>(c, B, A);
        else return hipErrorInvalidValue;
    default: return launch_phase<W, K, MODE, SSE_PASSES_ALL>(c, B, A);
    }
}
// The instantiations of sweep_kernel<W, K, MODE, PHASE, PASSES> that exist; launch_w refuses every other LaunchCfg with hipErrorInvalidValue:
//   W       1, 4, 6, 8, 16: one translation unit each (sweep_w*.hip)
//   K, MODE GENERAL and LDS_EDGES with K = 4, 2, 1; GLOBAL_TABLES with K = 4, 1; the two +-J decodes with W = 4, K = 4 alone
//   PASSES  ALL, DIAG and OFFDIAG for each of those; RVB too where the tables live in LDS (GENERAL, LDS_EDGES); PM_LDS_TABLES is DIAG alone
//   PHASE   0; and 1 next to it where K = 4 and PASSES is not RVB
// (sweep_rvb_global.hip adds <16, 4, GENERAL or LDS_EDGES, 0, RVB_G>.)
template <int W>
hipError_t launch_w(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    if (c.mode == SSE_MODE_PM_LDS_TABLES || c.mode == SSE_MODE_PM_GLOBAL_TABLES) { // +-J decode: the default geometry of large models only
        if constexpr (W == 4) {
            if (c.K != 4) return hipErrorInvalidValue;
            if (c.mode == SSE_MODE_PM_LDS_TABLES) {
                if (c.passes != SSE_PASSES_DIAG) return hipErrorInvalidValue;
                return launch_phase<4, 4, SSE_MODE_PM_LDS_TABLES, SSE_PASSES_DIAG>(c, B, A);
            }
            return launch_k<4, 4, SSE_MODE_PM_GLOBAL_TABLES>(c, B, A);
        } else return hipErrorInvalidValue;
    }
    if (c.mode == SSE_MODE_GLOBAL_TABLES) { // tables in HBM: slots_per_lane 4 and 1 only
        if (c.K == 4) return launch_k<W, 4, SSE_MODE_GLOBAL_TABLES>(c, B, A);
        if (c.K == 1) return launch_k<W, 1, SSE_MODE_GLOBAL_TABLES>(c, B, A);
        return hipErrorInvalidValue;
    }
    const bool cl = c.mode == SSE_MODE_LDS_EDGES;
    if (c.K == 4 && cl) return launch_k<W, 4, SSE_MODE_LDS_EDGES>(c, B, A);
    if (c.K == 4 && !cl) return launch_k<W, 4, SSE_MODE_GENERAL>(c, B, A);
    if (c.K == 1 && cl) return launch_k<W, 1, SSE_MODE_LDS_EDGES>(c, B, A);
    if (c.K == 1 && !cl) return launch_k<W, 1, SSE_MODE_GENERAL>(c, B, A);
    if (c.K == 2 && cl) return launch_k<W, 2, SSE_MODE_LDS_EDGES>(c, B, A);
    if (c.K == 2 && !cl) return launch_k<W, 2, SSE_MODE_GENERAL>(c, B, A);
    return hipErrorInvalidValue;
}

} // namespace sse
