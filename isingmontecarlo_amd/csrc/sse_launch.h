// sse_launch.h — the host-facing interface of the kernels' translation units: the launch configuration, one launcher per kernel
// family, the sizes their carves give, the sample record's constants, and the one way a kernel with dynamic LDS is launched.
#pragma once
#include <hip/hip_runtime.h>
#include "sse_batch.h"

namespace sse {

struct LaunchCfg {
    uint32_t W, K, mode, phase, passes; // mode: SSE_MODE_*
    size_t lds_bytes;
    hipStream_t stream;
};
// Launch a kernel that carves lds_bytes of dynamic LDS: the kernel is allowed that much first (beyond 64 KB it has to be asked for)
template <typename... Params, typename... Args>
hipError_t launch_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args &...args) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
    return hipGetLastError();
}
// one translation unit per W (sweep_w*.hip) defines these
hipError_t launch_sweep_w1(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A);
hipError_t launch_sweep_w4(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A);
hipError_t launch_sweep_w6(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A);
hipError_t launch_sweep_w8(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A);
hipError_t launch_sweep_w16(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A);
hipError_t launch_sweep_fast(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A); // sweep_fast.hip: sse_fast.hip.h, W = 4
uint32_t fast_max_vars();                                                               // ... and the most variables that kernel takes (SSE_FAST_MAX_VARS)
hipError_t launch_cluster(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A);    // sweep_cluster.hip: sse_cluster.hip.h, W = 16
size_t cluster_lds_words(uint32_t N, uint32_t nwords, uint32_t Nb, uint32_t ufcap, bool has_long); // dynamic LDS words of that kernel (ClLds::carve)
bool cluster_ids_fit(uint32_t N, uint32_t S, uint32_t ufcap);                          // ... and its gate on the ids of a replica
uint32_t cluster_max_vars();                                                           // ... and on the variables of the model (SSE_CL_MAX_VARS)
// sweep_rvb.hip (sse_rvb_split.hip.h): the RVB sweep as a growth launch (16 waves) and a main launch (c.W = 4, 8 or 16 waves)
hipError_t launch_rvb_grow(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A);
hipError_t launch_rvb_main(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A);
uint32_t rvb_grow_table_start(const DevBatch &B, uint32_t ledges);         // growth launch: where its constant-op table starts (rvb_carve_grow)
uint32_t rvb_main_lds_words(uint32_t W, const DevBatch &B, uint32_t ledges); // main launch: its dynamic LDS (rvb_carve_main)
size_t rvb_split_prod_stride(uint32_t Nb);                                                // words per attempt in DevBatch::rvb_prod; 0 = the model is too large for the two-launch form
// sweep_rvb_global.hip: the RVB sweep alone with its per-variable tables in HBM (SSE_PASSES_RVB_G; c.W = 16, c.K = 4; B.rvb_tbl allocated)
hipError_t launch_rvb_global(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A);

// observe.hip (sse_observe.hip.h): the sample record's observables, record -> bit series -> autocorrelations
constexpr uint32_t OBS_TILE = 64;         // samples per workgroup of record_series_kernel: one wave's ballot
constexpr uint32_t OBS_SERIES_WAVES = 4;  // waves of that workgroup (they share the staged rows and split the groups)
constexpr uint32_t OBS_LAGS = 4;          // lags per lane and pass of bit_autocorr_kernel
constexpr uint32_t OBS_MAX_THREADS = 1024;

// LDS row stride of the staged state rows: odd, so that the 32 lanes of a half-wave, which read the same word of 32
// consecutive rows, fall on 32 different banks (nwords = 32 at N = 1024 would put them all on one)
__host__ __device__ inline uint32_t obs_row_stride(uint32_t nwords) { return nwords | 1u; }
__host__ __device__ inline size_t obs_series_lds_words(uint32_t nwords) { return (size_t)OBS_TILE * obs_row_stride(nwords); }
// LDS words of bit_autocorr_kernel's series image: the series twice back to back (2 T bits in 2 Tw words).  Lag tau reads the
// words (tau >> 5) + w and + w + 1 for w < Tw, at most word 2 Tw - 1, and of them the bits below tau + T <= 2 T - 1.
__host__ __device__ inline size_t obs_autocorr_lds_words(uint32_t T) { return 2 * (size_t)((T + 31u) / 32u); }

struct ObsGroups {
    uint32_t ngroups;
    const uint32_t *start;  // [ngroups + 1] offsets into vars
    const uint32_t *vars;   // variables of every group, < N
    const uint8_t *flip;    // [ngroups] or nullptr
};

hipError_t launch_record_series(hipStream_t stream, const uint32_t *rec, uint32_t R, uint32_t nwords, uint32_t T, const ObsGroups &G, uint32_t *out);
hipError_t launch_bit_autocorr(hipStream_t stream, const uint32_t *series, uint32_t R, uint32_t ngroups, uint32_t T, double *out);

// itime.hip (sse_itime.hip.h): imaginary-time folds of two-valued observables and bond counts, one workgroup per replica
struct ItimeArgs {
    ObsGroups G;             // ngroups == 0: bond counts only
    const uint32_t *vstart;  // [N + 1] variable -> groups, offsets into vgroups (built on the host per call)
    const uint32_t *vgroups; // [nv] the groups of every variable
    uint32_t nv;             // group variables in all = G.start[G.ngroups]
    const uint32_t *flip_bits; // [2 * ceil(ngroups / 64)] G.flip as bits (bit g & 31 of word g >> 5), or nullptr
    int64_t *sum_all, *sum_occ; // [R][ngroups]
    uint32_t *counts;        // [R][Nb] or nullptr; zeroed by the caller when hist_lds == 0 (the kernel then adds to it)
    uint32_t W;              // waves of the workgroup
    uint32_t hist_lds;       // the bond histogram is kept in LDS
    uint32_t csr_lds;        // vstart / vgroups are staged in LDS
};
// The LDS of itime_kernel in words, in this order: 64-bit event sums [2][G] | per-wave group bits [W][sw] | per-wave variable bits
// [W][nwords] | per-wave occupied counts [W] | bond histogram [Nb] | p = 0 state [nwords] | vstart [N + 1] | vgroups [nv]
struct ItimeCarve { uint32_t o_acc, o_sign, sw, o_mask, o_cnt, o_hist, o_st0, o_vstart, o_vgroups; size_t words; };
__host__ __device__ inline ItimeCarve itime_carve(uint32_t W, uint32_t N, uint32_t nwords, uint32_t Nb, uint32_t G, uint32_t nv, bool hist_lds, bool csr_lds) {
    ItimeCarve c;
    size_t o = 0;
    c.o_acc = (uint32_t)o; o += 4 * (size_t)G; // first: 8-byte aligned
    c.sw = 2u * ((G + 63u) / 64u);             // a ballot of 64 groups is two words
    c.o_sign = (uint32_t)o; o += (size_t)W * c.sw;
    c.o_mask = (uint32_t)o; o += G ? (size_t)W * nwords : 0;
    c.o_cnt = (uint32_t)o; o += W;
    c.o_hist = (uint32_t)o; o += hist_lds ? Nb : 0;
    c.o_st0 = (uint32_t)o; o += G ? nwords : 0;
    c.o_vstart = (uint32_t)o; o += csr_lds ? (size_t)N + 1 : 0;
    c.o_vgroups = (uint32_t)o; o += csr_lds ? nv : 0;
    c.words = o;
    return c;
}
// What a launch keeps in LDS of `total_words`: 16 waves with everything there, then without the histogram (global atomics), then
// without the variable -> groups lists (read through L2), then the same with 4 waves; W = 0: the sums and bit arrays alone do not fit
struct ItimePlan { uint32_t W; bool hist_lds, csr_lds; size_t words; };
inline ItimePlan itime_plan(size_t total_words, uint32_t N, uint32_t nwords, uint32_t Nb, uint32_t G, uint32_t nv, bool counts) {
    const struct { uint32_t W; bool hist, csr; } tries[4] = {{16, true, true}, {16, false, true}, {16, false, false}, {4, false, false}};
    for (const auto &t : tries) {
        const bool hist = t.hist && counts, csr = t.csr && G;
        const size_t words = itime_carve(t.W, N, nwords, Nb, G, nv, hist, csr).words;
        if (words <= total_words) return {t.W, hist, csr, words};
    }
    return {0, false, false, 0};
}
// the most groups a model of N variables can be given (4 waves, nothing optional in LDS)
inline uint32_t itime_max_groups(size_t total_words, uint32_t N, uint32_t nwords) {
    uint32_t lo = 0, hi = 1u << 24;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (itime_carve(4, N, nwords, 0, mid, 0, false, false).words <= total_words) lo = mid; else hi = mid - 1;
    }
    return lo;
}
hipError_t launch_itime(hipStream_t stream, const DevBatch &B, const ItimeArgs &A);

} // namespace sse
