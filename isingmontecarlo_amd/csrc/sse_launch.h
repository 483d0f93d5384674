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

} // namespace sse
