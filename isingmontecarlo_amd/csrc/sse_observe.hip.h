// Observables of the sample record (include/isingmc_hip.h, isingmc_record_*): two-valued time series and their exact
// circular autocorrelations.
//
// The record is [capacity][R][nwords] words in the layout of DevBatch::state.  An observable is a group of variables and a
// flip bit: its bit at sample t is parity(state bits of the group's variables) ^ flip, bit 1 standing for the value +1
// (a variable, autocorrelations.rs:37-50; a product of spins, :52-75; a bond, qmc_ising.rs:988-997).
//
//   record_series_kernel   record -> time-major bit series [R][ngroups][Tw], Tw = (T + 31) / 32, bit t & 31 of word t >> 5
//   bit_autocorr_kernel    series -> [R][T] doubles: for a +-1 series x with s = sum_t x[t] = 2 ones - T and
//                          C(tau) = sum_t x[t] x[(t + tau) mod T] = T - 2 popcount(bits ^ rot(bits, tau)),
//                          the mean over the observables of (T C(tau) - s^2) / (T^2 - s^2)  (0 when T^2 == s^2),
//                          which is the reference's centred, unit-norm autocorrelation (autocorrelations.rs:99-133)
//                          with every step up to the one division in integers.
#pragma once
#include "sse_launch.h" // ObsGroups, the OBS_* constants, the LDS sizes and the launch prototypes

namespace sse {

// grid (tiles of 64 samples, R), OBS_SERIES_WAVES * 64 threads, dynamic LDS obs_series_lds_words(nwords) words.
// rec points at row `first` of the record; row t of replica r starts at rec + (t * R + r) * nwords.
__global__ void __launch_bounds__(OBS_SERIES_WAVES * 64)
record_series_kernel(const uint32_t *__restrict__ rec, uint32_t R, uint32_t nwords, uint32_t T, ObsGroups G, uint32_t *__restrict__ out) {
    extern __shared__ uint32_t obs_lds[];
    const uint32_t tile = blockIdx.x, r = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t stride = obs_row_stride(nwords);
    const uint32_t t0 = tile * OBS_TILE;
    const uint32_t rows = T - t0 < OBS_TILE ? T - t0 : OBS_TILE;
    // stage the tile: a wave takes a row at a time, its lanes consecutive words of it (one row = nwords * 4 contiguous bytes)
    for (uint32_t i = wave; i < rows; i += OBS_SERIES_WAVES) {
        const uint32_t *src = rec + ((size_t)(t0 + i) * R + r) * nwords;
        for (uint32_t j = lane; j < nwords; j += 64u) obs_lds[i * stride + j] = src[j];
    }
    __syncthreads();
    const uint32_t Tw = (T + 31u) / 32u;
    const bool live = lane < rows;
    const uint32_t *row = obs_lds + (live ? lane : 0u) * stride; // (idle lanes read row 0: staged, ignored by the ballot)
    for (uint32_t g = wave; g < G.ngroups; g += OBS_SERIES_WAVES) {
        const uint32_t b = G.start[g], e = G.start[g + 1];
        uint32_t par = G.flip ? (uint32_t)(G.flip[g] & 1u) : 0u;
        for (uint32_t k = b; k < e; ++k) {
            const uint32_t v = G.vars[k];
            par ^= row[v >> 5] >> (v & 31u);
        }
        const unsigned long long bits = __ballot(live && (par & 1u));
        if (lane == 0) {
            uint32_t *dst = out + ((size_t)r * G.ngroups + g) * Tw + 2u * tile;
            dst[0] = (uint32_t)bits;
            if (2u * tile + 1u < Tw) dst[1] = (uint32_t)(bits >> 32);
        }
    }
}

// 32 bits of the series x (Tw words, bits >= T zero) from bit p on, zero beyond the series
__device__ inline uint32_t obs_bits_at(const uint32_t *__restrict__ x, uint32_t Tw, uint32_t p) {
    const uint32_t i = p >> 5;
    const uint32_t lo = i < Tw ? x[i] : 0u, hi = i + 1u < Tw ? x[i + 1u] : 0u;
    return __funnelshift_r(lo, hi, p & 31u);
}

// grid R, ceil(T / OBS_LAGS) threads rounded up to whole waves and at most OBS_MAX_THREADS, dynamic LDS obs_autocorr_lds_words(T) + 2 words.
// Lanes take lags, OBS_LAGS of them blockDim apart per pass; the groups are walked in ascending order and every lag's terms are
// added in that order into one double in a register: the result does not depend on the launch geometry.
__global__ void __launch_bounds__(OBS_MAX_THREADS)
bit_autocorr_kernel(const uint32_t *__restrict__ series, uint32_t ngroups, uint32_t T, double *__restrict__ out) {
    extern __shared__ uint32_t obs_lds[];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const uint32_t Tw = (T + 31u) / 32u;
    const uint32_t nw2 = 2u * Tw;
    uint32_t *ones = obs_lds + nw2; // [2]: the series' population count, the two words in turn from one staged series to the next
    uint32_t turn = 0;
    if (tid < 2u) ones[tid] = 0u;
    const uint32_t sh = T & 31u;
    const uint32_t last_mask = sh ? (1u << sh) - 1u : 0xFFFFFFFFu;
    const int64_t T64 = (int64_t)T;
    for (uint32_t lag0 = 0; lag0 < T; lag0 += nthr * OBS_LAGS) {
        uint32_t tau[OBS_LAGS];
        double acc[OBS_LAGS];
#pragma unroll
        for (uint32_t k = 0; k < OBS_LAGS; ++k) {
            const uint32_t t = lag0 + k * nthr + tid;
            tau[k] = t < T ? t : 0u; // (lags beyond the series compute lag 0 and drop it)
            acc[k] = 0.0;
        }
        for (uint32_t g = 0; g < ngroups; ++g) {
            const uint32_t *x = series + ((size_t)r * ngroups + g) * Tw;
            __syncthreads(); // the lags of the group before are done with the LDS image and its count
            // the series twice back to back: word j holds x's bits from 32 j on, and the second copy's from 32 j - T on
            uint32_t cnt = 0;
            for (uint32_t j = tid; j < nw2; j += nthr) {
                uint32_t w = 0;
                if (j < Tw) { w = x[j]; cnt += __popc(w); }
                const uint32_t lo = 32u * j;
                if (lo >= T) w |= obs_bits_at(x, Tw, lo - T);
                else if (lo + 32u > T) w |= x[0] << (T - lo);
                obs_lds[j] = w;
            }
            for (uint32_t o = 32u; o; o >>= 1) cnt += __shfl_xor(cnt, o);
            if ((tid & 63u) == 0u && cnt) atomicAdd(&ones[turn], cnt);
            if (tid == 0u) ones[turn ^ 1u] = 0u; // (nobody reads or adds to it between the two barriers)
            __syncthreads();
            uint32_t ham[OBS_LAGS], lo[OBS_LAGS];
#pragma unroll
            for (uint32_t k = 0; k < OBS_LAGS; ++k) { ham[k] = 0u; lo[k] = obs_lds[tau[k] >> 5]; }
            auto step = [&](uint32_t w, uint32_t m) {
                const uint32_t xw = obs_lds[w]; // the same word for every lane: a broadcast
#pragma unroll
                for (uint32_t k = 0; k < OBS_LAGS; ++k) {
                    const uint32_t hi = obs_lds[(tau[k] >> 5) + w + 1u];
                    ham[k] += __popc((xw ^ __funnelshift_r(lo[k], hi, tau[k] & 31u)) & m);
                    lo[k] = hi;
                }
            };
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
            for (uint32_t w = 0; w + 1u < Tw; ++w) step(w, 0xFFFFFFFFu);
            step(Tw - 1u, last_mask);
            const int64_t s = 2 * (int64_t)ones[turn] - T64;
            turn ^= 1u;
            const int64_t den = T64 * T64 - s * s;
#pragma unroll
            for (uint32_t k = 0; k < OBS_LAGS; ++k) {
                const int64_t c = T64 - 2 * (int64_t)ham[k];
                const int64_t num = T64 * c - s * s;
                acc[k] += den ? (double)num / (double)den : 0.0;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < OBS_LAGS; ++k) {
            const uint32_t t = lag0 + k * nthr + tid;
            if (t < T) out[(size_t)r * T + t] = acc[k] / (double)ngroups;
        }
    }
}

} // namespace sse
