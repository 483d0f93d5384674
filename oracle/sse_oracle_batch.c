/*
 * sse_oracle_batch.c — CPU ORACLE batch runner (test infrastructure, NOT product).
 * Runs independent replicas on host threads, one replica per thread at a time, the way the reference
 * fans graphs out over rayon threads (src/sse/parallel_tempering/tempering_container.rs:367-371,
 * :428-434).  Used by tests for convenience and by bench.py's cpu_baseline leg.
 */
#include "sse_oracle_internal.h"
#include <stddef.h>
#include <stdlib.h>
#ifdef _OPENMP
#include <omp.h>
#endif

int ora_batch_timesteps(ora_replica **reps, uint32_t nreplicas, uint64_t t, const double *betas,
                        uint32_t sampling_freq, uint32_t flags, int nthreads) {
    int rc = 0;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#else
    (void)nthreads;
#endif
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (int64_t i = 0; i < (int64_t)nreplicas; ++i)
        rc |= ora_timesteps(reps[i], t, betas[i], sampling_freq, flags);
    return rc;
}

int ora_max_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* Batch accessors for tests that drive thousands of replicas from Python: one call instead of one per replica.
 * Any of n, cutoff, acc ([nreplicas][8]) may be NULL. */
void ora_batch_get(ora_replica *const *reps, uint32_t nreplicas, uint32_t *n, uint32_t *cutoff, uint64_t *acc) {
    for (uint32_t i = 0; i < nreplicas; ++i) {
        if (n) n[i] = ora_get_n(reps[i]);
        if (cutoff) cutoff[i] = ora_get_cutoff(reps[i]);
        if (acc) ora_get_accumulators(reps[i], acc + 8 * (size_t)i);
    }
}

/* ora_get_bond_count for bonds 0 .. nbonds - 1 of every replica in one pass over its op-string: out[nreplicas][nbonds] */
void ora_batch_bond_counts(ora_replica *const *reps, uint32_t nreplicas, uint32_t nbonds, uint32_t *out) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)nreplicas; ++i) {
        uint32_t *c = out + (size_t)i * nbonds;
        for (uint32_t b = 0; b < nbonds; ++b) c[b] = ora_get_bond_count(reps[i], b);
    }
}

/* The first Philox word of the tempering decision stream (ora_pt_step's counters) for index 0 .. nidx - 1 and chain
 * 0 .. nchains - 1 of one step: out[nidx][nchains] */
void ora_pt_words(uint64_t seed, uint64_t step, uint32_t nidx, uint32_t nchains, uint32_t *out) {
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    for (uint32_t i = 0; i < nidx; ++i)
        for (uint32_t k = 0; k < nchains; ++k) {
            const uint32_t ctr[4] = {i, (uint32_t)step, k, (SSE_TAG_PT << 24) | (uint32_t)((step >> 32) & 0xFFFFFFu)};
            uint32_t o[4];
            ora_philox4x32_10(ctr, key, o);
            out[(size_t)i * nchains + k] = o[0];
        }
}

/* ora_pt_step for every chain of a ladder: by_slot[ntemps][nchains] (row t, column k) is permuted in place, swaps[nchains] */
void ora_batch_pt_step(ora_replica **by_slot, const double *betas, uint32_t ntemps, uint32_t nchains, uint64_t seed, uint64_t step,
                       uint64_t *swaps) {
    ora_replica **chain = (ora_replica **)malloc(sizeof(*chain) * (ntemps ? ntemps : 1));
    for (uint32_t k = 0; k < nchains; ++k) {
        for (uint32_t t = 0; t < ntemps; ++t) chain[t] = by_slot[(size_t)t * nchains + k];
        swaps[k] = ora_pt_step(chain, betas, ntemps, seed, k, step);
        for (uint32_t t = 0; t < ntemps; ++t) by_slot[(size_t)t * nchains + k] = chain[t];
    }
    free(chain);
}

/* Tempering between different Hamiltonians on one graph: the configurations of a[i] and b[i] (op-string, state, update counter,
 * Philox identity, cutoff) change Hamiltonians, i.e. the two replica objects exchange their models.  The models must describe
 * the same variables and bonds (the scratch arrays are sized by them). */
void ora_batch_swap_models(ora_replica *const *a, ora_replica *const *b, uint32_t count) {
    for (uint32_t i = 0; i < count; ++i) { const ora_model *m = a[i]->m; a[i]->m = b[i]->m; b[i]->m = m; }
}
