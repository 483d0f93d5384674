/*
 * sse_oracle.h — CPU ORACLE for the SSE sweep.  TEST INFRASTRUCTURE, NOT PRODUCT.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use this library.
 * It is a plain-C, sequential, one-replica-at-a-time restatement of the reference algorithms
 * (file:line citations at each function in sse_oracle.c).  It shares only the data FORMAT
 * (include/sse_format.h) with the HIP product path; every algorithm is written independently
 * and in the most obvious sequential form, so that agreement with the parallel kernels is evidence.
 *
 * Pinning status: the reference is Rust with un-vendored dependencies and no Rust
 * toolchain exists in this image, so oracle/_ref cannot be built.  The reference's own tests pin only
 * structural invariants (verify()) and a few helper known-answers; energies/magnetisations are pinned
 * here by exact diagonalisation fixtures (tests/golden/ed_*.json, generator tests/golden/make_ed_golden.py).
 * RNG-stream-level parity with the Rust path is impossible by construction (the reference threads a
 * sequential rand::Rng; this build uses counter-based Philox), i.e. "parity unpinned" at the bit level
 * against the reference, statistical (1σ) against exact results.
 */
#ifndef SSE_ORACLE_H
#define SSE_ORACLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ora_model ora_model;
typedef struct ora_replica ora_replica;

/* update flags for ora_timestep(s) — same numeric values as include/isingmc_hip.h */
#define ORA_FLAG_LOOP 1u      /* one directed loop after the diagonal pass (Qmc::timestep) */
#define ORA_FLAG_NO_CLUSTER 2u /* skip the cluster step */
#define ORA_FLAG_HEATBATH 4u  /* heat-bath diagonal rule instead of Metropolis */
#define ORA_FLAG_RVB 8u       /* RVB sweep of (N+1)/2 attempts before the cluster step */

void ora_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

ora_model *ora_model_create(uint32_t nvars, uint32_t nedges, const uint32_t *edge_a, const uint32_t *edge_b,
                            const double *J, double gamma, double h);
/* generic 1- and 2-variable interactions (qmc_runner.rs:415-680); mats[b][in | out<<2] */
ora_model *ora_model_create_generic(uint32_t nvars, uint32_t nbonds, const uint32_t *k, const uint32_t *var_a,
                                    const uint32_t *var_b, const double *mats, double offset);
/* Interaction::at / sym_under_ising (qmc_runner.rs:573-612,639-664): mat is [4^k], or [2^k] when diagonal != 0 */
double ora_interaction_at(uint32_t k, uint32_t diagonal, const double *mat, const uint8_t *inputs, const uint8_t *outputs);
int ora_interaction_sym_under_ising(uint32_t k, uint32_t diagonal, const double *mat);
void ora_model_destroy(ora_model *m);
uint32_t ora_model_nbonds(const ora_model *m);
double ora_model_offset(const ora_model *m);

/* init_state may be NULL: random spins from Philox(tag INIT). */
ora_replica *ora_replica_create(const ora_model *m, uint32_t capacity, uint32_t cutoff0, uint64_t seed,
                                uint32_t replica, const uint8_t *init_state);
void ora_replica_destroy(ora_replica *r);

void ora_diagonal_update(ora_replica *r, double beta);
void ora_heatbath_update(ora_replica *r, double beta);
uint32_t ora_cluster_update(ora_replica *r, double prob);
void ora_flip_free_spins(ora_replica *r);
uint32_t ora_loop_update(ora_replica *r); /* returns number of vertices visited */
/* The same loop; rows (NULL, or [cap_rows][ORA_LOOP_NCOLS]) receives one row per visited vertex, start (NULL, or [2]) the rank nth
 * of the start vertex among the occupied slots and its slot p0.  A walk longer than cap_rows runs to its end and returns its
 * length; only the rows stop.  P slot; ESIDE, EREL the leg entered (side 0 inputs, 1 outputs); XSIDE, XREL the leg left; WORD the
 * op word as rewritten; CLOSED 1 the walk ended at this vertex (directed_loop.rs:266: no search follows, the next four are 0),
 * 2 it ended on arriving at the start leg (:293), 0 it went on.  Of the search that followed: VAR the worldline; DIST the distance
 * 1..cutoff at which the next op was found (cutoff: the op itself); FORWARD the direction; WRAPPED the search passed p = 0. */
enum { ORA_LOOP_P = 0, ORA_LOOP_ESIDE, ORA_LOOP_EREL, ORA_LOOP_XSIDE, ORA_LOOP_XREL, ORA_LOOP_VAR, ORA_LOOP_DIST, ORA_LOOP_FORWARD,
       ORA_LOOP_WRAPPED, ORA_LOOP_CLOSED, ORA_LOOP_WORD, ORA_LOOP_NCOLS };
uint32_t ora_loop_update_trace(ora_replica *r, uint32_t *rows, uint32_t cap_rows, uint32_t *start);
/* RvbUpdater::rvb_update_with_ising_weight (qmc_traits/rvb.rs:88-290): `updates` attempts; returns #accepted */
uint32_t ora_rvb_update(ora_replica *r, uint32_t updates);
/* The same sweep; stats (NULL, or [updates][ORA_RVB_NSTATS]) receives one row per attempt: the sizes that the device kernels hold
 * in fixed arrays.  CSIZE cluster size drawn; NCL members the cluster got; BF, BN peak entries of the two weighted boundary sets
 * (constant-op segments / variables without constant ops) while the cluster grew; NCAND = NCL + the two sets' entries when growth
 * ended (sub-variable candidates, before repeats are dropped); NSUB sub-variables; NTOG toggles after remove_doubles; NWIN time
 * windows with a non-empty cluster (counted for every attempt); BONDS_PROB peak entries of the before / after boundary-bond sets
 * of calculate_flip_prob; BONDS_MUT the same for mutate_graph (0 when rejected); NADJ sum of the sub-variables' degrees; ACCEPT. */
enum { ORA_RVB_CSIZE = 0, ORA_RVB_NCL, ORA_RVB_BF, ORA_RVB_BN, ORA_RVB_NCAND, ORA_RVB_NSUB, ORA_RVB_NTOG, ORA_RVB_NWIN,
       ORA_RVB_BONDS_PROB, ORA_RVB_BONDS_MUT, ORA_RVB_NADJ, ORA_RVB_ACCEPT, ORA_RVB_NSTATS };
uint32_t ora_rvb_update_stats(ora_replica *r, uint32_t updates, uint32_t *stats);
uint32_t ora_find_overlapping_starts(uint32_t p_start, uint32_t p_end, uint32_t cutoff, const uint32_t *fp, uint32_t L,
                                     uint32_t *out);
uint32_t ora_remove_doubles(uint32_t *v, uint32_t n);
int ora_timestep(ora_replica *r, double beta, uint32_t flags);
int ora_timesteps(ora_replica *r, uint64_t t, double beta, uint32_t sampling_freq, uint32_t flags);
int ora_verify(const ora_replica *r);
/* itime_fold (fast_ops.rs:1296-1315) of m, m^2, |m| over p = 0..cutoff-1 */
void ora_itime_magnetization(const ora_replica *r, int64_t *sum_m, uint64_t *sum_m2, uint64_t *sum_abs);

/* one parallel-tempering step of one chain; by_slot[t] = replica at temperature t (pointers are swapped) */
uint64_t ora_pt_step(ora_replica **by_slot, const double *betas, uint32_t ntemps, uint64_t seed, uint32_t chain,
                     uint64_t step);

uint32_t ora_get_n(const ora_replica *r);
uint32_t ora_get_cutoff(const ora_replica *r);
int ora_set_cutoff(ora_replica *r, uint32_t cutoff);
uint64_t ora_get_epoch(const ora_replica *r);
void ora_set_epoch(ora_replica *r, uint64_t epoch);
void ora_get_state(const ora_replica *r, uint8_t *out);
void ora_set_state(ora_replica *r, const uint8_t *in);
void ora_get_ops(const ora_replica *r, uint32_t *out /* cutoff words */);
int ora_set_ops(ora_replica *r, const uint32_t *words, uint32_t cutoff);
uint32_t ora_get_bond_count(const ora_replica *r, uint32_t bond);
/* acc[0]=sum n, acc[1]=nsamples, acc[2]=sum |2up-N|, acc[3]=sum (2up-N)^2, acc[4]=vertices visited by
 * off-diagonal passes, acc[5]=slots visited by diagonal passes, acc[6]=sum over samples of the number of transverse-bond ops */
void ora_get_accumulators(const ora_replica *r, uint64_t acc[8]);
void ora_reset_accumulators(ora_replica *r);

/* batch accessors (sse_oracle_batch.c): one call for many replicas; NULL outputs are skipped; acc is [nreplicas][8] */
void ora_batch_get(ora_replica *const *reps, uint32_t nreplicas, uint32_t *n, uint32_t *cutoff, uint64_t *acc);
void ora_batch_bond_counts(ora_replica *const *reps, uint32_t nreplicas, uint32_t nbonds, uint32_t *out /* [nreplicas][nbonds] */);
/* first Philox word of ora_pt_step's decision stream for index 0 .. nidx - 1 and chain 0 .. nchains - 1: out[nidx][nchains] */
void ora_batch_pt_step(ora_replica **by_slot /* [ntemps][nchains], permuted in place */, const double *betas, uint32_t ntemps,
                       uint32_t nchains, uint64_t seed, uint64_t step, uint64_t *swaps /* [nchains] */);
/* the replicas a[i] and b[i] exchange their models (same variables and bonds): their configurations change Hamiltonians */
void ora_batch_swap_models(ora_replica *const *a, ora_replica *const *b, uint32_t count);
void ora_pt_words(uint64_t seed, uint64_t step, uint32_t nidx, uint32_t nchains, uint32_t *out);

#ifdef __cplusplus
}
#endif
#endif
