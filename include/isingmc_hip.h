/*
 * isingmc_hip.h — C ABI of the MI355X-native SSE sweep engine (libisingmc_hip.so).
 *
 * The reference (Renmusxd/IsingMonteCarlo, crate `qmc`) is 100 % safe Rust with no FFI; its extension
 * point is "implement the manager traits on your own container M and instantiate QmcIsingGraph<R,M> /
 * Qmc<R,M>" (src/sse/qmc_ising.rs:20-23,80-91; src/sse/qmc_runner.rs:21).  A GPU manager cannot serve the
 * per-slot closures of those traits across a device boundary, so the boundary sits at the sweep-level
 * default methods, batch-first (one handle = R independent replicas, as ParallelQmcTimeSteps treats
 * graphs: src/sse/parallel_tempering/tempering_container.rs:321-340).  Each entry point below names the
 * reference interface it replaces.  The Rust-side binding a maintainer would add is in INTEGRATION.md.
 *
 * Conventions: every function returns 0 on success, a negative ISINGMC_E* code otherwise; the message is
 * available from isingmc_last_error().  Array arguments are borrowed for the duration of the call; outputs
 * are caller-allocated.  A handle may be moved between host threads but used by one at a time (!Sync),
 * matching `&mut self` on every reference update.  There is NO CPU fallback: without a HIP device
 * isingmc_create fails with ISINGMC_ENODEVICE.
 */
#ifndef ISINGMC_HIP_H
#define ISINGMC_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "sse_format.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISINGMC_OK 0
#define ISINGMC_EINVAL (-1)    /* bad argument (maps the reference's Result<(),String> errors) */
#define ISINGMC_ENODEVICE (-2) /* no usable HIP device / HIP runtime error */
#define ISINGMC_ECAPACITY (-3) /* cutoff would exceed the preallocated op-string capacity */
#define ISINGMC_EINTEGRITY (-4) /* device-side integrity failure (the reference would panic) */
#define ISINGMC_ENOTIMPL (-5)
#define ISINGMC_ELIMIT (-6)     /* a directed loop did not close within 64*cutoff+1024 vertices (the reference's loop is unbounded,
                                   directed_loop.rs:217-301); the replica's flag is cleared by isingmc_clear_errors */

/* update flags (isingmc_timesteps / isingmc_timestep) */
#define ISINGMC_FLAG_LOOP 1u       /* Qmc::set_do_loop_updates(true): one directed loop per step (qmc_runner.rs:268,366) */
#define ISINGMC_FLAG_NO_CLUSTER 2u /* skip the cluster step */
#define ISINGMC_FLAG_HEATBATH 4u   /* set_enable_heatbath(true) (qmc_ising.rs:444) / set_do_heatbath (qmc_runner.rs:258) */
#define ISINGMC_FLAG_RVB 8u        /* set_run_rvb(true) (qmc_ising.rs:435) */
#define ISINGMC_FLAG_PREP 0x10000u /* profiling label only: run the identical kernel under its "data preparation"
                                      symbol so that profilers separate input generation from the measured sweeps */

/* isingmc_config.flags */
#define ISINGMC_CFG_NO_LDS_TABLES 1u /* keep the bond table in HBM even when it would fit in LDS (testing) */
#define ISINGMC_CFG_PER_REPLICA_J 4u /* `J` holds nreplicas x nedges couplings (row r = replica r): independent disorder
                                        realisations on one graph. */
#define ISINGMC_CFG_GLOBAL_TABLES 8u /* keep the per-variable scan tables (spins, cut ranks) in a per-replica HBM scratch instead of
                                        LDS.  Chosen automatically for models whose tables exceed LDS (N >~ 10^4 variables, e.g. a
                                        32^3 lattice; the compact edge table of a uniform-|J| model leaves LDS first, and
                                        with it the tables of a chain stay in LDS up to N ~ 11000); this flag forces the path
                                        on any model (testing) and then needs
                                        ISINGMC_CFG_NO_LDS_TABLES or non-uniform couplings; slots_per_lane 1 or 4; RVB updates only with
                                        ISINGMC_CFG_RVB_GLOBAL_TABLES (without it they return ISINGMC_ENOTIMPL). */
#define ISINGMC_CFG_NO_FAST_DIAG 16u /* run the diagonal pass through the general kernel even where the instruction-trimmed one
                                        (csrc/sse_fast.hip.h: uniform |J|, N <= 4096, 4 waves per replica) applies (testing / A-B timing) */
/* bits 32 and 64 are retired (two experimental diagonal-to-cluster hand-overs): isingmc_create ignores them; do not reuse them */
#define ISINGMC_CFG_RVB_SERIAL_GROWTH 128u /* RVB sweeps grow the clusters of their attempts one at a time instead of a batch of them side by
                                            side on the waves of the workgroup (testing: the results are the same either way) */
#define ISINGMC_CFG_NO_LEAN_CLUSTER 256u /* run cluster updates through the general kernel even where the dedicated one (csrc/sse_cluster.hip.h:
                                           LDS edge tables, N <= 4095, default wave counts) applies (testing / A-B timing) */
#define ISINGMC_CFG_NO_DEFERRED_FLIPS 512u /* the dedicated cluster kernel rewrites the op-strings itself instead of leaving one flip byte per slot
                                             for the diagonal launch of the next timestep to apply (testing / A-B timing) */
#define ISINGMC_CFG_NO_PM_DECODE 1024u /* large disorder batches (per-replica coupling SIGNS, uniform |J| and fields, tables in HBM) decode
                                          bonds through the per-replica 16-byte records like any other model instead of the shared compact edge
                                          table + per-replica sign bits (testing / A-B timing) */
#define ISINGMC_CFG_RVB_FUSED 2048u /* run RVB sweeps through the fused kernel (growth and attempts in one launch, one replica per CU) even where
                                       the two-launch form applies (csrc/sse_rvb_split.hip.h); same results (testing / measurements) */
#define ISINGMC_CFG_RVB_GLOBAL_TABLES 4096u /* RVB sweeps keep their per-variable tables (constant-op starts and positions, variables without
                                             constant ops, variable -> sub-variable, edge -> boundary-bond entry) in a per-replica HBM scratch
                                             (about 4 (2.5 N + E/2 + capacity) bytes per replica, allocated on the first such sweep) instead of LDS, on
                                             any model: models whose scan tables live in HBM (ISINGMC_CFG_GLOBAL_TABLES) and models with more constant
                                             ops than LDS holds.  Every RVB sweep then runs as a launch of its own (16 waves per replica), also inside
                                             timesteps and with ISINGMC_CFG_FUSED_LAUNCH; never as growth + main launches.  Same results. */
#define ISINGMC_CFG_FUSED_LAUNCH 2u  /* run whole timesteps inside one kernel launch instead of a diagonal-pass launch
                                        followed by an off-diagonal launch per timestep (same results, lower occupancy) */

typedef struct isingmc_batch isingmc_batch;

typedef struct isingmc_config {
    uint32_t struct_size;     /* = sizeof(isingmc_config) */
    uint32_t nreplicas;       /* R independent replicas resident on this device */
    uint32_t nvars;           /* N (reference: max edge index + 1, qmc_ising.rs:92) */
    uint32_t nedges;          /* E */
    const uint32_t *edges;    /* [2E]: a0,b0,a1,b1,...  (Vec<(Edge,f64)>, qmc_ising.rs:81) */
    const double *J;          /* [E]  couplings, J>0 antiferromagnetic (src/lib.rs:29); [R][E] with ISINGMC_CFG_PER_REPLICA_J */
    double transverse;        /* Gamma */
    double longitudinal;      /* h */
    uint32_t capacity;        /* op-string slots preallocated per replica (>= cutoff0) */
    uint32_t cutoff0;         /* initial cutoff (QmcIsingGraph::new_with_rng `cutoff`) */
    uint64_t seed;            /* Philox key; replaces the reference's `rng` argument */
    uint32_t replica_offset;  /* global index of local replica 0 (replica sharding over GPUs) */
    int32_t device;           /* HIP device ordinal, -1 = current device */
    const uint8_t *init_state; /* [R][N] 0/1 or NULL = random (make_random_spin_state, classical/graph.rs:451) */
    uint32_t waves_per_replica; /* 0 = auto (4); workgroup = this many wave64s cooperating on one replica: 1,4,6,8,16 */
    uint32_t slots_per_lane;    /* 0 = auto (4); op-string slots each lane holds per tile: 1,2,4 */
    uint32_t flags;             /* ISINGMC_CFG_* */
    uint32_t lds_uf_ids_limit;  /* 0 = as many cluster-segment ids as fit in LDS; smaller values force the HBM
                                   union-find path earlier (testing) */
    uint32_t waves_offdiag;     /* wave64s per replica for launches without a diagonal pass (directed loop, cluster,
                                 * free spins): 0 = same as waves_per_replica when that is given, otherwise decided
                                 * per launch (16 while the scan tables and the union-find fit in LDS); 1, 4, 6, 8, 16 */
    /* Generic interactions (qmc::sse::Qmc, qmc_runner.rs:94-156, Interaction :415-680).  When `interactions` is non-NULL
     * the batch is built from them and edges / J / transverse / longitudinal are ignored: bond b = interaction b.
     * Available updates: diagonal (Metropolis or heat-bath), directed loop, free spins, and cluster updates when every
     * interaction is symmetric under a global spin flip (Qmc::cluster_update, qmc_runner.rs:222-236; one-variable
     * interactions with four equal entries are the cluster edges).  RVB updates return ISINGMC_ENOTIMPL. */
    const struct isingmc_interaction *interactions;
    uint32_t ninteractions;
    double energy_offset;       /* added to -<n>/beta by isingmc_get_offset (sum of the offsets the caller absorbed,
                                   Qmc::make_interaction_and_offset) */
    /* Per-replica fields, only with ISINGMC_CFG_PER_REPLICA_J (every replica then runs on its own bond table): [R] transverse
     * fields / [R] longitudinal fields replacing `transverse` / `longitudinal`; NULL = the scalar for every replica.  The
     * longitudinal fields must be all zero (|h| <= DBL_EPSILON) or all non-zero: the bond numbering (qmc_ising.rs:228-246) is
     * common to a batch.  Parallel tempering between graphs whose Gamma and h differ (GraphWeights::relative_weight,
     * tempering_traits.rs:126-155) builds on this: the tables belong to the temperature slot. */
    const double *transverse_r;
    const double *longitudinal_r;
} isingmc_config;

/* One interaction: k = 1 or 2 variables and the 4^k matrix of the reference (Interaction::at, qmc_runner.rs:573-612):
 * index = outputs then inputs, first variable most significant, i.e. for k = 2  (out0 out1 in0 in1)  as a 4-bit number.
 * All entries must be >= 0 (they are sampling weights). */
typedef struct isingmc_interaction {
    uint32_t nvars;           /* 1 or 2 (more: ISINGMC_ENOTIMPL, the operator word holds two variables) */
    uint32_t vars[2];
    uint32_t diagonal_only;   /* 0: mat is the full [4^nvars] matrix (InteractionType::Full); 1: mat holds the [2^nvars] diagonal
                                 only (InteractionType::Diagonal, qmc_runner.rs:594-610), every off-diagonal weight is 0 */
    const double *mat;
} isingmc_interaction;

/* Interaction::at (qmc_runner.rs:573-612): the weight for inputs[nvars] / outputs[nvars] (bytes 0/1).  Host-side, no device
 * needed; isingmc_create tabulates every interaction through this function. */
int isingmc_interaction_at(const isingmc_interaction *it, const uint8_t *inputs, const uint8_t *outputs, double *out);
/* Interaction::sym_under_ising (qmc_runner.rs:639-664), restated with its index range as written there: a full matrix is
 * compared on indices [0, 2^nvars) against their bit-complements, a diagonal one on [0, 2^(nvars/2)).  (The engine itself
 * enables cluster updates only when EVERY entry equals its complement's, which implies this.) */
int isingmc_interaction_sym_under_ising(const isingmc_interaction *it, int *out);

/* QmcIsingGraph::new_with_rng (qmc_ising.rs:131-148) + OpContainerConstructor::new_with_bonds
 * (op_container.rs:110), for R replicas at once. */
int isingmc_create(const isingmc_config *cfg, isingmc_batch **out);
/* Drop */
void isingmc_destroy(isingmc_batch *b);
/* error text of the last failing call on this handle (b may be NULL: last isingmc_create failure) */
const char *isingmc_last_error(const isingmc_batch *b);

/* DiagonalUpdater::make_diagonal_update_with_rng_and_state_ref (qmc_traits/diagonal.rs:114-135), or with
 * ISINGMC_FLAG_HEATBATH HeatBathDiagonalUpdater::make_heatbath_diagonal_update_with_rng_and_state_ref
 * (qmc_traits/heatbath.rs:106-127).  beta[R].  Also applies cutoff = max(cutoff, n + n/2)
 * (qmc_ising.rs:269,786; qmc_runner.rs:197). */
int isingmc_diagonal_update(isingmc_batch *b, const double *beta, uint32_t flags);
/* ClusterUpdater::flip_each_cluster_rng (qmc_traits/cluster.rs:36-172) with the weight function of
 * qmc_ising.rs:759-775.  n_clusters[R] may be NULL. */
int isingmc_cluster_update(isingmc_batch *b, double prob, uint32_t *n_clusters);
/* LoopUpdater::make_loop_update_with_rng (qmc_traits/directed_loop.rs:103-171); lengths[R] may be NULL. */
int isingmc_loop_update(isingmc_batch *b, uint32_t *lengths);
/* RvbUpdater::rvb_update_with_ising_weight (qmc_traits/rvb.rs:88-290) as QmcIsingGraph::single_rvb_sweep drives it
 * (qmc_ising.rs:323-418): `updates` attempts per replica (0 = (N+1)/2); successes[R] may be NULL. */
int isingmc_rvb_update(isingmc_batch *b, uint32_t updates, uint32_t *successes);
/* qmc_ising.rs:780-784 / Qmc::flip_free_bits (qmc_runner.rs:241-255) */
int isingmc_flip_free_spins(isingmc_batch *b);
/* QmcStepper::timesteps_measure_with_self (qmc_traits/qmc_stepper.rs:133-162) over
 * QmcIsingGraph::timestep (qmc_ising.rs:644-795) / Qmc::timestep (qmc_runner.rs:363-377), fused on device:
 * t steps, sampling when (step+1) % sampling_freq == 0, accumulating into the per-replica accumulators. */
int isingmc_timesteps(isingmc_batch *b, uint64_t t, const double *beta, uint32_t sampling_freq, uint32_t flags);

/* accumulators [R][8] (u64): 0 sum n, 1 samples, 2 sum |2up-N|, 3 sum (2up-N)^2, 4 vertices visited by
 * off-diagonal passes, 5 slots visited by diagonal passes, 6 sum of transverse-op counts, 7 reserved.
 * Energy: QmcStepper::get_energy_for_average_n (qmc_ising.rs:805-809) = -(acc0/acc1)/beta + offset. */
int isingmc_get_accumulators(isingmc_batch *b, uint64_t *out);
int isingmc_reset_accumulators(isingmc_batch *b);
/* restore accumulators saved by isingmc_get_accumulators (checkpoint / resume): in[nrows][8] */
int isingmc_set_accumulators(isingmc_batch *b, const uint64_t *in);
/* Device-side error flags are sticky per replica (a replica that hit ISINGMC_ECAPACITY / ISINGMC_ELIMIT / an integrity
 * error is skipped by later launches).  This clears all of them; isingmc_import_ops clears the flag of the replica it
 * rewrites.  The reference panics instead (release = abort, Cargo.toml:43), so there is nothing to mirror. */
int isingmc_clear_errors(isingmc_batch *b);
/* QmcIsingGraph::get_offset (qmc_ising.rs:558) */
double isingmc_get_offset(const isingmc_batch *b);
/* the same per replica, out[R] (differs between replicas only with ISINGMC_CFG_PER_REPLICA_J) */
int isingmc_get_offsets(const isingmc_batch *b, double *out);
uint32_t isingmc_num_bonds(const isingmc_batch *b);

/* state_ref / clone_state / state_mut (qmc_ising.rs:497-509,797): out/in are [N] bytes 0/1 of replica r;
 * r == UINT32_MAX addresses all replicas, buffers are then [R][N]. */
int isingmc_get_state(isingmc_batch *b, uint32_t r, uint8_t *out);
int isingmc_set_state(isingmc_batch *b, uint32_t r, const uint8_t *in);
/* OpContainer::get_n / get_cutoff / set_cutoff (qmc_traits/op_container.rs:119-123), out[R] */
int isingmc_get_n(isingmc_batch *b, uint32_t *out);
int isingmc_get_cutoff(isingmc_batch *b, uint32_t *out);
int isingmc_set_cutoff(isingmc_batch *b, uint32_t r, uint32_t cutoff);
int isingmc_get_epoch(isingmc_batch *b, uint64_t *out);
/* restore the per-replica update counters (the Philox epoch): with isingmc_import_ops / isingmc_set_state /
 * isingmc_set_cutoffs this makes a resumed batch continue bit-exactly (checkpoint / resume; the reference's serde
 * support, qmc_ising.rs:1001-1087, serialises the same fields plus its RNG) */
int isingmc_set_epoch(isingmc_batch *b, const uint64_t *epochs);
/* OpContainer::itime_fold (fast_ops.rs:1296-1315; QmcStepper::imaginary_time_fold, qmc_ising.rs:815-821) for the
 * magnetisation m = sum_v (2 s_v - 1) of the propagated state: per replica the sums over p = 0..cutoff-1 of m, m^2
 * and |m| (divide by the cutoff for imaginary-time averages).  Arbitrary closures fold on the host over
 * isingmc_export_ops. */
int isingmc_itime_magnetization(isingmc_batch *b, int64_t *sum_m, uint64_t *sum_m2, uint64_t *sum_abs_m);
/* OpContainer::get_count (op_container.rs:129; fast_ops.rs:1281-1294) */
int isingmc_get_bond_count(isingmc_batch *b, uint32_t r, uint32_t bond, uint32_t *out);
/* itime_fold (fast_ops.rs:1296-1315; QmcStepper::imaginary_time_fold, qmc_ising.rs:815-821) of two-valued observables, every replica,
 * one pass on the device.  Groups exactly as in isingmc_record_series (same validation, same flip convention: the observable's bit is
 * parity(state bits of the group) ^ group_flip[g], 1 standing for +1).  x_g(p) = +1/-1 is the observable on the propagated state BEFORE
 * slot p's op.
 *   sum_all[r][g] = sum over p < cutoff[r] of x_g(p)
 *   sum_occ[r][g] = the same sum over occupied slots only (ops[p] != 0)
 * Either pointer may be NULL (not both).  Rows are replicas (not tempering slots).  Exact integers: x_g only changes at off-diagonal ops,
 * and the fold is evaluated from those (csrc/sse_itime.h).  The batch is left as it was (pending cluster flips are brought into the
 * op-strings first, as by isingmc_verify).  ISINGMC_ENOTIMPL, before anything is launched, when the groups' sums and bit arrays exceed
 * LDS: 16 bytes per group and N / 2 bytes (about 9800 groups at N = 1024, 8600 at N = 32768); the message names the cap. */
int isingmc_itime_groups(isingmc_batch *b, uint32_t ngroups, const uint32_t *group_start, const uint32_t *group_vars, const uint8_t *group_flip,
                         int64_t *sum_all, int64_t *sum_occ);
/* OpContainer::get_count (op_container.rs:129; fast_ops.rs:1281-1294) for every bond of every replica in one pass on the device:
 * out[R][isingmc_num_bonds] */
int isingmc_bond_counts(isingmc_batch *b, uint32_t *out);
/* get_pth for every p (op_container.rs:127): words[cutoff] in the sse_format.h encoding */
int isingmc_export_ops(isingmc_batch *b, uint32_t r, uint32_t *words, uint32_t nwords);
/* FastOps::new_from_ops (fast_ops.rs:80-174): install an op-string (words[nwords], slot p = index) */
int isingmc_import_ops(isingmc_batch *b, uint32_t r, const uint32_t *words, uint32_t nwords);
/* DebugOps::count_diagonal_and_off and count_constant_ops (qmc_debug.rs:10-41) for every replica: out[R][3] = diagonal ops,
 * off-diagonal ops (their sum is get_n), constant ops */
int isingmc_debug_counts(isingmc_batch *b, uint32_t *out);
/* Verify::verify (qmc_ising.rs:829-860; op_container.rs:137-159), ok[R] */
int isingmc_verify(isingmc_batch *b, uint8_t *ok);

/* ---- parallel tempering (src/sse/parallel_tempering/tempering_container.rs) -------------------------------
 * Configurations never move: a tempering swap exchanges the TEMPERATURE LABELS of two configurations (the
 * reference swaps (manager,state) between (graph,beta) slots, qmc_ising.rs:593-602 — the same thing seen
 * from the other side).  The per-replica beta[] argument of isingmc_timesteps carries the current labels. */
/* TemperingContainer::tempering_step decisions (:121-149, :241-302) for nchains independent chains of ntemps
 * temperatures sharing one Hamiltonian; host-side control logic exactly like the reference's container.
 *   betas[ntemps]; n_of_config[nchains*ntemps] = operator count of every configuration (global ids);
 *   config_at[ntemps*nchains] in/out: configuration id at slot t*nchains+chain; *nswaps += swaps done.
 * Philox tag PT: replica field = chain, epoch = step, index 0 = order coin, 1+t = pair (t,t+1). */
int isingmc_pt_decide(uint64_t seed, uint64_t step, uint32_t nchains, uint32_t ntemps, const double *betas,
                      const uint32_t *n_of_config, uint32_t *config_at, uint64_t *nswaps);
/* set_op_cutoff for every replica at once (tempering_container.rs:129-137): cutoffs[R], each only grows */
int isingmc_set_cutoffs(isingmc_batch *b, const uint32_t *cutoffs);
/* replica r accumulates into row rows[r] of an accumulator table with nrows rows (default: nrows = R, rows[r] = r);
 * isingmc_get_accumulators then returns [nrows][8].  Used to keep statistics per temperature slot. */
int isingmc_set_accumulator_rows(isingmc_batch *b, uint32_t nrows, const uint32_t *rows);

/* ---- native tempering step: temperature blocks sharded over ranks, neighbour exchange point to point --------------------
 * Rank g of `world` owns ntemps/world consecutive temperatures of every chain; its batch holds ntemps/world * nchains
 * replicas (replica r starts as slot (g*tper + r / nchains, r % nchains), isingmc_config.replica_offset = g * R).  Swaps inside
 * the block exchange temperature labels; at a block boundary the two ranks exchange the boundary walkers' operator counts
 * (tempering_container.rs:274-302: the swap test needs nothing else) and, when a swap is accepted, the two configurations
 * themselves, so that a rank always holds the configurations of its own temperatures.  Transport: RCCL ncclSend / ncclRecv on
 * device buffers inside one group call per exchange once isingmc_pt_attach_nccl succeeded, otherwise the host-staged
 * `transport` of the layout (one rank: none needed). */
typedef struct isingmc_pt_transport {
    void *ctx;
    /* blocking exchange with rank `peer`: send sbytes from sbuf and receive rbytes into rbuf (host memory); 0 on success */
    int (*sendrecv)(void *ctx, int peer, const void *sbuf, size_t sbytes, void *rbuf, size_t rbytes);
    /* element-wise maximum over all ranks, in place; 0 on success */
    int (*allreduce_max_u32)(void *ctx, uint32_t *buf, size_t count);
} isingmc_pt_transport;
typedef struct isingmc_pt_layout {
    uint32_t struct_size;     /* = sizeof(isingmc_pt_layout) */
    uint32_t ntemps, nchains; /* global */
    uint32_t rank, world;
    const double *betas;      /* [ntemps] */
    uint64_t seed;            /* Philox key of the swap decisions (the same on every rank) */
    const isingmc_pt_transport *transport; /* may be NULL when world == 1 */
} isingmc_pt_layout;
typedef struct isingmc_nccl_id { char internal[128]; } isingmc_nccl_id; /* = ncclUniqueId */
/* TemperingContainer::new + add_qmc_stepper (tempering_container.rs:40-75) for a batch that already holds the replicas.
 * With ISINGMC_CFG_PER_REPLICA_J the couplings belong to the temperature slot (row r of J = slot r of this rank) and swaps
 * use GraphWeights::relative_weight (tempering_traits.rs:126-155; the fields are common to the batch). */
int isingmc_pt_create(isingmc_batch *b, const isingmc_pt_layout *layout);
/* ncclGetUniqueId (rank 0, then broadcast by the launcher) and ncclCommInitRank for this batch's rank / world */
int isingmc_pt_nccl_unique_id(isingmc_nccl_id *out);
int isingmc_pt_attach_nccl(isingmc_batch *b, const isingmc_nccl_id *id);
/* TemperingContainer::tempering_step (tempering_container.rs:121-149).  *nswaps += swaps whose LOWER temperature this rank owns.
 * Accumulator rows: a swap inside a rank exchanges the labels of two replicas, so statistics per temperature need the rows to follow
 * the labels.  They do exactly when the caller has asked for it: isingmc_set_accumulator_rows, called after isingmc_pt_create with
 * nrows = ntemps * nchains and rows[r] = the slot of replica r (isingmc_pt_get_slots), makes every later isingmc_pt_step (and
 * isingmc_pt_set_state) keep row = slot, on the device path and on the host path alike.  Any other rows, the default ones (row r for
 * replica r) included, are left alone by both paths: they then count per replica, i.e. per configuration on a single rank.  A new
 * isingmc_pt_create or isingmc_set_accumulator_rows call with other rows ends the following. */
int isingmc_pt_step(isingmc_batch *b, uint64_t *nswaps);
/* Where the swap decisions are taken.  A rank that owns every temperature of a batch with one Hamiltonian (world == 1, no
 * ISINGMC_CFG_PER_REPLICA_J) decides on the device by default: one small kernel per step equalises the cutoffs of each chain, draws the
 * same Philox numbers as the host path and swaps the labels in device memory; nothing is copied to the host unless the caller asks
 * (isingmc_pt_step with nswaps != NULL reads 8 bytes back; isingmc_pt_get_slots / get_state refresh the host mirrors).  on = 0
 * returns to the host path (same decisions: tested).  Multi-rank layouts and different Hamiltonians per temperature decide on the host. */
int isingmc_pt_set_device_decisions(isingmc_batch *b, int on);
int isingmc_pt_get_device_decisions(const isingmc_batch *b, int *on);
/* isingmc_timesteps at the temperatures of the current labels (TemperingContainer::timesteps, tempering_container.rs:100-119); with
 * device-side decisions the per-replica betas are read from device memory, no host array is involved */
int isingmc_pt_timesteps(isingmc_batch *b, uint64_t t, uint32_t sampling_freq, uint32_t flags);
/* current labels of the local replicas: global slot (t * nchains + chain), its beta, and the configuration's identity */
int isingmc_pt_get_slots(isingmc_batch *b, uint32_t *slot_of_replica, double *beta_of_replica, uint32_t *config_id_of_replica);

/* container-level save / load (the reference serialises the whole container, tempering_container.rs:683-792): labels, configuration
 * identities, step counter and swap count; the replicas themselves travel through export_ops / get_state / get_epoch */
int isingmc_pt_get_state(isingmc_batch *b, uint64_t *step, uint64_t *total_swaps);
int isingmc_pt_set_state(isingmc_batch *b, const uint32_t *slot_of_replica, const uint32_t *config_id_of_replica, uint64_t step, uint64_t total_swaps);

/* ---- sample record: the sampled p = 0 states kept on the device, and exact autocorrelations of two-valued observables ------------
 * QmcStepper::timesteps_sample / timesteps_measure (qmc_traits/qmc_stepper.rs:23-95) hand the caller the state at every sampled
 * step, and autocorrelations.rs builds on that list.  While a record is attached, every sampled step of isingmc_timesteps
 * ((step + 1) % sampling_freq == 0) appends the p = 0 states of all replicas, exactly what isingmc_get_state would return if the
 * call ended on that step: a device-to-device copy on the batch's stream, no host synchronisation.  The record is
 * [capacity][R][state words] in device memory; rows are indexed by replica, not by tempering slot (isingmc_pt_timesteps goes
 * through isingmc_timesteps and records too).  A call whose t / sampling_freq samples do not fit returns ISINGMC_ECAPACITY before
 * anything is launched and leaves the batch and the record as they were.  Launches that run several steps
 * (ISINGMC_CFG_FUSED_LAUNCH) end on each sampled step while a record is attached: same epochs, same results.  Nothing is
 * recorded, and no launch changes, without a record.  Checkpoints do not carry the record. */
/* capacity samples (<= 1 << 20); 0 detaches and frees; attaching again replaces the record by an empty one */
int isingmc_record_attach(isingmc_batch *b, uint32_t capacity);
/* rows written so far and the capacity (both 0 without a record); either pointer may be NULL */
int isingmc_record_count(const isingmc_batch *b, uint32_t *count, uint32_t *capacity);
/* the next sample goes to row 0 again */
int isingmc_record_clear(isingmc_batch *b);
/* rows first .. first + count - 1 as bytes 0/1 like isingmc_get_state: out[count][N] of replica r; r == UINT32_MAX: out[count][R][N] */
int isingmc_record_read(isingmc_batch *b, uint32_t first, uint32_t count, uint32_t r, uint8_t *out);
/* Two-valued observables of the recorded states.  Observable g is the group of variables group_vars[group_start[g] ..
 * group_start[g + 1]) (non-empty, variables < N, group_start[0] = 0; a variable may repeat across groups) and a flip bit: its bit at
 * sample t is parity(state bits of the group) ^ group_flip[g] (NULL: no flips), 1 standing for the value +1.  This covers a variable
 * (autocorrelations.rs:37-50: {v}, 0), a product of spins (:52-75: its variables, 1 if their number is even) and a bond
 * (qmc_ising.rs:988-997: {a, b}, 1 if J < 0).  out_bits[R][ngroups][(count + 31) / 32]: bit t & 31 of word t >> 5 is sample
 * first + t; unused high bits of the last word are 0.  ISINGMC_ENOTIMPL for models whose 64 state rows exceed LDS (N > ~20000). */
int isingmc_record_series(isingmc_batch *b, uint32_t ngroups, const uint32_t *group_start, const uint32_t *group_vars, const uint8_t *group_flip,
                          uint32_t first, uint32_t count, uint32_t *out_bits);
/* fft_autocorrelation (autocorrelations.rs:99-133) of those observables over samples first .. first + count - 1, without transforms
 * and exact: with T = count, x the +-1 series of one observable, s = sum_t x[t] and C(tau) = sum_t x[t] x[(t + tau) mod T] =
 * T - 2 popcount(bits ^ rotate(bits, tau)), the observable contributes (T C(tau) - s^2) / (T^2 - s^2) (integers up to this one
 * double division; 0 for a series that never changed); out[R][count] is the mean over the observables, added in group order.  The
 * result does not depend on the flips and is reproducible bit for bit.  ISINGMC_ENOTIMPL when the series, twice, exceeds LDS
 * (count > ~650000). */
int isingmc_record_autocorrelation(isingmc_batch *b, uint32_t ngroups, const uint32_t *group_start, const uint32_t *group_vars,
                                   uint32_t first, uint32_t count, double *out);

/* stream plumbing: use the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) */
int isingmc_set_stream(isingmc_batch *b, void *hip_stream);
int isingmc_synchronize(isingmc_batch *b);
/* HIP-event timing of the most recent isingmc_timesteps launch(es): total ms and number of kernel launches */
int isingmc_last_kernel_ms(isingmc_batch *b, float *ms, uint32_t *launches);
/* the same run split by kernel: ms[0]/launches[0] = diagonal-pass launches, ms[1]/launches[1] = all other launches */
int isingmc_last_pass_ms(isingmc_batch *b, float ms[2], uint32_t launches[2]);
/* ... and, of ms[1], the part spent in the RVB-sweep launches of split timesteps (0 when none ran) */
int isingmc_last_rvb_ms(isingmc_batch *b, float *ms, uint32_t *launches);
/* out[R][16] per-replica debug words.  Diagnostic builds (-DSSE_PHASE_TIMING): phase durations in 10-ns ticks.  Every build: the
 * dedicated cluster kernel adds the unions its build scan parked to word 11 and the queue drains in front of a range's last one to
 * word 15 (whole queues: 64 unions each); the other words are zero outside diagnostic builds.  reset != 0 clears the array. */
int isingmc_debug_phase_ticks(isingmc_batch *b, uint64_t *out, int reset);
/* number of sweeps fused into one kernel launch by isingmc_timesteps (0 = all t steps in one launch) */
int isingmc_set_steps_per_launch(isingmc_batch *b, uint64_t steps);
/* build/launch configuration actually in use: out[0]=waves per replica, out[1]=dynamic LDS bytes,
 * out[2]=union-find ids that fit in LDS, out[3]=state words per replica, out[4]=slots per lane,
 * out[5]=1 if the edge table is staged in LDS, out[6]=bit 0: timesteps are issued as two launches (diagonal, rest); bit 1: per-variable
 * tables live in HBM (ISINGMC_CFG_GLOBAL_TABLES path); bit 2: the diagonal-pass launch is the trimmed kernel of sse_fast.hip.h; bits 3-4:
 * reserved (always 0); bit 5: the most recent cluster launch was the dedicated kernel; bit 6: the most recent RVB sweep ran as
 * growth + main launches (bits 16-23: waves per replica of that main launch); bit 7: the most recent RVB sweep kept its per-variable
 * tables in HBM (ISINGMC_CFG_RVB_GLOBAL_TABLES); bits 8-15: waves per replica of the most recent
 * off-diagonal launch, out[7]=dynamic LDS bytes of the diagonal-pass launch */
int isingmc_get_launch_info(const isingmc_batch *b, uint32_t out[8]);
/* Host-only: the chunk grid and op-string row stride isingmc_create derives for `capacity` slots and kernels of W (diagonal
 * launches) / up to Wmax (off-diagonal launches) wave64s per replica at K slots per lane: out = {chunk size, chunks, row stride in
 * words, tile = slots of the widest whole-tile access}.  Exposed so that the bounds every kernel relies on (whole-tile loads and
 * stores, the prefetch of an empty chunk range, cached-id rows) can be asserted on a CPU box. */
int isingmc_plan_geometry(uint32_t capacity, uint32_t W, uint32_t K, uint32_t Wmax, uint32_t out[4]);
/* Host-only: the LDS layout of the dedicated cluster kernel (16 waves) for N variables (nwords state words, Nb bonds), a 16-bit
 * parent table of ufcap ids, has_long != 0 when the model has a longitudinal field, and a replica with S ids (16 N + cuts):
 * out = {word offsets o_tab, o_state, o_touch, o_misc, o_chn, o_chtr, o_ent (per-wave tables, after the joins: S flip bits, then
 * the u16 root list), o_frozen, o_froot, o_parent; dynamic LDS words of the launch; 1 if the replica is the kernel's case (else
 * it is left to the general kernel); entries of the root list}.  Exposed so that the layout can be asserted on a CPU box. */
int isingmc_plan_cluster_lds(uint32_t N, uint32_t nwords, uint32_t Nb, uint32_t has_long, uint32_t ufcap, uint32_t S, uint32_t out[13]);
/* Host-only: in that layout, the per-wave queues of unions the build scan parks (16 x (entries + 1 count word), in front of o_ent):
 * out = {word offset, words, entries per wave}. */
int isingmc_plan_cluster_queue(uint32_t N, uint32_t nwords, uint32_t Nb, uint32_t has_long, uint32_t ufcap, uint32_t out[3]);
/* Host-only: every launch geometry and mode isingmc_create chooses for cfg on a device whose workgroups have lds_bytes of LDS, by the
 * function create itself calls; or the code and message (isingmc_last_error(NULL)) create would refuse cfg with once it has found a
 * device.  No device is looked for and nothing is allocated.  LDS sizes are in 32-bit words.
 *   out[0]  W waves per replica            out[1]  K slots per lane             out[2]  mode (0 general bond table, 1 compact edge
 *   table in LDS, 2 per-variable tables in HBM, 4 the same with the +-J decode)
 *   out[3]  waves of off-diagonal launches (0 = decided per launch)             out[4]  Wmax, most waves of any launch
 *   out[5]  1 if the 8-wave geometry without an LDS union-find is allowed       out[6..8]  chunk size, chunks, row stride
 *   (isingmc_plan_geometry)                out[9]  +-J decode: sign words per bond-table row
 *   out[10] +-J decode: LDS of the diagonal launch with its spin bytes in LDS (0 = they stay in HBM)
 *   out[11] LDS of the general diagonal launch                                  out[12] LDS of the trimmed diagonal kernel
 *   out[13] 1 = the trimmed diagonal kernel runs        out[14] 1 = the dedicated cluster kernel may run
 *   out[15] 1 = its flips are deferred to the next diagonal launch              out[16] LDS of a general launch with an RVB sweep
 *   out[17] 1 = RVB sweeps keep their tables in HBM      out[18] 1 = RVB sweeps run as growth + main launch
 *   out[19] waves of that main launch      out[20] bytes per replica of the per-variable tables in HBM (0 = in LDS)
 *   out[21], out[22] words per replica of the union-find scratch in HBM (low, high half)
 *   out[23] LDS of the general launch and out[24] ids of its LDS union-find, both before any sweep has run
 *   out[25] state words per replica        out[26] bonds                        out[27..31] 0 */
int isingmc_plan_batch(const isingmc_config *cfg, uint32_t lds_bytes, uint32_t out[32]);
/* Host-only, a device-free test entry: the swap decisions of one phase (0, 1) of isingmc_pt_step's host leg as one rank sees them,
 * by the function the step itself calls (the rule: csrc/pt_rule.h).  Rank `rank` of `world` owns temperatures [rank * tper,
 * (rank + 1) * tper) of nchains chains: R = tper * nchains local replicas, local slot ls = (t - rank * tper) * nchains + chain.
 * Side 0 is the lower neighbour (rank - 1), side 1 the upper one; a side without a neighbour is ignored (pointers may be NULL).
 * An accepted pair inside the block exchanges the labels of its two replicas (slot_of, at); an accepted pair across a boundary
 * becomes an item of that side, (replica, word offset of its configuration in the message, cutoff) as the pack kernel takes them, in
 * chain order on both ranks: the caller moves the configurations (and their operator counts) before the next phase.  Neither a
 * device nor an isingmc_batch is read, so ranks with two neighbours can be simulated in one process. */
typedef struct isingmc_pt_wire { /* what neighbours exchange per chain and phase: 16 bytes */
    uint32_t n, pad; /* operator count of the boundary walker */
    double rel;      /* its relative weight towards the other side's Hamiltonian; read only when the boundary pair is in the phase */
} isingmc_pt_wire;
typedef struct isingmc_pt_phase {
    uint32_t struct_size; /* = sizeof(isingmc_pt_phase) */
    uint32_t rank, world, tper, nchains, phase;
    const double *betas;  /* [world * tper] */
    uint64_t seed, step;
    const uint32_t *n;    /* [R] operator count of local replica r */
    const double *rel;    /* [R] relative weight of replica r towards the partner of its pair in this phase; NULL: all 1 (one Hamiltonian) */
    const isingmc_pt_wire *from[2]; /* [nchains] what the neighbour of that side sent */
    const uint32_t *cutoff;         /* [nchains] the chain's (equalised) cutoff */
    uint32_t fixed_words;           /* words of a configuration in the message besides its cutoff op words */
    uint32_t *slot_of, *at;         /* in/out [R]: global slot t * nchains + chain of replica r; replica at local slot ls */
    uint32_t *items[2];             /* out [3 * nchains] per side */
    uint32_t nitems[2];             /* out */
    uint64_t words[2];              /* out: words of that side's message */
    uint64_t nswaps;                /* out: accepted pairs whose LOWER temperature this rank owns */
} isingmc_pt_phase;
int isingmc_pt_plan_phase(isingmc_pt_phase *view);

/* ---- classical Monte Carlo: qmc::classical::GraphState (src/classical/graph.rs) for a batch of replicas --------------------------
 * One handle = R replicas of one graph (edges and biases common to the batch; couplings common, or with
 * ISINGMC_CLASSICAL_CFG_PER_REPLICA_J one row per replica: disorder realisations; beta per replica), resident on one device.
 * The moves are stated once in csrc/classical_rule.h; their random numbers are the Philox streams of sse_format.h (tags CLASSICAL
 * and CLASSICAL_WORM; epoch = the replica's time-step counter), so a run is a function of (seed, replica, epoch) alone: any split of
 * a run into calls, batches or devices gives the same states.  On the device one wave64 owns a replica and evaluates 64 consecutive
 * moves of a spin or edge step side by side (csrc/sse_classical.hip.h); the result equals the sequential rule move for move. */
#define ISINGMC_CLASSICAL_CFG_EDGE_IMPORTANCE 1u /* enable_edge_importance_sampling(true) (graph.rs:320-336); needs every J > 0 */
#define ISINGMC_CLASSICAL_CFG_GLOBAL_TABLES 2u   /* keep the graph tables in global memory even when they fit in LDS (testing) */
#define ISINGMC_CLASSICAL_CFG_SERIAL_MOVES 4u    /* the wave takes one move at a time (testing / A-B timing); same results */
/* J is [R][E], row r for local replica r (as ISINGMC_CFG_PER_REPLICA_J of isingmc_create): disorder realisations on one topology.
 * Replica r runs exactly as a replica of a shared-coupling batch with J = row r at the same global index replica_offset + r. */
#define ISINGMC_CLASSICAL_CFG_PER_REPLICA_J 8u
#define ISINGMC_CLASSICAL_CFG_GLOBAL_CODES 16u /* keep the per-replica coupling codes in global memory (testing / A-B timing); same results */
/* `kinds` of isingmc_classical_timesteps */
#define ISINGMC_CLASSICAL_KINDS_ALL 0u   /* spin, edge or worm step, drawn per step as do_time_step does (graph.rs:364-365) */
#define ISINGMC_CLASSICAL_KINDS_BASIC 1u /* only_basic_moves = Some(true): spin or edge step */
#define ISINGMC_CLASSICAL_KINDS_SPIN 2u  /* every step: nspin x do_spin_flip */
#define ISINGMC_CLASSICAL_KINDS_EDGE 3u  /* every step: nedge x do_edge_flip */
#define ISINGMC_CLASSICAL_KINDS_WORM 4u  /* every step: nworm x do_worm_flip with allow_doubles = true (as do_time_step calls it) */
#define ISINGMC_CLASSICAL_KINDS_WORM_NO_DOUBLES 5u /* ... with allow_doubles = false (the reference's own tests, graph.rs:481-562) */

typedef struct isingmc_classical isingmc_classical;
typedef struct isingmc_classical_config {
    uint32_t struct_size;      /* = sizeof(isingmc_classical_config) */
    uint32_t nreplicas;        /* R */
    uint32_t nvars;            /* N = biases.len() (graph.rs:69); at most 2^24 */
    uint32_t nedges;           /* E >= 1 (the reference's edge move would panic on an empty edge list) */
    const uint32_t *edges;     /* [2E]: a0,b0,a1,b1,...; a self-loop is ISINGMC_EINVAL as in isingmc_create */
    const double *J;           /* [E]; [R][E] with ISINGMC_CLASSICAL_CFG_PER_REPLICA_J */
    const double *biases;      /* [N] longitudinal fields, or NULL: all zero */
    uint64_t seed;             /* Philox key */
    uint32_t replica_offset;   /* global index of local replica 0 */
    int32_t device;            /* HIP device ordinal, -1 = current device */
    const uint8_t *init_state; /* [R][N] 0/1, or NULL: random under SSE_TAG_INIT exactly as isingmc_create draws it */
    uint32_t flags;            /* ISINGMC_CLASSICAL_CFG_* */
} isingmc_classical_config;

/* GraphState::new / new_with_state_and_rng (graph.rs:56-88).  No CPU fallback: ISINGMC_ENODEVICE without a HIP device.
 * ISINGMC_ENOTIMPL, before anything is allocated, when the per-replica state bits and move stamps (N / 8 + N bytes) exceed LDS. */
int isingmc_classical_create(const isingmc_classical_config *cfg, isingmc_classical **out);
void isingmc_classical_destroy(isingmc_classical *g);
/* error text of the last failing call on this handle (g may be NULL: the last failing create / plan / host_steps call) */
const char *isingmc_classical_last_error(const isingmc_classical *g);
/* t x do_time_step (graph.rs:350-406) for every replica in one launch; beta[R].  nspin / nedge / nworm: moves per spin / edge /
 * worm step, UINT32_MAX = the reference's None: max(1, N / 2), max(1, E / 2), 1.  kinds: ISINGMC_CLASSICAL_KINDS_*. */
int isingmc_classical_timesteps(isingmc_classical *g, uint64_t t, const double *beta, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds);
/* state_ref / clone_state / set_state (graph.rs:414-427): [N] bytes 0/1 of replica r; r == UINT32_MAX: all replicas, [R][N] */
int isingmc_classical_get_state(isingmc_classical *g, uint32_t r, uint8_t *out);
int isingmc_classical_set_state(isingmc_classical *g, uint32_t r, const uint8_t *in);
/* the per-replica time-step counters (the Philox epoch), [R]: with get / set_state a run resumes bit-exactly */
int isingmc_classical_get_epoch(isingmc_classical *g, uint64_t *out);
int isingmc_classical_set_epoch(isingmc_classical *g, const uint64_t *epochs);
/* get_energy (graph.rs:430-447) of every replica, one pass on the device: out[R] */
int isingmc_classical_energies(isingmc_classical *g, double *out);
/* out[R][8]: spin moves attempted, accepted, edge moves attempted, accepted, worms attempted, kept (neither failed nor rejected by the
 * field energy), worm failures (path longer than N, graph.rs:281-285), worm path entries */
int isingmc_classical_counters(isingmc_classical *g, uint64_t *out);
int isingmc_classical_set_stream(isingmc_classical *g, void *hip_stream);
int isingmc_classical_synchronize(isingmc_classical *g);
/* HIP-event time of the most recent isingmc_classical_timesteps launch */
int isingmc_classical_last_kernel_ms(isingmc_classical *g, float *ms);
/* Host-only, a device-free test entry: the launch isingmc_classical_create plans for cfg on a device whose workgroups have lds_bytes
 * of LDS, by the function create itself calls, or the code and message it would refuse cfg with.  out[0] waves (= replicas) per
 * workgroup; out[1] which tables live in LDS, bit 0 row starts, 1 row entries, 2 couplings, 3 biases, 4 edge list, 5 cumulative edge
 * weights, 6 the per-replica coupling table (a table the model does not have has its bit clear); out[2] dynamic LDS words of the
 * launch; out[3] LDS words per wave (state bits and stamp bytes, and the wave's coupling codes when they are in LDS); out[4] bits of
 * out[1] that the model has at all; out[5] 1 = couplings kept as a dictionary of at most 256 values; out[6] 1 = edges packed into
 * one word; out[7] the coupling format: 0 shared by the batch, 1 per-replica code bytes into a dictionary of the whole batch (at most
 * 256 distinct values over all R E couplings), 2 per-replica doubles.  With per-replica couplings bit 2 is the dictionary (format 1
 * only), and the doubles of format 2 and the per-replica cumulative weights are read from global memory always. */
int isingmc_classical_plan(const isingmc_classical_config *cfg, uint32_t lds_bytes, uint32_t out[8]);
/* The launch this handle runs with: the eight slots of isingmc_classical_plan, as isingmc_classical_create chose them from the LDS
 * size of the handle's own device.  Read-only; no device call. */
int isingmc_classical_launch_plan(isingmc_classical *g, uint32_t out[8]);
/* Host-only, a device-free test entry: t time steps of the sequential rule (csrc/classical_rule.h) on the CPU, for the graph, seed
 * and replica_offset of cfg (init_state is not read): states[R][N] and epochs[R] in / out, counters[R][8] added to (may be NULL).
 * exp is the host's libm. */
int isingmc_classical_host_steps(const isingmc_classical_config *cfg, uint64_t t, const double *beta, uint32_t nspin, uint32_t nedge,
                                 uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint64_t *counters);

/* ---- classical parallel tempering (replica exchange) on the device; the rule is stated once in csrc/classical_pt_rule.h ----
 * The batch is C chains of T = ntemps temperatures, R = C T, slot r = c T + i; betas[T] is one ladder shared by the chains (finite,
 * any order, equal neighbours allowed).  temp_of[r] is the temperature index slot r holds (initially r % T).  A swap exchanges
 * temperature labels: states, epochs, move counters and Philox streams stay with their slots.  The swap decisions of chain
 * replica_offset / T + c come from the SSE_TAG_PT stream at the handle's step number pt_step, so a run is a function of (seed,
 * replica_offset, pt_step, the states) alone.  One round = `steps` time steps of every slot at betas[temp_of[r]], then one launch that
 * computes every slot's energy and magnetisation, records them by temperature (the values before the round's swaps) and takes one
 * tempering step of every chain; pt_step increments per round.
 * Errors (ISINGMC_EINVAL with a message): ntemps < 2, R % ntemps != 0, replica_offset % ntemps != 0, a non-finite beta, a null
 * ladder; with ISINGMC_CLASSICAL_CFG_PER_REPLICA_J, a chain whose T coupling rows are not bitwise equal (the swap rule holds inside
 * one Hamiltonian: the batch is C realisations x T temperatures; chains may differ from each other); pt_run / pt_get / pt_set / pt_swap_counts before pt_attach.  isingmc_classical_timesteps on an attached handle behaves as
 * without tempering: it takes its own beta array and leaves the maps alone. */
/* Allocate (first call) and reset the maps, the swap counters and pt_step. */
int isingmc_classical_pt_attach(isingmc_classical *g, uint32_t ntemps, const double *betas);
/* rounds x (steps launch, tempering launch) enqueued on the handle's stream, one synchronisation at the end.  energy_out
 * double [rounds][C][T] and mag_out int32 [rounds][C][T] (M = sum_v (2 s_v - 1)) by temperature, either may be NULL.  rounds == 0 is a
 * no-op; steps == 0 gives swaps only.  nspin / nedge / nworm / kinds as in isingmc_classical_timesteps. */
int isingmc_classical_pt_run(isingmc_classical *g, uint64_t rounds, uint64_t steps, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds,
                             double *energy_out, int32_t *mag_out);
/* temp_of[R] and pt_step, for checkpoints (either output may be NULL); set refuses what is not a permutation within each chain */
int isingmc_classical_pt_get(isingmc_classical *g, uint32_t *temp_of, uint64_t *pt_step);
int isingmc_classical_pt_set(isingmc_classical *g, const uint32_t *temp_of, uint64_t pt_step);
/* swap attempts and acceptances of the pairs (t, t + 1), uint64 [C][T - 1] each, cumulative since attach (either may be NULL);
 * set_swap_counts restores them from a checkpoint */
int isingmc_classical_pt_swap_counts(isingmc_classical *g, uint64_t *attempts, uint64_t *accepts);
int isingmc_classical_pt_set_swap_counts(isingmc_classical *g, const uint64_t *attempts, const uint64_t *accepts);
/* Host-only, a device-free test entry: the same rounds by the sequential rule on the CPU (the step loop of
 * isingmc_classical_host_steps, the energy in the kernel's order of additions), with attach's argument checks.  states[R][N],
 * epochs[R], temp_of[R] and *pt_step in / out; counters[R][8], attempts and accepts [C][T - 1] added to (may be NULL); energy_out and
 * mag_out as in isingmc_classical_pt_run.  exp is the host's libm. */
int isingmc_classical_host_pt_run(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint64_t rounds, uint64_t steps,
                                  uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                                  uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out);

/* ---- overlaps between copies of a realisation under tempering; the definitions are stated once in csrc/classical_overlap_rule.h ----
 * With ncopies = K >= 2 consecutive chains form G = C / K groups of K independent copies of one realisation; the pairs of a group are
 * (a, b), 0 <= a < b < K, a-major, P = K (K - 1) / 2.  A measured round compares, after its time steps and before its swaps, the two
 * states that hold temperature t in the chains g K + a and g K + b: nq variables differ (spin overlap Q = N - 2 nq) and nl entries of
 * the edge list have one endpoint that differs and one that does not (link overlap QL = E - 2 nl; multi-edges count apiece, the
 * value of J does not matter).  The histograms hq [G][P][T][N + 1] (by nq) and hl [G][P][T][E + 1] (by nl), uint64, gain one count
 * per measured round and accumulate over calls until reset.
 * ISINGMC_EINVAL: ncopies == 1; C not a multiple of K; replica_offset / T not a multiple of K (a batch splits over handles at whole
 * groups); per-replica couplings whose rows differ within a group (compared as bits: +0 and -0 differ); tempering not attached; the
 * other overlap calls before overlap_attach. */
/* Needs isingmc_classical_pt_attach.  Allocates and zeroes both histograms; ncopies == 0 detaches and frees them.
 * isingmc_classical_pt_attach on a handle with overlaps detaches them: the shape of the batch changed. */
int isingmc_classical_overlap_attach(isingmc_classical *g, uint32_t ncopies);
/* The loop of isingmc_classical_pt_run with the overlap launch between the steps launch and the tempering launch of every round, one
 * synchronisation at the end.  q_out and ql_out: int32 [rounds][G][P][T], Q and QL; each of the four series may be NULL.  The
 * histograms always accumulate.  (isingmc_classical_pt_run on a handle with overlaps attached measures nothing and leaves the
 * histograms alone: that is how to thermalise.) */
int isingmc_classical_pt_run_overlaps(isingmc_classical *g, uint64_t rounds, uint64_t steps, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds,
                                      double *energy_out, int32_t *mag_out, int32_t *q_out, int32_t *ql_out);
/* read (either may be NULL), restore from a checkpoint (both non-NULL), zero */
int isingmc_classical_overlap_histograms(isingmc_classical *g, uint64_t *hq, uint64_t *hl);
int isingmc_classical_overlap_set_histograms(isingmc_classical *g, const uint64_t *hq, const uint64_t *hl);
int isingmc_classical_overlap_reset(isingmc_classical *g);
/* Host-only, a device-free test entry: isingmc_classical_host_pt_run with the measurement, by the sequential rule on the CPU and
 * with overlap_attach's argument checks.  q_out and ql_out as above; hq and hl are added to in place; all four may be NULL. */
int isingmc_classical_host_pt_run_overlaps(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint32_t ncopies, uint64_t rounds,
                                           uint64_t steps, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs,
                                           uint32_t *temp_of, uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts,
                                           double *energy_out, int32_t *mag_out, int32_t *q_out, int32_t *ql_out, uint64_t *hq, uint64_t *hl);

/* ---- isoenergetic cluster moves (Houdayer moves) between the copies of a group; the rule is stated once in csrc/classical_icm_rule.h ----
 * With a window t_first <= t < t_last of ladder indices attached, a round with cluster moves forms M = K / 2 disjoint pairs of copies in
 * every group (pair m is the copies (o + 2 m) mod K and (o + 2 m + 1) mod K, o = pt_step mod K) and, at every temperature of the window,
 * takes the two states that hold it, picks one of the variables in which they differ with one Philox draw (tag SSE_TAG_CLASSICAL_ICM),
 * and flips in both states the connected component of that variable among the differing variables, over the entries of the edge list
 * (any J).  The move is rejection-free and leaves E_A + E_B and both overlaps as they are.  It runs after the round's overlap
 * measurement and before its tempering step, so the E and M series of such a round hold the values after the moves.
 * Counts, uint64 [G][M][T] each, cumulative since attach or reset: moves, empty (the two states were equal) and size_sum (the sizes of
 * the flipped clusters added up); zero outside the window.
 * ISINGMC_EINVAL: overlaps (or tempering) not attached; t_last > T; an empty or reversed window; the other cluster-move calls before
 * icm_attach.  ISINGMC_ENOTIMPL: the three bit sets of one item exceed the LDS of a workgroup (the message names the largest N). */
/* Needs isingmc_classical_overlap_attach.  t_last == 0 means T; t_first == t_last == UINT32_MAX detaches.  Allocates and zeroes
 * the counts.  isingmc_classical_pt_attach and isingmc_classical_overlap_attach detach the cluster moves. */
int isingmc_classical_icm_attach(isingmc_classical *g, uint32_t t_first, uint32_t t_last);
/* the window as attached (either may be NULL) */
int isingmc_classical_icm_window(isingmc_classical *g, uint32_t *t_first, uint32_t *t_last);
/* The loop of isingmc_classical_pt_run_overlaps with the cluster-move launch in front of the tempering launch of every round.
 * measure != 0: the overlaps are measured as in pt_run_overlaps; measure == 0: they are not, and q_out and ql_out are ignored. */
int isingmc_classical_pt_run_icm(isingmc_classical *g, uint64_t rounds, uint64_t steps, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds,
                                 double *energy_out, int32_t *mag_out, int32_t *q_out, int32_t *ql_out, uint32_t measure);
/* read (each may be NULL), restore from a checkpoint (all non-NULL), zero */
int isingmc_classical_icm_counts(isingmc_classical *g, uint64_t *moves, uint64_t *empty, uint64_t *size_sum);
int isingmc_classical_icm_set_counts(isingmc_classical *g, const uint64_t *moves, const uint64_t *empty, const uint64_t *size_sum);
int isingmc_classical_icm_reset(isingmc_classical *g);
/* Host-only, device-free: the cluster-move launch of a model of nvars variables on a device whose workgroups have lds_bytes of LDS.
 * out[0] waves per workgroup (4, 2 or 1), out[1] the dynamic LDS in words, out[2] the words of one wave's area (three bit sets),
 * out[3] the most variables that launch takes at all.  isingmc_classical_icm_launch_plan: the same of an attached handle. */
int isingmc_classical_icm_plan(uint32_t nvars, uint32_t lds_bytes, uint32_t out[4]);
int isingmc_classical_icm_launch_plan(isingmc_classical *g, uint32_t out[4]);
/* For tests and A-B timing: run the cluster-move launch with fewer waves per workgroup than planned (1, 2 or 4, at most the plan's;
 * 0 restores the plan).  The moves do not depend on it. */
int isingmc_classical_icm_force_waves(isingmc_classical *g, uint32_t waves);
/* Host-only, a device-free test entry: isingmc_classical_host_pt_run_overlaps with cluster moves in the window [t_first, t_last) in
 * every round, by the sequential rule on the CPU and with icm_attach's argument checks.  measure as in pt_run_icm; moves, empty and
 * size_sum [G][M][T] are added to in place and may be NULL. */
int isingmc_classical_host_pt_run_icm(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint32_t ncopies, uint64_t rounds, uint64_t steps,
                                      uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                                      uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out,
                                      int32_t *q_out, int32_t *ql_out, uint64_t *hq, uint64_t *hl, uint32_t measure, uint32_t t_first, uint32_t t_last,
                                      uint64_t *moves, uint64_t *empty, uint64_t *size_sum);
/* Host-only, a device-free test entry: the cluster of one move.  state_a and state_b [N] bytes (of cfg's graph; its couplings are not
 * read); the seed is the rank-th variable, in increasing order, in which they differ.  mask_out [N]: 1 on the cluster; *size_out its
 * size.  ISINGMC_EINVAL when fewer than rank + 1 variables differ. */
int isingmc_classical_host_icm_cluster(const isingmc_classical_config *cfg, const uint8_t *state_a, const uint8_t *state_b, uint32_t rank, uint8_t *mask_out,
                                       uint32_t *size_out);

#ifdef __cplusplus
}
#endif
#endif /* ISINGMC_HIP_H */
