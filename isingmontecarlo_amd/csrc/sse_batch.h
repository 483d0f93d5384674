// sse_batch.h — the plain data that the host and every kernel share: the batch and argument structs, the bond record, what a launch
// runs (SSE_DO_*), how a kernel decodes bonds and keeps its tables (SSE_MODE_*), which passes it holds (SSE_PASSES_*) and the size
// limits.  No device code: host-only files may include it.
#pragma once
#include <stdint.h>

namespace sse {

struct BondRec {       // 16 B, one dwordx4 load (general table, any N / E)
    uint32_t a_info;   // var a | (kind|pref) << 29
    uint32_t c;        // second var or SSE_NO_VAR
    double w;          // weight when satisfied: 2|J|, Gamma, 2|h|
};
#define SSE_INFO_SHIFT 29
#define SSE_VAR_MASK 0x1FFFFFFFu
// compact edge entry (staged in LDS when N <= 32768): a | c << 15 | prefers_aligned << 30
#define SSE_CE_VAR_MASK 0x7FFFu
#define SSE_CE_MAX_VARS 32768u
#define SSE_MAX_CHUNKS 128u

struct DevBatch {
    uint32_t R, N, E, Nb, cap, nwords;
    uint32_t stride;      // words between the op-strings (and segment-id rows) of consecutive replicas: cap rounded up to
                          // a whole number of tiles, so that full-tile loads and stores never leave the row; slots >= cutoff hold 0
    uint32_t *ops;        // [R][cap]
    uint32_t *state;      // [R][nwords] bit v of word v>>5
    uint32_t *n, *ntrans, *cutoff, *err, *aux;  // [R]
    uint64_t *epoch;      // [R]
    uint64_t *acc;        // [acc_rows][8]
    const uint32_t *acc_row; // [R] accumulator row of each replica
    const BondRec *bonds; // [Nb]
    const uint32_t *edges_compact; // [E] or null
    const uint32_t *pm_signs; // [rows][pm_words]: bit e = edge e prefers aligned spins (J < 0), one row per bond-table row: the "+-J"
                          // decode (MODE >= 3) takes a bond's variables from the shared compact edge table and only its sign from here
    uint32_t pm_words;    // words per row of pm_signs = ceil(E / 32)
    const double *edge_w; // [E] 2|J|
    const double *cumw;   // [Nb] heat-bath cumulative weights
    double wtot;
    double wJ, gamma, wh; // uniform 2|J| (if uniformJ), Gamma, 2|h|
    uint32_t uniformJ, hpos, has_long;
    uint32_t *segs;       // [R][cap] segment ids of every slot's two legs (lo | hi << 16), written by the cluster build
    uint32_t *segs2;      // [R][stride] second id of each slot when the ids need 32 bits (HBM union-find); nullptr until such a launch is planned
                          // and read by the apply pass of the LDS union-find path (spends spare HBM bandwidth to
                          // avoid recomputing the ordered scan)
    uint32_t *chunks;     // [R][2*SSE_MAX_CHUNKS]: per chunk of CH slots: occupied count, transverse-op count
    uint32_t CH, nchunks; // chunk size (multiple of 256 slots) and number of chunks covering cap
    uint32_t *uf_scratch; // [R][W*N+cap (+bit arrays)] union-find fallback in HBM
    uint32_t *rvb_tbl;    // [R][rvb_tbl_words(N, E, cap)] the per-variable tables of RVB sweeps kept in HBM (SSE_PASSES_RVB_G, ISINGMC_CFG_RVB_GLOBAL_TABLES;
                          // null until the first such sweep).  This 8-byte slot used to be an unused pad word, and it still keeps the fields below
                          // at their offsets modulo 64: the register allocation of the general kernels depends on where these kernel arguments
                          // fall (without the word a dozen of them gain scalar or vector spills), and a field at the end would grow the
                          // workgroup-private copy of this struct that some kernels keep in scratch
    uint8_t *tbl;         // [R][tbl_stride] per-variable tables in HBM/L2 for models whose tables exceed LDS (MODE 2, see Tab)
    uint32_t tbl_stride;  // bytes per replica: Wmax*N*4 (scan records {rank, marker, touched} / spin bytes of the diagonal pass) + N, rounded up to 16
    uint32_t seed_lo, seed_hi, replica_offset;
    const uint32_t *rid;     // [R] or null: identity of the configuration held by each local replica = the `replica` word of its Philox
                             // counters (null: replica_offset + r).  Parallel tempering moves configurations between ranks at
                             // temperature-block boundaries; their random streams move with them
    const uint32_t *ham_row; // [R] or null: with per-replica couplings, the row of the bond tables a replica runs with (null: r).
                             // Tempering between different Hamiltonians: the row belongs to the temperature slot, not the configuration
    uint32_t lds_ufcap;   // ids that fit the LDS union-find arrays
    uint32_t lds_flipcap; // HBM union-find launches: ids whose flip BITS fit in LDS behind the fixed regions (0 = none): the apply pass
                          // then looks the two flips of every op up in LDS instead of in the parent array in HBM
    uint32_t lds_words;   // dynamic LDS words available to the workgroup
    const double *mats;   // generic interactions (Qmc, qmc_runner.rs:415-680): [Nb][16] weights indexed in | out<<2; NULL = Ising bonds
    uint32_t bond_stride; // 0, or Nb when every replica has its own bond table / cumulative weights (per-replica couplings)
    const double *wtot_r; // [R] per-replica total weight (bond_stride != 0)
    const uint32_t *adj_start, *adj; // [N+1], [2E] bonds_for_var (make_classical_bonds, qmc_ising.rs:421-432)
    // deferred cluster flips (sse_cluster.hip.h -> sse_fast.hip.h): instead of rewriting the op-string, the cluster update leaves one
    // byte per slot — the xor mask of the word's four state bits — and the diagonal pass of the next timestep applies it while it
    // streams the string anyway (the apply pass was bound by its 10 B/slot of memory traffic).  pend[r] = 1: replica r's string
    // in HBM is still the one BEFORE the flips; every other consumer of the strings goes through materialize_kernel first.
    uint8_t *flipb;       // [R][stride] or null
    uint32_t *pend;       // [R]
    uint32_t rvb_growers; // RVB: attempts grown side by side (0 = one at a time on wave 0)
    uint32_t *rvb_prod;   // [R][rvb_prod_cap][SSE_RVB_PROD_STRIDE] growth products of a sweep's attempts (sse_rvb_split.hip.h); null until an RVB sweep is planned
    uint32_t rvb_prod_cap; // attempts per replica that rvb_prod holds
    uint32_t rvb_prod_stride; // words per attempt in rvb_prod
    uint32_t dbg_flags;   // diagnostic builds only
    unsigned long long *dbg; // [R][16] phase durations in 10-ns ticks (diagnostic builds only, -DSSE_PHASE_TIMING); every build: words 11 and 15, the cluster kernel's parked unions and full-queue drains
};

// which primitives a launch runs per step
#define SSE_DO_DIAG 1u
#define SSE_DO_LOOP 2u
#define SSE_DO_CLUSTER 4u
#define SSE_DO_FREE 8u
#define SSE_DO_GROW 16u
#define SSE_DO_HEATBATH 32u
#define SSE_DO_RVB 64u

struct SweepArgs {
    const double *beta; // [R]
    uint64_t nsteps;
    uint64_t step0;     // index of the first step of this launch within the caller's timesteps() call
    uint32_t sampling_freq; // 0 = never sample
    uint32_t domask;
    double prob;
    uint32_t rvb_updates; // RVB attempts per step (0 = (N+1)/2, qmc_ising.rs:711)
    uint32_t *out_u32; // optional per-replica output (n_clusters / loop length / RVB successes) of the LAST step
    uint32_t only_flagged; // 1 = run only the replicas flagged in DevBatch::aux (left over by sse::cluster_kernel) and clear their flags
    uint32_t defer_flips;  // sse::cluster_kernel: leave the flips as one byte per slot (DevBatch::flipb) instead of applying them;
                           // sse::sweep_fast_kernel: apply the pending flip bytes of a replica while loading its string
};

// DevBatch::err[r]: why replica r stopped (0 = it did not; sticky until isingmc_clear_errors).  The kernels set these, check_errors()
// (driver.hip) turns them into return codes and messages.  4 was never used.
enum SseErr : uint32_t {
    SSE_ERR_CAPACITY = 1,   // cutoff n + n/2 exceeds the op-string capacity
    SSE_ERR_COUNT = 2,      // directed loop: n disagrees with the op-string
    SSE_ERR_LOOP_OPEN = 3,  // directed loop still open at its vertex bound
    SSE_ERR_RVB_LDS = 5,    // RVB: the launch's LDS does not hold the fixed scratch
    SSE_ERR_RVB_TABLE = 6,  // RVB: the constant-op table does not fit in LDS
    SSE_ERR_RVB_SETS = 7,   // RVB: a cluster's sets outgrew their LDS areas
    SSE_ERR_SCAN_RANGE = 8, // cluster scan: more than 65534 transverse ops inside one wave's range
};

// MODE of a kernel: how bonds are decoded and where the per-variable tables live
// (3 / 4: the "+-J" decode — every replica its own coupling SIGNS on a shared graph with uniform |J| and fields: a bond's variables
// come from the shared compact edge table in global memory (L2-resident), its sign from a per-replica bit array in LDS, its weight
// from three scalars; nothing per replica is fetched from HBM to decode an op.  3 = per-variable tables in LDS (diagonal launches
// only), 4 = in HBM like mode 2)
enum { SSE_MODE_GENERAL = 0, SSE_MODE_LDS_EDGES = 1, SSE_MODE_GLOBAL_TABLES = 2, SSE_MODE_PM_LDS_TABLES = 3, SSE_MODE_PM_GLOBAL_TABLES = 4 };

enum { SSE_PASSES_ALL = 0, SSE_PASSES_DIAG = 1, SSE_PASSES_OFFDIAG = 2, SSE_PASSES_RVB = 3, SSE_PASSES_RVB_G = 4 }; // DIAG: diagonal pass + directed loop; OFFDIAG: cluster + free spins + sampling; RVB: the RVB sweep alone (its own register budget)
// RVB_G: the RVB sweep alone with its per-variable tables in HBM (DevBatch::rvb_tbl) on any model: only the bit arrays of the Lds carve (as MODE 2) and the fixed
// RVB scratch stay in LDS (sweep_rvb_global.hip: W = 16, K = 4, MODE 1 or 0 = the LDS edge table or the general bond records)

} // namespace sse
