// driver.hip — the sweep driver behind the five single updates and isingmc_timesteps: prepare() once per call, plan_step() for the
// launches of a timestep, run() walks them in one loop; check_errors() reads the replicas' error codes back.
#include "batch.hip.h"
#include "sse_launch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

using namespace sse;

// Deferred cluster flips (sse_cluster.hip.h) applied in place: ops[p] ^= flip byte, for the replicas whose flag is set.  Used by
// every consumer of the op-strings other than the trimmed diagonal kernel, which applies the bytes itself while it streams.
__global__ __launch_bounds__(1024) void materialize_kernel(DevBatch B) {
    const uint32_t r = blockIdx.x;
    if (!B.pend[r]) return; // (uniform per workgroup)
    uint32_t *ops = B.ops + (size_t)r * B.stride;
    const uint8_t *fb = B.flipb + (size_t)r * B.stride;
    const uint32_t M = B.cutoff[r];
    for (uint32_t p = threadIdx.x; p < M; p += blockDim.x) { const uint32_t f = fb[p]; if (f) ops[p] ^= f; }
    __syncthreads();
    if (threadIdx.x == 0) B.pend[r] = 0u;
}
int sse::ensure_materialized(isingmc_batch *b) {
    if (!b->pending) return ISINGMC_OK;
    hipLaunchKernelGGL(materialize_kernel, dim3(b->dev.R), dim3(1024), 0, b->stream, b->dev);
    HIP_TRY(b, hipGetLastError());
    HIP_TRY(b, hipStreamSynchronize(b->stream)); // (callers read the strings with blocking copies or their own kernels on this stream; keep it simple)
    b->pending = false;
    return ISINGMC_OK;
}

// a launch and the DevBatch it is given: the LDS it asks for and the LDS its kernel sees (DevBatch::lds_words), from one word count
static void give_lds(LaunchCfg &c, DevBatch &d, size_t words) {
    c.lds_bytes = lds_bytes_of(words);
    d.lds_words = (uint32_t)(c.lds_bytes / 4);
}

static void size_lds(isingmc_batch *b) {
    const LdsPlan p = plan_lds(b, b->W);
    b->dev.lds_ufcap = p.ufcap;
    b->lds_words = p.words;
}

// LDS plan of the dedicated cluster kernel (sse_cluster.hip.h): 16 waves, packed per-wave tables, 16-bit parents for
// 16 N + (transverse ops seen so far + headroom) ids.  ok = false: the ids do not fit (the general kernel takes the launch);
// also when the largest id count the kernel would accept under that cap (want - 1) is not its case (cl_ids_fit: few
// variables and many cuts, whose flip bits would overrun the per-wave tables).
struct LeanPlan { bool ok; uint32_t ufcap; size_t words; };
static LeanPlan plan_lean(const isingmc_batch *b) {
    const DevBatch &D = b->dev;
    LeanPlan p{false, 0u, 0};
    if (!b->lean_cluster) return p;
    const size_t ids_max = (size_t)16 * D.N + D.cap;
    size_t want = uf_ids_wanted(lds_needs(b), 16);
    if (want > ids_max) want = ids_max;
    if (want > 65535 || !cluster_ids_fit(D.N, (uint32_t)want - 1u, (uint32_t)want)) return p;
    const size_t words = cluster_lds_words(D.N, D.nwords, D.Nb, (uint32_t)want, D.has_long != 0u);
    if (words > b->lds_total_words) return p;
    p.ok = true; p.ufcap = (uint32_t)want; p.words = words;
    return p;
}

// The device error codes (SseErr) as the caller sees them: the return value, and the message made from the replica and one more number
// (the capacity for SSE_ERR_CAPACITY, the code itself for every other).  A code without a row of its own is an integrity error.
struct DeviceError { uint32_t code; int rc; const char *fmt; };
static const DeviceError DEVICE_ERRORS[] = {
    {SSE_ERR_CAPACITY, ISINGMC_ECAPACITY, "replica %u: cutoff n + n/2 exceeds the op-string capacity %u"},
    {SSE_ERR_SCAN_RANGE, ISINGMC_ECAPACITY, "replica %u: more than 65534 transverse ops inside one wave's range of the cluster scan; raise waves_per_replica"},
    {SSE_ERR_RVB_LDS, ISINGMC_ECAPACITY, "replica %u: RVB working set exceeds the LDS scratch (code %u)"},
    {SSE_ERR_RVB_TABLE, ISINGMC_ECAPACITY, "replica %u: RVB working set exceeds the LDS scratch (code %u)"},
    {SSE_ERR_RVB_SETS, ISINGMC_ECAPACITY, "replica %u: RVB working set exceeds the LDS scratch (code %u)"},
    {SSE_ERR_LOOP_OPEN, ISINGMC_ELIMIT, "replica %u: directed loop still open after 64*cutoff+1024 vertices (the reference has no bound; "
                                        "clear with isingmc_clear_errors and continue)"},
    {0u, ISINGMC_EINTEGRITY, "replica %u: device integrity error %u"}, // (every other code; SSE_ERR_COUNT among them)
};
static int check_errors(isingmc_batch *b) {
    std::vector<uint32_t> err(b->dev.R), ntr(b->dev.R);
    HIP_TRY(b, hipMemcpyAsync(err.data(), b->dev.err, sizeof(uint32_t) * b->dev.R, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipMemcpyAsync(ntr.data(), b->dev.ntrans, sizeof(uint32_t) * b->dev.R, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    for (uint32_t r = 0; r < b->dev.R; ++r) if (ntr[r] > b->max_ntrans) b->max_ntrans = ntr[r];
    for (uint32_t r = 0; r < b->dev.R; ++r)
        if (err[r]) {
            const DeviceError *e = DEVICE_ERRORS;
            while (e->code && e->code != err[r]) ++e;
            char buf[160];
            snprintf(buf, sizeof buf, e->fmt, r, e->code == SSE_ERR_CAPACITY ? b->dev.cap : err[r]);
            b->err = buf;
            return e->rc;
        }
    return ISINGMC_OK;
}

// ---- The sweep driver: prepare() once per call, plan_step() for the launches of a timestep, run() walks them in one loop ----
// One kernel launch of a timestep as a value: plan_step() lists them in order, issue() makes its DevBatch and SweepArgs and dispatches it.
enum LaunchKind : uint8_t {
    L_SWEEP, L_FAST_DIAG, // the general kernel of cfg.W waves and cfg.passes; the trimmed diagonal kernel (sse_fast.hip.h)
    L_CLUSTER,            // the dedicated cluster kernel (sse_cluster.hip.h); an only_flagged L_SWEEP follows for the replicas it flagged
    L_RVB_FUSED, L_RVB_GROW, L_RVB_MAIN, L_RVB_GLOBAL, // the RVB sweep: in the general kernel; growth, then main launch (sse_rvb_split.hip.h); tables in HBM
};
enum Bucket : uint8_t { B_DIAG = 0, B_OTHER = 1, B_RVB = 2 }; // index into pass_ms / pass_launches; an RVB launch counts under B_OTHER too
struct Launch {
    LaunchKind kind;
    Bucket bucket;
    bool sampled;      // carries the call's sampling_freq / out_u32 (and runs on a sampled step even with an empty domask)
    bool only_flagged; // SweepArgs::only_flagged
    bool follows;      // second kernel of the launch before it: counted and timed with that one
    uint32_t domask, ufcap, flipcap; // its passes; DevBatch::lds_ufcap and lds_flipcap
    size_t words;      // its dynamic LDS
    LaunchCfg cfg;     // (lds_bytes: filled in by issue())
};
struct Plan {
    Launch l[5];    // (at most: diagonal, RVB growth + main, cluster + its follow-up)
    uint32_t n;
    bool replan;    // a split call without RVB sweeps: planned again every REPLAN_EVERY steps, from the transverse-op counts seen by then
    bool lean;      // the dedicated cluster kernel would take a cluster launch (reported as last_lean whether or not one follows)
    uint32_t W_off; // waves chosen for the off-diagonal launches (reported as last_W_off), 0 = no choice made
};
struct Call { // what a call asks for, fixed by prepare()
    SweepArgs A;          // passes, sampling and outputs of the whole call; issue() narrows them per launch
    uint64_t nsteps, chunk; // chunk: steps per walk through the plan (1, or the steps of a fused launch)
    uint32_t phase;
    bool split;           // a diagonal launch and the rest per timestep, instead of whole timesteps per launch
    bool recording;       // a sample record is attached and the call samples
};
constexpr size_t MAX_TIMED = 256; // steps of a split call whose launches carry events
constexpr uint64_t REPLAN_EVERY = 16;
static bool rvb_alone(uint32_t m) { return (m & ~SSE_DO_GROW) == SSE_DO_RVB; }
// whole timesteps per launch around an RVB sweep with its tables in HBM, which needs a launch of its own
static bool fused_around_rvb_g(const isingmc_batch *b, const Call &c) { return !c.split && (c.A.domask & SSE_DO_RVB) && b->rvb_global && !rvb_alone(c.A.domask); }
// the RVB sweep of a split timestep is a launch of its own unless a directed loop runs too (then both stay in the all-passes
// second launch; with the tables in HBM there is no such kernel and the sweep is split out all the same)
static bool split_rvb_own_launch(const isingmc_batch *b, uint32_t m) { return (m & SSE_DO_RVB) && (!(m & SSE_DO_LOOP) || b->rvb_global); }
static uint32_t rvb_attempts(const isingmc_batch *b) { return b->rvb_updates ? b->rvb_updates : (b->dev.N + 1u) / 2u; }
// Does the dedicated cluster kernel take a launch of these passes?  Its plan fits, K is one of its two, no test limit on the
// ids, cluster with or without free spins and nothing else, one step per launch.
static bool lean_takes(const isingmc_batch *b, const LeanPlan &lean, uint32_t mask, bool one_step) {
    return lean.ok && (b->K == 4 || b->K == 2) && !b->uf_ids_limit && (mask & SSE_DO_CLUSTER) && !(mask & ~(SSE_DO_CLUSTER | SSE_DO_FREE)) && one_step;
}

// Once per call: argument checks, the beta upload, pending flips, every allocation.  The step loop allocates and frees nothing.
static int prepare(isingmc_batch *b, const double *beta, uint64_t nsteps, uint32_t freq, uint32_t domask, double prob, uint32_t *out_host, Call &c) {
    HIP_TRY(b, hipSetDevice(b->device));
    SweepArgs &A = c.A;
    if (beta) {
        for (uint32_t r = 0; r < b->dev.R; ++r)
            if (!(beta[r] >= 0.0) || !std::isfinite(beta[r])) { b->err = "beta must be finite and >= 0"; return ISINGMC_EINVAL; }
        HIP_TRY(b, hipMemcpyAsync(b->d_beta, beta, sizeof(double) * b->dev.R, hipMemcpyHostToDevice, b->stream));
        A.beta = b->d_beta;
    } else if (b->beta_dev) A.beta = b->beta_dev;
    else if (domask & SSE_DO_DIAG) { b->err = "beta is required for a diagonal update"; return ISINGMC_EINVAL; }
    if ((domask & SSE_DO_RVB) && b->generic) { b->err = "RVB updates are Ising-specific: not available with generic interactions"; return ISINGMC_ENOTIMPL; }
    if ((domask & SSE_DO_CLUSTER) && b->generic && !b->generic_sym) { b->err = "Cannot perform cluster updates on graphs that break ising symmetry."; return ISINGMC_ENOTIMPL; } // qmc_runner.rs:224-226
    if ((domask & SSE_DO_RVB) && is_tg(b) && !b->rvb_global) { b->err = "RVB updates keep their working set in LDS: not available for models whose per-variable tables live in HBM (set ISINGMC_CFG_RVB_GLOBAL_TABLES)"; return ISINGMC_ENOTIMPL; }
    A.sampling_freq = freq; A.domask = domask & 0xFFFFu; A.prob = prob; A.rvb_updates = b->rvb_updates;
    A.out_u32 = out_host ? b->d_out : nullptr;
    c.nsteps = nsteps; c.phase = (domask >> 16) & 1u;
    c.split = !b->fused_launch && (domask & SSE_DO_DIAG);
    c.recording = b->rec && freq; // (freq != 0: timesteps; single updates sample nothing)
    c.chunk = (c.split || fused_around_rvb_g(b, c)) ? 1 : (b->steps_per_launch && b->steps_per_launch < nsteps ? b->steps_per_launch : nsteps);
    const bool rvb_g = (domask & SSE_DO_RVB) && b->rvb_global;
    if (rvb_g && !b->dev.rvb_tbl) { // the per-replica table scratch of RVB_G launches, on the first one (no fall-back when it cannot be had)
        const size_t words = rvb_tbl_words(b->dev);
        if (words > 0xFFFFFFFFull) { b->err = "RVB table scratch: more than 2^32 words per replica"; return ISINGMC_ECAPACITY; }
        if (b->rvb_tbl.alloc((size_t)b->dev.R * words * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            char buf[160];
            snprintf(buf, sizeof buf, "RVB table scratch (ISINGMC_CFG_RVB_GLOBAL_TABLES): hipMalloc of %zu bytes failed", (size_t)b->dev.R * words * sizeof(uint32_t));
            b->err = buf;
            return ISINGMC_ENODEVICE;
        }
        b->dev.rvb_tbl = b->rvb_tbl.as<uint32_t>();
    }
    if (rvb_g && rvb_global_lds_words(b->dev, lds_edges(b), 0) > b->lds_total_words) { b->err = "RVB scratch (ISINGMC_CFG_RVB_GLOBAL_TABLES): the spin-state bit arrays and the fixed RVB regions exceed LDS"; return ISINGMC_ENOTIMPL; }
    if (domask & SSE_DO_RVB) b->last_rvb_global = false;
    // Pending cluster flips: only a call whose first launch is the trimmed diagonal kernel may start on the un-flipped strings
    const bool first_is_fast_diag = c.split && b->fast_diag && !(domask & SSE_DO_HEATBATH) && b->defer;
    if (b->pending && !first_is_fast_diag) { const int rcm = ensure_materialized(b); if (rcm) return rcm; }
    size_lds(b);
    if (!b->dev.segs2 && (domask & SSE_DO_CLUSTER) && !plan_lds(b, b->W_off ? b->W_off : b->W).all_ids_fit) {
        // the cluster ids of (some) replicas need the 32-bit union-find in HBM: room for the second id of every slot
        if (const int rc2 = dalloc(b, &b->dev.segs2, (size_t)b->dev.R * b->dev.stride, false)) return rc2;
    }
    b->pass_ms[0] = b->pass_ms[1] = b->pass_ms[2] = 0.f;
    b->pass_launches[0] = b->pass_launches[1] = b->pass_launches[2] = 0;
    // records of a sweep's attempts, for an RVB sweep as a growth and a main launch (the attempt count is fixed for the call)
    const uint32_t updates = rvb_attempts(b);
    const size_t pstride = rvb_split_prod_stride(b->dev.Nb);
    const bool rvb_own_launch = c.split ? split_rvb_own_launch(b, A.domask) : rvb_alone(A.domask);
    if (rvb_own_launch && !b->rvb_global && b->rvb_split && c.chunk == 1 && pstride && b->dev.rvb_prod_cap < updates) {
        // (more attempts than rvb_prod_cap are more bytes than the block has: it grows)
        if (b->rvb_prod.reserve((size_t)b->dev.R * updates * pstride * sizeof(uint32_t), b->stream) == hipSuccess) { b->dev.rvb_prod_cap = updates; b->dev.rvb_prod_stride = (uint32_t)pstride; }
        else { (void)hipGetLastError(); b->dev.rvb_prod_cap = 0; b->rvb_split = false; } // no room for the records: the fused kernel from now on
        b->dev.rvb_prod = b->rvb_prod.as<uint32_t>();
    }
    const size_t want_ev = c.split ? 4 * (size_t)(c.nsteps < MAX_TIMED ? c.nsteps : MAX_TIMED) : 0;
    while (b->evpool.size() < want_ev) { hipEvent_t ev; HIP_TRY(b, hipEventCreate(&ev)); b->evpool.push_back(ev); }
    return ISINGMC_OK;
}

// Kernel and geometry of the launch that carries a call's off-diagonal work: all of a fused call, what follows the diagonal launch
// of a split one.  `base` is the all-passes launch in the batch's own geometry.
static Launch plan_off(const isingmc_batch *b, const Call &c, const Launch &base, uint32_t *W_chosen) {
    const uint32_t m = c.A.domask;
    Launch o = base;
    if ((c.split || rvb_alone(m)) && (m & SSE_DO_RVB) && !b->W_off && b->W < 16) {
        // RVB sweeps: the cooperative window scans of an attempt cover 4x more slots per step with 16 waves (the
        // sequential lane does not care); taken when the cluster tables of that geometry fit as well
        const LdsPlan p16 = plan_lds(b, 16);
        if (p16.all_ids_fit) {
            const size_t words = std::min(rvb_lds_words(16, b->dev, lds_edges(b), false, 0u), b->lds_total_words);
            *W_chosen = o.cfg.W = 16; o.ufcap = p16.ufcap; o.words = std::max(words, p16.words);
        }
    }
    // launches without a diagonal or RVB pass use the kernel that leaves that code out
    const bool loop_only = (m & (SSE_DO_DIAG | SSE_DO_RVB | SSE_DO_CLUSTER | SSE_DO_FREE)) == 0 && (m & SSE_DO_LOOP);
    if (rvb_alone(m)) o.cfg.passes = SSE_PASSES_RVB;   // the RVB sweep alone: its own kernel (no scratch spills, unlike the all-passes kernel)
    else if (loop_only) o.cfg.passes = SSE_PASSES_DIAG; // a lone directed loop uses the small launch geometry too
    else if (!(m & (SSE_DO_DIAG | SSE_DO_RVB | SSE_DO_LOOP)) || (c.split && !(m & SSE_DO_RVB))) o.cfg.passes = SSE_PASSES_OFFDIAG;
    if (o.cfg.passes != SSE_PASSES_OFFDIAG) return o;
    // The off-diagonal kernel is latency-bound and small in registers: more waves per replica help as long as the
    // per-wave scan tables and the union-find of W*N + (transverse ops) ids still fit in LDS.  Decided from the largest
    // transverse-op count seen so far, and again every few timesteps of a long call (the count grows while a batch
    // equilibrates; replicas that outgrow the table only fall back to the slower HBM union-find, never fail).
    uint32_t Wo = b->W_off ? b->W_off : b->W;
    bool hbm_uf = false;
    if (!b->W_off && b->W < 16) {
        if (plan_lds(b, 16).all_ids_fit) Wo = 16;
        else if (b->w8_ok && !b->uf_ids_limit && !plan_lds(b, b->W).all_ids_fit) {
            // the largest replicas need the 32-bit union-find in HBM whatever the geometry: spend the LDS on the scan
            // tables of 8 waves instead of on a 16-bit parent table that they cannot use (the HBM path is bound by
            // memory latency: twice the waves, twice the accesses in flight)
            Wo = 8; hbm_uf = true;
        }
    }
    LdsPlan po = plan_lds(b, Wo);
    if (hbm_uf) { po.ufcap = 0; po.words = general_lds_words(Wo, b->dev, lds_edges(b), false, 0u, 0u) + 64; }
    *W_chosen = o.cfg.W = Wo; o.ufcap = po.ufcap; o.flipcap = 0u; o.words = po.words;
    if (is_tg(b) || hbm_uf) {
        // HBM union-find launch: the LDS behind the fixed regions takes the flip bits of the ids (those the union-find is sized
        // for; a replica with more ids looks its flips up in HBM as before)
        const size_t used = lds_bytes_of(po.words) / 4;
        const size_t want = (uf_ids_wanted(lds_needs(b), Wo) + 31) / 32;
        const size_t avail = b->lds_total_words > used + 16 ? b->lds_total_words - used - 16 : 0;
        const size_t fw = want < avail ? want : avail;
        o.words = used + fw; o.flipcap = (uint32_t)(32 * fw);
    }
    return o;
}

// The RVB sweep as a launch of its own, in one of its three forms.  r: the launch of the fused kernel (SSE_PASSES_RVB).
static void add_rvb(Plan &P, const isingmc_batch *b, Launch r, bool one_step) {
    const DevBatch &D = b->dev;
    r.domask = SSE_DO_RVB;
    const bool records = !b->rvb_global && b->rvb_split && one_step && D.rvb_prod && D.rvb_prod_cap >= rvb_attempts(b);
    const size_t main_words = records ? rvb_main_lds_words(b->rvb_main_W, D, lds_edges(b)) : 0;
    if (b->rvb_global) { // the tables in HBM (sweep_rvb_global.hip): 16 waves, the LDS scratch without the per-variable tables + one small growth area per wave
        r.kind = L_RVB_GLOBAL; r.ufcap = D.lds_ufcap; r.flipcap = 0u;
        r.cfg.W = 16; r.cfg.K = 4; r.cfg.passes = SSE_PASSES_RVB_G; r.cfg.mode = b->mode == SSE_MODE_LDS_EDGES ? SSE_MODE_LDS_EDGES : SSE_MODE_GENERAL;
        r.words = std::min(rvb_global_lds_words(b->dev, lds_edges(b), 16), b->lds_total_words); // (fewer small growth areas; the large one always fits)
    } else if (records && lds_bytes_of(main_words) <= b->lds_total_words * 4) { // growth launch + main launch (sse_rvb_split.hip.h)
        r.kind = L_RVB_GROW; r.cfg.W = 16; r.ufcap = D.lds_ufcap; r.flipcap = 0u;
        r.words = std::min((size_t)rvb_grow_table_start(D, lds_edges(b)) + D.cap + 16 * 640, b->lds_total_words); // the constant-op table, 16 small growth areas
        P.l[P.n++] = r;
        r.kind = L_RVB_MAIN; r.follows = true; r.cfg.W = b->rvb_main_W; r.words = main_words;
    } else r.kind = L_RVB_FUSED;
    P.l[P.n++] = r;
}
// Cluster / free-spin / sampling passes in launch `L`, or in the dedicated cluster kernel when it takes them: then the general
// kernel follows for the replicas it flagged (ids beyond its LDS union-find, no op, no cut: a handful while a batch equilibrates,
// none afterwards; that launch runs in the small diagonal geometry and its workgroups leave at once when their flag is clear).
static void add_offdiag(Plan &P, const isingmc_batch *b, const LeanPlan &lean, Launch L, uint32_t mask, bool one_step) {
    L.domask = mask; L.sampled = true;
    if (lean_takes(b, lean, mask, one_step)) {
        Launch cl = L;
        cl.kind = L_CLUSTER; cl.cfg.W = 16; cl.ufcap = lean.ufcap; cl.flipcap = 0u; cl.words = lean.words;
        P.l[P.n++] = cl;
        const LdsPlan pf = plan_lds(b, b->W);
        L.follows = L.only_flagged = true; L.cfg.W = b->W; L.cfg.passes = SSE_PASSES_OFFDIAG;
        L.ufcap = pf.ufcap; L.flipcap = 0u; L.words = pf.words;
    }
    P.l[P.n++] = L;
}

// The launches of one timestep (of one chunk of timesteps on the fused path), in order.  Reads the batch and the call; changes nothing.
static Plan plan_step(const isingmc_batch *b, const Call &c) {
    Plan P{};
    const uint32_t m = c.A.domask;
    Launch base{};
    base.kind = L_SWEEP; base.bucket = B_OTHER; base.ufcap = b->dev.lds_ufcap;
    base.cfg.W = b->W; base.cfg.K = b->K; base.cfg.mode = b->mode; base.cfg.phase = c.phase; base.cfg.passes = SSE_PASSES_ALL; base.cfg.stream = b->stream;
    base.words = ((m & SSE_DO_RVB) && b->lds_words_rvb > b->lds_words) ? b->lds_words_rvb : b->lds_words;
    const Launch off = plan_off(b, c, base, &P.W_off);
    const LeanPlan lean = plan_lean(b);
    P.lean = lean_takes(b, lean, SSE_DO_CLUSTER, true);
    P.replan = c.split && off.cfg.passes == SSE_PASSES_OFFDIAG;
    if (fused_around_rvb_g(b, c)) {
        // per step, the passes in front of the sweep, the sweep, the passes behind it (the kernel's order: same epochs, same results),
        // in the batch's own geometry and the all-passes kernel
        const uint32_t pre = m & (SSE_DO_DIAG | SSE_DO_HEATBATH | SSE_DO_GROW), post = m & ~(pre | SSE_DO_RVB);
        if (pre & SSE_DO_DIAG) { P.l[P.n] = off; P.l[P.n++].domask = pre; }
        add_rvb(P, b, off, true);
        P.l[P.n] = off; P.l[P.n].domask = post; P.l[P.n++].sampled = true;
    } else if (!c.split) {
        if (rvb_alone(m)) { Launch r = off; r.sampled = true; add_rvb(P, b, r, c.chunk == 1); } // (sampled: isingmc_rvb_update's successes)
        else add_offdiag(P, b, lean, off, m, c.chunk == 1);
    } else {
        // Two launches per timestep: the diagonal pass as its own kernel (twice the occupancy: it needs neither the
        // union-find LDS nor the registers of the cluster scan), then everything else.  Same Philox epochs, same
        // results as the fused launch; n / cutoff / chunk counters go through HBM in between (a few KB per replica).
        // The first launch takes the diagonal pass and, unless an RVB sweep has to come in between, the directed loop (one
        // sequential walk: it gains nothing from the wider off-diagonal geometry)
        const uint32_t diag_bits = SSE_DO_DIAG | SSE_DO_HEATBATH | SSE_DO_GROW | ((m & SSE_DO_RVB) ? 0u : SSE_DO_LOOP);
        const bool use_fast = b->fast_diag && !(m & SSE_DO_HEATBATH);
        Launch d = base;
        d.kind = use_fast ? L_FAST_DIAG : L_SWEEP; d.bucket = B_DIAG; d.domask = m & diag_bits; d.cfg.passes = SSE_PASSES_DIAG;
        // the diagonal launch needs the fixed regions up to the per-wave tables, which it uses as [W][N] bytes
        d.words = use_fast ? b->lds_words_fast : b->lds_words_diag;
        if (is_pm(b) && b->lds_words_pm_diag) { d.cfg.mode = SSE_MODE_PM_LDS_TABLES; d.words = b->lds_words_pm_diag; } // (the cluster tables stay in HBM)
        P.l[P.n++] = d;
        uint32_t rest = m & ~diag_bits;
        Launch second = off;
        if (split_rvb_own_launch(b, rest)) {
            // the RVB sweep as its own launch (register budget of its own: the all-passes kernel spills to scratch), then the
            // cluster / free-spin launch: the plain off-diagonal kernel in the same geometry (with a directed loop — only behind an
            // RVB_G launch — the kernel of every pass, as without the RVB launch)
            Launch r = off; r.bucket = B_RVB; r.cfg.passes = SSE_PASSES_RVB; add_rvb(P, b, r, true);
            rest &= ~SSE_DO_RVB;
            if (!(rest & SSE_DO_LOOP)) {
                const LdsPlan po = plan_lds(b, off.cfg.W);
                second.cfg.passes = SSE_PASSES_OFFDIAG; second.ufcap = po.ufcap; second.flipcap = 0u; second.words = po.words;
            }
        }
        add_offdiag(P, b, lean, second, rest, true);
    }
    return P;
}

static void report_plan(isingmc_batch *b, const Plan &P) { b->last_lean = P.lean; if (P.W_off) b->last_W_off = P.W_off; }
static hipError_t launch_sweep(const LaunchCfg &c, const DevBatch &dev, const SweepArgs &a) {
    static constexpr decltype(&launch_sweep_w1) of_waves[5] = {launch_sweep_w1, launch_sweep_w4, launch_sweep_w6, launch_sweep_w8, launch_sweep_w16}; // (by wave_index)
    const int i = wave_index(c.W);
    return i < 0 ? hipErrorInvalidValue : of_waves[i](c, dev, a);
}
// Launch L for `steps` timesteps from step0: the one place where a launch's DevBatch and SweepArgs are made
static hipError_t issue(isingmc_batch *b, const Call &c, const Launch &L, uint64_t step0, uint64_t steps) {
    LaunchCfg cfg = L.cfg; DevBatch d = b->dev;
    d.lds_ufcap = L.ufcap; d.lds_flipcap = L.flipcap; give_lds(cfg, d, L.words);
    SweepArgs a = c.A;
    a.domask = L.domask; a.nsteps = steps; a.step0 = step0; a.only_flagged = L.only_flagged ? 1u : 0u;
    if (!L.sampled) { a.sampling_freq = 0; a.out_u32 = nullptr; }
    switch (L.kind) {
    case L_SWEEP: return launch_sweep(cfg, d, a);
    case L_FAST_DIAG: // (every step of a run after the first: the cluster update of the step before left flip bytes)
        if (b->pending && b->defer) { a.defer_flips = 1u; b->pending = false; }
        return launch_sweep_fast(cfg, d, a);
    case L_CLUSTER: {
        a.defer_flips = b->defer ? 1u : 0u;
        const hipError_t e = launch_cluster(cfg, d, a);
        if (e == hipSuccess && b->defer) b->pending = true;
        return e;
    }
    case L_RVB_FUSED: b->last_rvb_split = false; return launch_sweep(cfg, d, a);
    case L_RVB_GROW: b->last_rvb_split = false; return launch_rvb_grow(cfg, d, a);
    case L_RVB_MAIN: b->last_rvb_split = true; return launch_rvb_main(cfg, d, a);
    case L_RVB_GLOBAL: b->last_rvb_split = false; b->last_rvb_global = true; return launch_rvb_global(cfg, d, a);
    }
    return hipErrorInvalidValue;
}

static int run(isingmc_batch *b, const double *beta, uint64_t nsteps, uint32_t freq, uint32_t domask, double prob, uint32_t *out_host) {
    if (!b) return ISINGMC_EINVAL;
    Call c{};
    int rc = prepare(b, beta, nsteps, freq, domask, prob, out_host, c);
    if (rc) return rc;
    Plan P = plan_step(b, c); report_plan(b, P);
    HIP_TRY(b, hipEventRecord(b->ev0, b->stream));
    size_t timed_steps = 0;
    for (uint64_t done = 0, len = 0; done < nsteps; done += len) {
        if (P.replan && done && done % REPLAN_EVERY == 0) {
            if ((rc = check_errors(b))) return rc; // drains the stream, refreshes max_ntrans; an error ends the call here
            P = plan_step(b, c); report_plan(b, P);
        }
        len = std::min(c.chunk, nsteps - done);
        // with a sample record attached a launch ends on the next sampled step, whose state the record takes (same epochs, same results)
        if (c.recording && len > freq - done % freq) len = freq - done % freq;
        const bool sample = freq && (done + len) % freq == 0;
        // flip bytes left by the cluster update of the step before: the trimmed diagonal kernel applies them, any other needs them applied
        if (b->pending && c.split && !(P.l[0].kind == L_FAST_DIAG && b->defer)) { rc = ensure_materialized(b); if (rc) return rc; }
        // events of a timed step: [0] in front of the diagonal launch, [1] behind it, [2] behind the RVB sweep (= [1] without one), [3] at the end
        hipEvent_t *ev = (c.split && done < MAX_TIMED) ? &b->evpool[4 * done] : nullptr;
        uint32_t stage = 0;
        for (uint32_t i = 0; i < P.n; ++i) {
            const Launch &L = P.l[i];
            if (!L.domask && !sample) continue; // nothing to run behind the other launches and nothing to sample
            constexpr uint32_t events_before[3] = {1u, 3u, 2u}; // by bucket
            if (ev) while (stage < events_before[L.bucket]) HIP_TRY(b, hipEventRecord(ev[stage++], b->stream));
            const hipError_t e = issue(b, c, L, done, len);
            if (e != hipSuccess) { b->err = std::string("sweep launch: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
            if (L.follows) continue;
            b->pass_launches[L.bucket]++; if (L.bucket == B_RVB) b->pass_launches[B_OTHER]++;
        }
        if (ev) { while (stage < 4) HIP_TRY(b, hipEventRecord(ev[stage++], b->stream)); timed_steps++; }
        const hipError_t er = c.recording && sample ? record_append(b) : hipSuccess;
        if (er != hipSuccess) { b->err = std::string("sample record: ") + hipGetErrorString(er); return ISINGMC_ENODEVICE; }
    }
    HIP_TRY(b, hipEventRecord(b->ev1, b->stream));
    rc = check_errors(b);
    // kernel time of the call and of its buckets: the events of the timed steps, scaled up to the whole run; all of it under B_OTHER when not split
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->ev0, b->ev1) == hipSuccess) { b->last_ms = ms; b->last_launches = b->pass_launches[B_DIAG] + b->pass_launches[B_OTHER]; }
    if (!c.split) b->pass_ms[B_OTHER] = b->last_ms;
    for (size_t i = 0; i < timed_steps; ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, b->evpool[4 * i], b->evpool[4 * i + 1]) == hipSuccess) b->pass_ms[B_DIAG] += t;
        if (hipEventElapsedTime(&t, b->evpool[4 * i + 1], b->evpool[4 * i + 3]) == hipSuccess) b->pass_ms[B_OTHER] += t;
        if (hipEventElapsedTime(&t, b->evpool[4 * i + 1], b->evpool[4 * i + 2]) == hipSuccess) b->pass_ms[B_RVB] += t;
    }
    const float scale = timed_steps && timed_steps < nsteps ? (float)nsteps / (float)timed_steps : 1.f;
    for (float &t : b->pass_ms) t *= scale;
    if (rc) return rc;
    if (out_host) HIP_TRY(b, hipMemcpy(out_host, b->d_out, sizeof(uint32_t) * b->dev.R, hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}

extern "C" {

int isingmc_diagonal_update(isingmc_batch *b, const double *beta, uint32_t flags) {
    uint32_t m = SSE_DO_DIAG | SSE_DO_GROW;
    if (flags & ISINGMC_FLAG_HEATBATH) m |= SSE_DO_HEATBATH;
    return run(b, beta, 1, 0, m, 0.5, nullptr);
}
int isingmc_cluster_update(isingmc_batch *b, double prob, uint32_t *n_clusters) {
    if (b && !(prob >= 0.0 && prob <= 1.0)) { b->err = "prob must be in [0,1]"; return ISINGMC_EINVAL; }
    std::vector<uint32_t> tmp;
    if (b && !n_clusters) { tmp.resize(b->dev.R); n_clusters = tmp.data(); }
    return run(b, nullptr, 1, 0, SSE_DO_CLUSTER, prob, n_clusters);
}
int isingmc_loop_update(isingmc_batch *b, uint32_t *lengths) {
    std::vector<uint32_t> tmp;
    if (b && !lengths) { tmp.resize(b->dev.R); lengths = tmp.data(); }
    return run(b, nullptr, 1, 0, SSE_DO_LOOP, 0.5, lengths);
}
int isingmc_rvb_update(isingmc_batch *b, uint32_t updates, uint32_t *successes) {
    if (!b) return ISINGMC_EINVAL;
    std::vector<uint32_t> tmp;
    if (!successes) { tmp.resize(b->dev.R); successes = tmp.data(); }
    b->rvb_updates = updates;
    const int rc = run(b, nullptr, 1, 0, SSE_DO_RVB, 0.5, successes);
    b->rvb_updates = 0;
    return rc;
}
int isingmc_flip_free_spins(isingmc_batch *b) { return run(b, nullptr, 1, 0, SSE_DO_FREE, 0.5, nullptr); }

int isingmc_timesteps(isingmc_batch *b, uint64_t t, const double *beta, uint32_t sampling_freq, uint32_t flags) {
    if (!b) return ISINGMC_EINVAL;
    b->rvb_updates = 0;
    uint32_t m = SSE_DO_DIAG | SSE_DO_GROW | SSE_DO_FREE;
    if (flags & ISINGMC_FLAG_HEATBATH) m |= SSE_DO_HEATBATH;
    if (flags & ISINGMC_FLAG_LOOP) m |= SSE_DO_LOOP;
    if (flags & ISINGMC_FLAG_RVB) m |= SSE_DO_RVB;
    if (!(flags & ISINGMC_FLAG_NO_CLUSTER)) m |= SSE_DO_CLUSTER;
    if (flags & ISINGMC_FLAG_PREP) m |= 0x10000u;
    if (sampling_freq == 0) sampling_freq = 1; // qmc_stepper.rs:147 unwrap_or(1)
    if (t == 0) return ISINGMC_OK;
    if (b->rec && t / sampling_freq > (uint64_t)(b->rec_cap - b->rec_count)) { // before anything is launched: the batch stays as it is
        char buf[160];
        snprintf(buf, sizeof buf, "sample record: %llu samples do not fit behind the %u recorded (capacity %u)", (unsigned long long)(t / sampling_freq), b->rec_count, b->rec_cap);
        b->err = buf;
        return ISINGMC_ECAPACITY;
    }
    return run(b, beta, t, sampling_freq, m, 0.5, nullptr);
}

} // extern "C"
