// isingmc_hip.hip — C ABI (include/isingmc_hip.h) over the gfx950 kernels (sse_launch.h); parallel tempering lives in pt.hip, the sample record in record.hip.
// Host side only sequences launches and moves small control arrays; there is no CPU compute fallback.
#include "batch.hip.h"
#include "sse_core.hip.h" // Lds<W>::carve, Rng
#include "sse_fast.hip.h" // fast_carve
#include "sse_launch.h"
#include "sse_rvb.hip.h"  // rvb_carve

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace sse;

static thread_local std::string g_create_error;

// All that plan_batch() chooses (isingmc_plan_batch reports it): the geometry, and what isingmc_create sizes its allocations by or
// hands to the DevBatch, which owns those values from then on
struct BatchPlan : BatchGeometry {
    uint32_t Wmax = 0;                  // most waves any launch may use: sizes the row stride, the HBM tables and the union-find scratch
    uint32_t CH = 0, nchunks = 0, stride = 0; // isingmc_plan_geometry(cap, W, K, Wmax)
    uint32_t pm_words = 0;              // +-J decode: sign words per bond-table row (0 = another decode)
    uint32_t tbl_stride = 0;            // bytes per replica of the per-variable tables in HBM (0 = they live in LDS)
    size_t ufstride = 0;                // words per replica of the union-find scratch in HBM: Wmax N + cap ids and two bit arrays over them
    uint32_t lds_ufcap = 0;             // ids of the LDS union-find of the first general launch
};


template <typename T>
static int dalloc(isingmc_batch *b, T **p, size_t count, bool zero = true) {
    void *q = nullptr;
    size_t bytes = (count ? count : 1) * sizeof(T);
    HIP_TRY(b, hipMalloc(&q, bytes));
    b->allocs.push_back(q);
    if (zero) HIP_TRY(b, hipMemset(q, 0, bytes));
    *p = reinterpret_cast<T *>(q);
    return ISINGMC_OK;
}

__global__ void init_state_kernel(DevBatch B) {
    // classical/graph.rs:451-453 make_random_spin_state: one fair bit per variable (Philox tag INIT, epoch 0)
    const uint32_t r = blockIdx.x;
    const Rng rng = make_rng(B, r, 0ull);
    for (uint32_t i = threadIdx.x; i < B.nwords; i += blockDim.x) {
        uint32_t s = 0;
        for (uint32_t j = 0; j < 32 && i * 32 + j < B.N; ++j) s |= (rng.draw(SSE_TAG_INIT, i * 32 + j).x >> 31) << j;
        B.state[(size_t)r * B.nwords + i] = s;
    }
}


// Verify::verify (qmc_ising.rs:829-860; op_container.rs:137-159), one thread per replica (debug API, not on
// the hot path).  ok[r] = 1 iff every op has non-zero weight, the propagated state matches every op's
// inputs, periodicity holds, no op sits beyond the cutoff and the counters n / ntrans match the op-string.
__global__ void verify_kernel(DevBatch B, uint32_t *scratch_state /*[R][nwords]*/, uint8_t *ok) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B.R) return;
    uint32_t *s = scratch_state + (size_t)r * B.nwords;
    const uint32_t *s0 = B.state + (size_t)r * B.nwords;
    for (uint32_t i = 0; i < B.nwords; ++i) s[i] = s0[i];
    const uint32_t *ops = B.ops + (size_t)r * B.stride;
    const uint32_t M = B.cutoff[r];
    bool good = true;
    uint32_t count = 0, ntr = 0, ccn = 0, cctr = 0;
    const uint32_t *chunks = B.chunks + (size_t)r * 2 * SSE_MAX_CHUNKS;
    for (uint32_t p = 0; p < B.cap; ++p) {
        if (p % B.CH == 0 && p) { // per-chunk counters kept by the diagonal pass must match the op-string
            const uint32_t c = p / B.CH - 1;
            if (chunks[c] != ccn || chunks[SSE_MAX_CHUNKS + c] != cctr) good = false;
            ccn = 0; cctr = 0;
        }
        const uint32_t w = ops[p];
        if (!w) continue;
        ccn++;
        if (p >= M) { good = false; break; }
        count++;
        const uint32_t b = sse_op_bond(w);
        if (b >= B.Nb) { good = false; break; }
        const BondRec rec = B.bonds[(size_t)(B.ham_row ? B.ham_row[r] : r) * B.bond_stride + b];
        Bd d;
        d.a = rec.a_info & SSE_VAR_MASK; d.c = rec.c; d.kp = rec.a_info >> SSE_INFO_SHIFT; d.w = rec.w;
        const uint32_t in = sse_op_in(w), out = sse_op_out(w);
        if (!(op_weight(B, b, d, in, out) > 2.220446049250313e-16)) good = false;
        if (bd_kind(d) == SSE_BOND_TRANSVERSE) { ntr++; cctr++; }
        const uint32_t a = d.a, c = d.c;
        if (((s[a >> 5] >> (a & 31)) & 1u) != (in & 1u)) good = false;
        s[a >> 5] = (s[a >> 5] & ~(1u << (a & 31))) | ((out & 1u) << (a & 31));
        if (c != SSE_NO_VAR) {
            if (((s[c >> 5] >> (c & 31)) & 1u) != ((in >> 1) & 1u)) good = false;
            s[c >> 5] = (s[c >> 5] & ~(1u << (c & 31))) | (((out >> 1) & 1u) << (c & 31));
        } else if ((in | out) & 2u) good = false;
    }
    if (good) { // last chunk
        const uint32_t c = (B.cap - 1) / B.CH;
        if (chunks[c] != ccn || chunks[SSE_MAX_CHUNKS + c] != cctr) good = false;
    }
    for (uint32_t i = 0; i < B.nwords; ++i) if (s[i] != s0[i]) good = false;
    if (count != B.n[r] || ntr != B.ntrans[r]) good = false;
    ok[r] = good ? 1 : 0;
}

// OpContainer::itime_fold (fast_ops.rs:1296-1315) for the magnetisation: sums over p = 0..cutoff-1 of m, m^2, |m| of
// the propagated state BEFORE slot p's op, m = sum_v (2 s_v - 1).  m only moves at off-diagonal ops (+-2 per flipped
// spin), so every thread takes a contiguous block of slots: block deltas -> exclusive prefix over the workgroup ->
// each thread replays its block from its starting m.  One workgroup of 256 threads per replica.
__global__ __launch_bounds__(256) void itime_magnetization_kernel(DevBatch B, long long *sum_m, unsigned long long *sum_m2,
                                                                  unsigned long long *sum_abs) {
    __shared__ long long sh[256];
    __shared__ long long red[3][4];
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    const uint32_t M = B.cutoff[r];
    const uint32_t *ops = B.ops + (size_t)r * B.stride;
    long long m0 = 0;
    for (uint32_t i = tid; i < B.nwords; i += 256) m0 += 2ll * __popc(B.state[(size_t)r * B.nwords + i]);
    for (int off = 32; off > 0; off >>= 1) m0 += __shfl_down(m0, off);
    if ((tid & 63) == 0) red[0][tid >> 6] = m0;
    const uint32_t per = (M + 255u) / 256u, p_lo = min(tid * per, M), p_hi = min(p_lo + per, M);
    auto delta = [](uint32_t w) -> long long {
        const uint32_t x = sse_op_in(w), y = sse_op_out(w);
        return 2ll * ((long long)(y & 1u) - (long long)(x & 1u) + (long long)((y >> 1) & 1u) - (long long)((x >> 1) & 1u));
    };
    long long d = 0;
    for (uint32_t p = p_lo; p < p_hi; ++p) d += delta(ops[p]);
    sh[tid] = d;
    __syncthreads();
    long long m = red[0][0] + red[0][1] + red[0][2] + red[0][3] - (long long)B.N; // popcount bits outside N are zero
    for (uint32_t t = 0; t < tid; ++t) m += sh[t];
    long long s1 = 0;
    unsigned long long s2 = 0, sa = 0;
    for (uint32_t p = p_lo; p < p_hi; ++p) {
        s1 += m; s2 += (unsigned long long)(m * m); sa += (unsigned long long)(m < 0 ? -m : m);
        m += delta(ops[p]);
    }
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); sa += __shfl_down(sa, off);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = s1; red[1][tid >> 6] = (long long)s2; red[2][tid >> 6] = (long long)sa; }
    __syncthreads();
    if (tid == 0) {
        sum_m[r] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        sum_m2[r] = (unsigned long long)(red[1][0] + red[1][1] + red[1][2] + red[1][3]);
        sum_abs[r] = (unsigned long long)(red[2][0] + red[2][1] + red[2][2] + red[2][3]);
    }
}

// DebugOps::count_diagonal_and_off / count_constant_ops (qmc_debug.rs:10-41): one workgroup per replica, out[r] = {diagonal,
// off-diagonal, constant} ops among the slots below the cutoff
__global__ __launch_bounds__(256) void debug_counts_kernel(DevBatch B, uint32_t *out) {
    __shared__ uint32_t red[3];
    const uint32_t r = blockIdx.x;
    if (threadIdx.x < 3) red[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t *ops = B.ops + (size_t)r * B.stride;
    const uint32_t M = B.cutoff[r];
    const BondRec *bonds = B.bonds + (size_t)(B.bond_stride ? (B.ham_row ? B.ham_row[r] : r) : 0u) * B.bond_stride;
    uint32_t d = 0, o = 0, c = 0;
    for (uint32_t p = threadIdx.x; p < M; p += blockDim.x) {
        const uint32_t w = ops[p];
        if (!w) continue;
        if (sse_op_is_diagonal(w)) d++; else o++;
        if (((bonds[sse_op_bond(w)].a_info >> SSE_INFO_SHIFT) & SSE_BOND_KIND_MASK) == SSE_BOND_TRANSVERSE) c++; // BasicOp::constant
    }
    atomicAdd(&red[0], d); atomicAdd(&red[1], o); atomicAdd(&red[2], c);
    __syncthreads();
    if (threadIdx.x < 3) out[3 * r + threadIdx.x] = red[threadIdx.x];
}

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

static bool is_tg(uint32_t mode) { return mode == SSE_MODE_GLOBAL_TABLES || mode == SSE_MODE_PM_GLOBAL_TABLES; }
static bool is_pm(uint32_t mode) { return mode == SSE_MODE_PM_GLOBAL_TABLES; }
static bool is_tg(const isingmc_batch *b) { return is_tg(b->mode); }
static bool is_pm(const isingmc_batch *b) { return is_pm(b->mode); }
static uint32_t lds_edges(uint32_t mode, const DevBatch &D) { return mode == SSE_MODE_LDS_EDGES ? D.E : 0u; } // compact edge table words in LDS
static uint32_t lds_edges(const isingmc_batch *b) { return lds_edges(b->mode, b->dev); }
// the wave counts per replica that the kernels are built for (sweep_w*.hip), and a count's place among them (-1: not one)
constexpr uint32_t WAVES[5] = {1, 4, 6, 8, 16};
static int wave_index(uint32_t W) { for (int i = 0; i < 5; ++i) if (WAVES[i] == W) return i; return -1; }

// Dynamic LDS of every kind of launch, read off the carve its kernel lays its LDS out with (the carves are the only statement of
// the layouts; what the host adds on top — constant-op tables, growth areas, headroom — is policy and stays at the call sites).
// f(L) on a fresh Lds<W> for the runtime wave count W (one of WAVES)
template <class F>
static size_t with_lds(uint32_t W, F &&f) {
    switch (wave_index(W)) {
    case 0: return f(Lds<WAVES[0]>{});
    case 1: return f(Lds<WAVES[1]>{});
    case 2: return f(Lds<WAVES[2]>{});
    case 3: return f(Lds<WAVES[3]>{});
    default: return f(Lds<WAVES[4]>{});
    }
}
// general / off-diagonal launch at W waves whose LDS union-find holds ufcap ids (tg: per-variable tables in HBM; pm_words: +-J signs)
static size_t general_lds_words(uint32_t W, const DevBatch &D, uint32_t ledges, bool tg, uint32_t pm_words, uint32_t ufcap) {
    return with_lds(W, [&](auto L) { L.carve(D.N, D.nwords, ufcap, ledges, D.has_long, tg, pm_words); return (size_t)L.end; });
}
// diagonal-pass launch (diag_only: the +-J decode's diagonal kernel, mode SSE_MODE_PM_LDS_TABLES)
static size_t diag_lds_words(uint32_t W, const DevBatch &D, uint32_t ledges, bool tg, uint32_t pm_words, bool diag_only = false) {
    return with_lds(W, [&](auto L) { L.carve(D.N, D.nwords, 0u, ledges, 0u, tg, pm_words, diag_only); return (size_t)L.end_diag; });
}
// trimmed diagonal-pass launch (sse_fast.hip.h): its tables, or the compact edge table that the directed loop behind the pass stages
// in the same place
static size_t fast_lds_words(const DevBatch &D) {
    Lds<4> L;
    L.carve(D.N, D.nwords, 0u, D.E, 0u);
    return std::max<size_t>(fast_carve<4>(L, D).end, L.o_signs);
}
// RVB sweep inside the general kernel at W waves: its scratch (rvb_carve) and a constant-op table of cap entries (cutoff <= cap)
static size_t rvb_lds_words(uint32_t W, const DevBatch &D, uint32_t ledges, bool tg, uint32_t pm_words) {
    return with_lds(W, [&](auto L) { RvbLds R; L.carve(D.N, D.nwords, 0u, ledges, 0u, tg, pm_words); rvb_carve(R, L, D); return (size_t)R.o_cps + D.cap; });
}
// RVB sweep with its tables in HBM (SSE_PASSES_RVB_G, 16 waves): the LDS scratch of rvb_carve<16, true> and `areas` small growth areas
static size_t rvb_global_lds_words(const isingmc_batch *b, uint32_t areas) {
    Lds<16> L; RvbLds R;
    L.carve(b->dev.N, b->dev.nwords, 0u, lds_edges(b), 0u, true);
    rvb_carve<16, true>(R, L, b->dev);
    return (size_t)R.o_free + (size_t)areas * SSE_RVB_SLOT_WORDS;
}
// bytes of a launch of `words` dynamic LDS words (whole 8-byte units)
static size_t lds_bytes_of(size_t words) { return (4 * words + 7) & ~(size_t)7; }
// a launch and the DevBatch it is given: the LDS it asks for and the LDS its kernel sees (DevBatch::lds_words), from one word count
static void give_lds(LaunchCfg &c, DevBatch &d, size_t words) {
    c.lds_bytes = lds_bytes_of(words);
    d.lds_words = (uint32_t)(c.lds_bytes / 4);
}

// LDS footprint of the next launch.  The union-find of the cluster pass lives in LDS as 16-bit parents when all
// ids fit; its capacity follows the largest transverse-op count seen so far (+ headroom), so that the footprint
// stays small enough for two workgroups per CU whenever the model allows it.  Replicas that outgrow it use the HBM
// union-find for that sweep and the host enlarges the table before the next launch.
struct LdsPlan { uint32_t W, ufcap; size_t words; bool all_ids_fit; };
// What such a plan is made from: the model's shape (D: N, E, cap, nwords, has_long, pm_words), the batch's mode, all of LDS, the
// test limit on the ids and the largest transverse-op count seen so far
struct LdsNeeds { const DevBatch &D; uint32_t mode; size_t total_words; uint32_t uf_ids_limit, max_ntrans; };
static LdsNeeds lds_needs(const isingmc_batch *b) { return {b->dev, b->mode, b->lds_total_words, b->uf_ids_limit, b->max_ntrans}; }
// ids that the union-find of a launch at W waves is sized for: W per variable, the transverse ops seen so far, headroom
static size_t uf_ids_wanted(const LdsNeeds &n, uint32_t W) { return (size_t)W * n.D.N + n.max_ntrans + n.max_ntrans / 16 + 384; }
static LdsPlan plan_lds(const LdsNeeds &n, uint32_t W) {
    const DevBatch &D = n.D;
    const bool tg = is_tg(n.mode);
    auto words = [&](size_t ids) { return general_lds_words(W, D, lds_edges(n.mode, D), tg, is_pm(n.mode) ? D.pm_words : 0u, (uint32_t)ids); };
    const size_t ids_max = (size_t)W * D.N + D.cap;
    const size_t want = uf_ids_wanted(n, W);
    size_t ids = want;
    if (n.uf_ids_limit) ids = n.uf_ids_limit;
    if (tg) ids = 0; // tables in HBM: the union-find lives there too
    if (ids > 65535) ids = 65535;
    if (ids > ids_max) ids = ids_max;
    while (ids > 0 && words(ids) > n.total_words) ids -= (ids > 64 ? 64 : ids);
    LdsPlan p;
    p.W = W; p.ufcap = (uint32_t)ids;
    p.words = words(ids);
    p.all_ids_fit = !tg && words(0) + 64 <= n.total_words && ids >= (want < ids_max ? want : ids_max) && !n.uf_ids_limit;
    return p;
}
static LdsPlan plan_lds(const isingmc_batch *b, uint32_t W) { return plan_lds(lds_needs(b), W); }
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

static int check_errors(isingmc_batch *b) {
    std::vector<uint32_t> err(b->dev.R), ntr(b->dev.R);
    HIP_TRY(b, hipMemcpyAsync(err.data(), b->dev.err, sizeof(uint32_t) * b->dev.R, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipMemcpyAsync(ntr.data(), b->dev.ntrans, sizeof(uint32_t) * b->dev.R, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    for (uint32_t r = 0; r < b->dev.R; ++r) if (ntr[r] > b->max_ntrans) b->max_ntrans = ntr[r];
    for (uint32_t r = 0; r < b->dev.R; ++r)
        if (err[r]) {
            char buf[160];
            if (err[r] == 1u) {
                snprintf(buf, sizeof buf, "replica %u: cutoff n + n/2 exceeds the op-string capacity %u", r, b->dev.cap);
                b->err = buf;
                return ISINGMC_ECAPACITY;
            }
            if (err[r] == 8u) {
                snprintf(buf, sizeof buf, "replica %u: more than 65534 transverse ops inside one wave's range of the cluster scan; raise waves_per_replica", r);
                b->err = buf;
                return ISINGMC_ECAPACITY;
            }
            if (err[r] == 6u || err[r] == 7u || err[r] == 5u) {
                snprintf(buf, sizeof buf, "replica %u: RVB working set exceeds the LDS scratch (code %u)", r, err[r]);
                b->err = buf;
                return ISINGMC_ECAPACITY;
            }
            if (err[r] == 3u) {
                snprintf(buf, sizeof buf, "replica %u: directed loop still open after 64*cutoff+1024 vertices (the reference has no bound; "
                                          "clear with isingmc_clear_errors and continue)", r);
                b->err = buf;
                return ISINGMC_ELIMIT;
            }
            snprintf(buf, sizeof buf, "replica %u: device integrity error %u", r, err[r]);
            b->err = buf;
            return ISINGMC_EINTEGRITY;
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
        const size_t words = rvb_tbl_words(b->dev.N, b->dev.E, b->dev.cap);
        if (words > 0xFFFFFFFFull) { b->err = "RVB table scratch: more than 2^32 words per replica"; return ISINGMC_ECAPACITY; }
        void *q = nullptr;
        if (hipMalloc(&q, (size_t)b->dev.R * words * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            char buf[160];
            snprintf(buf, sizeof buf, "RVB table scratch (ISINGMC_CFG_RVB_GLOBAL_TABLES): hipMalloc of %zu bytes failed", (size_t)b->dev.R * words * sizeof(uint32_t));
            b->err = buf;
            return ISINGMC_ENODEVICE;
        }
        b->dev.rvb_tbl = (uint32_t *)q;
    }
    if (rvb_g && rvb_global_lds_words(b, 0) > b->lds_total_words) { b->err = "RVB scratch (ISINGMC_CFG_RVB_GLOBAL_TABLES): the spin-state bit arrays and the fixed RVB regions exceed LDS"; return ISINGMC_ENOTIMPL; }
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
        if (b->dev.rvb_prod) { (void)hipStreamSynchronize(b->stream); (void)hipFree(b->dev.rvb_prod); b->dev.rvb_prod = nullptr; b->dev.rvb_prod_cap = 0; }
        void *q = nullptr;
        if (hipMalloc(&q, (size_t)b->dev.R * updates * pstride * sizeof(uint32_t)) == hipSuccess) { b->dev.rvb_prod = (uint32_t *)q; b->dev.rvb_prod_cap = updates; b->dev.rvb_prod_stride = (uint32_t)pstride; }
        else { (void)hipGetLastError(); b->rvb_split = false; } // no room for the records: the fused kernel from now on
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
        r.words = std::min(rvb_global_lds_words(b, 16), b->lds_total_words); // (fewer small growth areas; the large one always fits)
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

// ---- isingmc_create in four parts: check_config, build_tables, plan_batch, allocate_and_upload -------------------------------
// Everything up to the plan reads the config alone and touches no device, so that isingmc_plan_batch can run it on any host.
static int refuse(int rc, const char *why) { g_create_error = why; return rc; }
static bool per_replica_J(const isingmc_config *cfg) { return (cfg->flags & ISINGMC_CFG_PER_REPLICA_J) != 0; }
static double gamma_of(const isingmc_config *cfg, uint32_t row) { return cfg->transverse_r ? cfg->transverse_r[row] : cfg->transverse; }
static double hfield_of(const isingmc_config *cfg, uint32_t row) { return cfg->longitudinal_r ? cfg->longitudinal_r[row] : cfg->longitudinal; }
static bool has_longitudinal(const isingmc_config *cfg) { return !cfg->interactions && std::fabs(hfield_of(cfg, 0)) > DBL_EPSILON; } // qmc_ising.rs:230

// The argument checks that isingmc_create makes before it looks for a device (cfg itself is readable: the entry points see to that)
static int check_config(const isingmc_config *cfg) {
    const bool generic = cfg->interactions != nullptr;
    if (generic) {
        if (cfg->nreplicas == 0 || cfg->nvars == 0 || cfg->ninteractions == 0) return refuse(ISINGMC_EINVAL, "nreplicas, nvars, ninteractions must be > 0");
        if (per_replica_J(cfg)) return refuse(ISINGMC_EINVAL, "per-replica couplings are not available with generic interactions");
        for (uint32_t i = 0; i < cfg->ninteractions; ++i) {
            const isingmc_interaction &it = cfg->interactions[i];
            if (it.nvars > 2) // qmc_runner.rs:415-680 allows any k; the 32-bit operator word holds two variables
                return refuse(ISINGMC_ENOTIMPL, "interactions on more than two variables are not implemented (operator word = 2 in + 2 out bits)");
            if ((it.nvars != 1 && it.nvars != 2) || !it.mat || it.vars[0] >= cfg->nvars || (it.nvars == 2 && (it.vars[1] >= cfg->nvars || it.vars[1] == it.vars[0])))
                return refuse(ISINGMC_EINVAL, "interaction must act on 1 or 2 distinct variables inside the model and carry a matrix");
            for (uint32_t k = 0; k < (it.diagonal_only ? (1u << it.nvars) : (1u << (2 * it.nvars))); ++k)
                if (!(it.mat[k] >= 0.0) || !std::isfinite(it.mat[k])) return refuse(ISINGMC_EINVAL, "interaction matrix entries must be finite and >= 0");
        }
    } else if (cfg->nreplicas == 0 || cfg->nvars == 0 || (cfg->nedges != 0 && (!cfg->edges || !cfg->J)))
        return refuse(ISINGMC_EINVAL, "nreplicas and nvars must be > 0 and edges/J non-null when nedges > 0");
    if (cfg->capacity == 0) return refuse(ISINGMC_EINVAL, "capacity must be > 0");
    if (cfg->cutoff0 > cfg->capacity) return refuse(ISINGMC_EINVAL, "cutoff0 exceeds capacity");
    if (cfg->nvars > SSE_VAR_MASK) return refuse(ISINGMC_EINVAL, "too many variables");
    if (!generic && !(cfg->transverse >= 0.0)) return refuse(ISINGMC_EINVAL, "transverse field must be >= 0");
    for (uint32_t e = 0; !generic && e < cfg->nedges; ++e)
        if (cfg->edges[2 * e] >= cfg->nvars || cfg->edges[2 * e + 1] >= cfg->nvars || cfg->edges[2 * e] == cfg->edges[2 * e + 1])
            return refuse(ISINGMC_EINVAL, cfg->edges[2 * e] == cfg->edges[2 * e + 1] ? "edge joins a variable to itself (self-loop)" : "edge endpoint out of range");
    return ISINGMC_OK;
}
// The model fields of a DevBatch (its shape and fields; the tables add uniformJ / wJ / wtot, the plan its geometry)
static DevBatch model_of(const isingmc_config *cfg) {
    const bool generic = cfg->interactions != nullptr, has_long = has_longitudinal(cfg);
    DevBatch D{};
    D.R = cfg->nreplicas; D.N = cfg->nvars; D.E = generic ? 0u : cfg->nedges;
    D.Nb = generic ? cfg->ninteractions : cfg->nedges + cfg->nvars + (has_long ? cfg->nvars : 0);
    D.cap = cfg->capacity; D.nwords = (cfg->nvars + 31) / 32;
    D.seed_lo = (uint32_t)cfg->seed; D.seed_hi = (uint32_t)(cfg->seed >> 32);
    D.replica_offset = cfg->replica_offset;
    D.gamma = cfg->transverse; D.wh = 2.0 * std::fabs(cfg->longitudinal); D.hpos = cfg->longitudinal > 0.0 ? 1u : 0u;
    D.has_long = has_long ? 1u : 0u;
    D.bond_stride = per_replica_J(cfg) ? D.Nb : 0u;
    D.rvb_growers = (cfg->flags & ISINGMC_CFG_RVB_SERIAL_GROWTH) ? 0u : 64u;
    return D;
}

// The checks behind the device probe that need no plan: fields, bond count, the geometry wishes (plan_batch refuses the rest where it
// meets them, in the order they always had)
static int check_config_model(const isingmc_config *cfg) {
    const bool generic = cfg->interactions != nullptr, perJ = per_replica_J(cfg), has_long = has_longitudinal(cfg);
    if ((cfg->transverse_r || cfg->longitudinal_r) && (!perJ || generic)) return refuse(ISINGMC_EINVAL, "per-replica fields need ISINGMC_CFG_PER_REPLICA_J (per-replica bond tables)");
    for (uint32_t r = 0; !generic && r < (perJ ? cfg->nreplicas : 1u); ++r) {
        if (!(gamma_of(cfg, r) >= 0.0) || !std::isfinite(gamma_of(cfg, r)) || !std::isfinite(hfield_of(cfg, r))) return refuse(ISINGMC_EINVAL, "fields must be finite, transverse field >= 0");
        if ((std::fabs(hfield_of(cfg, r)) > DBL_EPSILON) != has_long) return refuse(ISINGMC_EINVAL, "longitudinal fields must be all zero or all non-zero within a batch");
    }
    if (model_of(cfg).Nb > SSE_MAX_BONDS) return refuse(ISINGMC_EINVAL, "too many bonds");
    if (wave_index(cfg->waves_per_replica ? cfg->waves_per_replica : 4) < 0) return refuse(ISINGMC_EINVAL, "waves_per_replica must be 1, 4, 6, 8 or 16");
    const uint32_t K = cfg->slots_per_lane ? cfg->slots_per_lane : 4;
    if (K != 1 && K != 2 && K != 4) return refuse(ISINGMC_EINVAL, "slots_per_lane must be 1, 2 or 4");
    return ISINGMC_OK;
}

// Everything that create uploads, on the host: made from the config alone
struct Tables {
    std::vector<BondRec> bonds;          // [nH][Nb], nH = one row, or one per replica (ISINGMC_CFG_PER_REPLICA_J: cfg->J is [R][E])
    std::vector<double> cum, wtots;      // [nH][Nb] heat-bath cumulative weights; [nH] their totals
    std::vector<double> offsets;         // [nH] energy offsets (per-replica J only)
    double offset = 0.0;                 // ... of row 0
    std::vector<double> mats;            // generic interactions: [Nb][16] in | out<<2
    bool generic_sym = false;            // ... all of them symmetric under a global spin flip
    uint32_t uniformJ = 1u; double wJ = 0.0; // one |J| on every edge of every row (the kernels keep 2|J| in a scalar register)
    std::vector<double> edge_w;          // [E] 2|J| of row 0
    std::vector<uint32_t> edges_compact; // [E] a | c << 15 | prefers_aligned << 30 (N <= SSE_CE_MAX_VARS, else zeros)
    std::vector<uint32_t> signs;         // [nH][ceil(E / 32)] bit e = prefers aligned (J < 0): the +-J decode's rows
    std::vector<uint32_t> adj_start, adj; // [N + 2], [2 E + 1] bonds_for_var (make_classical_bonds, qmc_ising.rs:421-432): edge order
};
// bond b = interaction b.  Weights go to mats[b][in | out<<2] (bit 0 = first variable); the reference's index is (out0 out1 in0 in1)
// with the first variable most significant (Interaction::index_from_state, qmc_runner.rs:666-679).  Kinds only feed the
// transverse-op counters: a one-variable interaction with four equal entries is a cluster edge (cluster.rs:284-286).
static void generic_tables(const isingmc_config *cfg, uint32_t Nb, Tables &T) {
    T.mats.assign((size_t)Nb * 16, 0.0);
    T.generic_sym = true;
    double c = 0.0;
    for (uint32_t i = 0; i < Nb; ++i) {
        const isingmc_interaction &it = cfg->interactions[i];
        double *mb = T.mats.data() + (size_t)i * 16;
        for (uint32_t in = 0; in < (1u << it.nvars); ++in)      // device layout: bit 0 = first variable
            for (uint32_t out = 0; out < (1u << it.nvars); ++out) {
                const uint8_t ib[2] = {(uint8_t)(in & 1u), (uint8_t)((in >> 1) & 1u)}, ob[2] = {(uint8_t)(out & 1u), (uint8_t)((out >> 1) & 1u)};
                (void)isingmc_interaction_at(&it, ib, ob, &mb[in | (out << 2)]);
            }
        double maxw = 0.0; // heatbath.rs:130-146 make_bond_weights: largest diagonal element
        for (uint32_t st = 0; st < (it.nvars == 2 ? 4u : 2u); ++st) maxw = std::max(maxw, mb[st | (st << 2)]);
        const uint32_t kind = it.nvars == 2 ? SSE_BOND_TWO_SITE
                              : ((mb[0] == mb[1] && mb[0] == mb[4] && mb[0] == mb[5]) ? SSE_BOND_TRANSVERSE : SSE_BOND_LONGITUDINAL);
        T.bonds[i].a_info = it.vars[0] | (kind << SSE_INFO_SHIFT);
        T.bonds[i].c = it.nvars == 2 ? it.vars[1] : SSE_NO_VAR;
        T.bonds[i].w = maxw;
        c = (i == 0) ? maxw : maxw + c;
        T.cum[i] = c;
        // EVERY weight equals the weight with all spins flipped.  (Not isingmc_interaction_sym_under_ising: like the reference's
        // Interaction::sym_under_ising, qmc_runner.rs:639-664, that one only compares the entries whose outputs are all 0, and
        // passes two-variable matrices that break the symmetry elsewhere.)
        const uint32_t mask = it.nvars == 2 ? 0xFu : 0x5u;
        for (uint32_t idx = 0; idx < 16; ++idx)
            if ((idx & ~mask) == 0 && std::fabs(mb[idx] - mb[idx ^ mask]) >= DBL_EPSILON) T.generic_sym = false;
    }
    T.wtots[0] = c;
    T.offset = cfg->energy_offset;
}
// Bond-table row hI of an Ising model (qmc_ising.rs:186-205,228-246; weights :863-888; offsets :97-99): edges, transverse bonds,
// longitudinal bonds when there is a field
static void ising_row(const isingmc_config *cfg, const DevBatch &D, uint32_t hI, Tables &T) {
    BondRec *t0 = T.bonds.data() + (size_t)hI * D.Nb;
    const double *Jh = cfg->J + (size_t)hI * D.E;
    double off = 0.0;
    for (uint32_t e = 0; e < D.E; ++e) {
        const double J = Jh[e];
        t0[e].a_info = cfg->edges[2 * e] | ((SSE_BOND_TWO_SITE | (J < 0.0 ? SSE_BOND_PREF_BIT : 0u)) << SSE_INFO_SHIFT);
        t0[e].c = cfg->edges[2 * e + 1];
        t0[e].w = 2.0 * std::fabs(J);
        off += std::fabs(J);
        if (J < 0.0) T.signs[(size_t)hI * ((D.E + 31u) / 32u) + (e >> 5)] |= 1u << (e & 31);
    }
    const double gam = gamma_of(cfg, hI), hl = hfield_of(cfg, hI);
    for (uint32_t v = 0; v < D.N; ++v) {
        BondRec &t = t0[D.E + v];
        t.a_info = v | (SSE_BOND_TRANSVERSE << SSE_INFO_SHIFT); t.c = SSE_NO_VAR; t.w = gam;
    }
    for (uint32_t v = 0; D.has_long && v < D.N; ++v) {
        BondRec &t = t0[D.E + D.N + v];
        t.a_info = v | ((SSE_BOND_LONGITUDINAL | (hl > 0.0 ? SSE_BOND_PREF_BIT : 0u)) << SSE_INFO_SHIFT);
        t.c = SSE_NO_VAR; t.w = 2.0 * std::fabs(hl);
    }
    const double offset = off + (double)D.N * (gam + std::fabs(hl));
    if (hI == 0) T.offset = offset;
    if (D.bond_stride) T.offsets[hI] = offset;
    double c = 0.0;
    for (uint32_t i = 0; i < D.Nb; ++i) { c = (i == 0) ? t0[0].w : t0[i].w + c; T.cum[(size_t)hI * D.Nb + i] = c; }
    T.wtots[hI] = c;
}
static Tables build_tables(const isingmc_config *cfg, const DevBatch &D) {
    const bool generic = cfg->interactions != nullptr;
    const uint32_t nH = D.bond_stride ? D.R : 1u;
    Tables T;
    T.bonds.resize((size_t)nH * D.Nb); T.cum.resize((size_t)nH * D.Nb); T.wtots.resize(nH);
    if (D.bond_stride) T.offsets.resize(nH);
    T.signs.assign((size_t)nH * ((D.E + 31u) / 32u), 0u);
    if (generic) generic_tables(cfg, D.Nb, T);
    else for (uint32_t hI = 0; hI < nH; ++hI) ising_row(cfg, D, hI, T);
    T.wJ = T.bonds[0].w;
    for (uint32_t hI = 0; hI < nH && T.uniformJ; ++hI)
        for (uint32_t e = 0; e < D.E; ++e) if (T.bonds[(size_t)hI * D.Nb + e].w != T.bonds[0].w) { T.uniformJ = 0u; break; }
    T.edge_w.resize(D.E); T.edges_compact.assign(D.E, 0u);
    for (uint32_t e = 0; e < D.E; ++e) {
        const BondRec &t = T.bonds[e];
        T.edge_w[e] = t.w;
        if (D.N <= SSE_CE_MAX_VARS)
            T.edges_compact[e] = (t.a_info & SSE_CE_VAR_MASK) | ((t.c & SSE_CE_VAR_MASK) << 15) | (((t.a_info >> (SSE_INFO_SHIFT + 2)) & 1u) << 30);
    }
    std::vector<uint32_t> &as = T.adj_start, &ad = T.adj, fill(D.N, 0u);
    as.assign(D.N + 2, 0u); ad.resize(2 * (size_t)D.E + 1);
    for (uint32_t e = 0; e < D.E; ++e) { as[cfg->edges[2 * e] + 1]++; as[cfg->edges[2 * e + 1] + 1]++; }
    for (uint32_t v = 0; v < D.N; ++v) as[v + 1] += as[v];
    for (uint32_t e = 0; e < D.E; ++e) {
        const uint32_t a = cfg->edges[2 * e], c2 = cfg->edges[2 * e + 1];
        ad[as[a] + fill[a]++] = e;
        ad[as[c2] + fill[c2]++] = e;
    }
    return T;
}

// Where the per-variable scan tables live when the caller wishes for W_wish waves (0 = no wish) and `ledges` words of compact edge
// table share the LDS: the wave count to run with, and whether the engine moves the tables to HBM by itself (they do not fit)
struct TablesHome { uint32_t W; bool hbm; };
static TablesHome tables_home(const DevBatch &D, uint32_t W_wish, uint32_t ledges, size_t total_words) {
    auto fixed_lds = [&](uint32_t w) { return general_lds_words(w, D, ledges, false, 0u, 0u); }; // (tables in LDS, no union-find)
    uint32_t W = W_wish ? W_wish : 4;
    if (fixed_lds(W) + 4096 <= total_words) return {W, false};
    if (!W_wish) return {W, true};
    // explicit geometry: keep the LDS tables if a smaller W makes them fit
    while (W > 1 && fixed_lds(W) + 4096 > total_words) W = (W == 4) ? 1 : (W == 6 ? 4 : W >> 1);
    if (fixed_lds(W) + 64 <= total_words) return {W, false};
    return {W_wish, true};
}
// What plan_batch reads: the model's shape (D: N, E, Nb, cap, nwords, has_long, uniformJ), its kind, the caller's flags and geometry
// wishes, the LDS bytes of a workgroup
struct PlanInputs {
    DevBatch D;
    bool generic, perJ, fields_r; // interaction matrices; per-replica bond tables; per-replica fields among them
    uint32_t flags, waves_per_replica, slots_per_lane, waves_offdiag, lds_uf_ids_limit, lds_bytes;
};
static PlanInputs plan_inputs(const isingmc_config *cfg, const DevBatch &D, uint32_t lds_bytes) {
    return {D, cfg->interactions != nullptr, per_replica_J(cfg), cfg->transverse_r || cfg->longitudinal_r,
            cfg->flags, cfg->waves_per_replica, cfg->slots_per_lane, cfg->waves_offdiag, cfg->lds_uf_ids_limit, lds_bytes};
}
// Every launch geometry and mode of a batch.  Reads its inputs and nothing else: no device, no batch.  The configs it cannot serve
// it refuses like the checks do, where their order among them has always been.
static int plan_batch(const PlanInputs &in, BatchPlan &p) {
    DevBatch D = in.D; // (gains pm_words below)
    const uint32_t flags = in.flags;
    const size_t total_words = (size_t)in.lds_bytes / 4; // all of LDS for one workgroup
    p = BatchPlan{};
    p.lds_total_words = total_words; p.uf_ids_limit = in.lds_uf_ids_limit;
    p.fused_launch = (flags & ISINGMC_CFG_FUSED_LAUNCH) != 0;
    // default 4 waves per replica: with 16-bit union-find parents the footprint at the headline size stays below half
    // of the 160 KB LDS, so two workgroups share a CU and overlap each other's barriers (measured best on MI355X)
    uint32_t W = in.waves_per_replica ? in.waves_per_replica : 4;
    uint32_t K = in.slots_per_lane ? in.slots_per_lane : 4;
    // compact edge table staged in LDS when it is small enough (a|c<<15|pref<<30 needs N <= 32768)
    bool CL = !in.generic && !in.perJ && D.uniformJ && D.N <= SSE_CE_MAX_VARS && (size_t)D.E * 4 <= 48 * 1024 && !(flags & ISINGMC_CFG_NO_LDS_TABLES);
    // Per-variable scan tables: in LDS while W copies of them fit (with room for a union-find), otherwise in a per-replica
    // HBM scratch served by L2 / Infinity Cache (MODE 2; ISINGMC_CFG_GLOBAL_TABLES forces it on any model).
    bool TG = (flags & ISINGMC_CFG_GLOBAL_TABLES) != 0;
    if (!TG) {
        TablesHome h = tables_home(D, in.waves_per_replica, CL ? D.E : 0u, total_words);
        // The tables do not fit next to the compact edge table (a long chain: up to 48 KB of edges): the edge table leaves LDS first
        // (the general bond table serves the model), and the HBM tables, which need the general bond table, come without it too.
        if (h.hbm && CL) { CL = false; h = tables_home(D, in.waves_per_replica, 0u, total_words); }
        W = h.W; TG = h.hbm;
    }
    const uint32_t ledges = CL ? D.E : 0u;
    // (only with the caller's own ISINGMC_CFG_GLOBAL_TABLES)
    if (TG && CL) return refuse(ISINGMC_EINVAL, "ISINGMC_CFG_GLOBAL_TABLES needs the general bond table: combine it with ISINGMC_CFG_NO_LDS_TABLES");
    if (TG && K == 2) K = 4;
    const uint32_t pm_room = TG ? (D.E + 31u) / 32u : 0u; // (room for the +-J decode's signs, decided below)
    if (general_lds_words(W, D, ledges, TG, pm_room, 0u) + 64 > total_words) return refuse(ISINGMC_ENOTIMPL, "model too large: the spin-state bit arrays alone exceed LDS");
    // off-diagonal launches may use their own wave count (see plan_off()): explicit, or decided per launch (then up to 16)
    uint32_t W_off = in.waves_offdiag;
    // (a check of the wish alone; it stands here, behind the two refusals above, because that has always been its place among them)
    if (W_off != 0 && wave_index(W_off) < 0) return refuse(ISINGMC_EINVAL, "waves_offdiag must be 0, 1, 4, 6, 8 or 16");
    if (!W_off && in.waves_per_replica) W_off = W; // an explicit waves_per_replica pins both kinds of launch
    if (TG) W_off = W;                             // tables in HBM: one geometry for every launch
    if (W_off && general_lds_words(W_off, D, ledges, TG, 0u, 0u) + 64 > total_words) W_off = W;
    auto fits_in_lds = [&](uint32_t w) { return !TG && general_lds_words(w, D, ledges, false, 0u, 0u) + 64 <= total_words; };
    const bool w16_possible = fits_in_lds(16);
    // (8 waves without an LDS union-find: the geometry of launches whose cluster ids need the 32-bit union-find in HBM anyway)
    const bool w8_possible = W < 8 && (K == 4 || K == 1) && fits_in_lds(8);
    p.w8_ok = w8_possible && !W_off;
    const uint32_t Wmax = W_off ? (W_off > W ? W_off : W) : ((W < 16 && w16_possible) ? 16u : (w8_possible ? 8u : W));
    p.W = W; p.K = K; p.W_off = W_off; p.Wmax = Wmax;
    p.mode = TG ? SSE_MODE_GLOBAL_TABLES : (CL ? SSE_MODE_LDS_EDGES : SSE_MODE_GENERAL);
    // "+-J" decode for large disorder batches (BASELINE configs[4]): every replica its own coupling signs on one graph with uniform
    // |J|, Gamma, h.  The general decode fetches a 16-byte record per op and pass from a per-replica table of megabytes — one random
    // HBM sector each time, in a mode that is bound by exactly those; here the variables come from the shared compact edge table
    // (L2-resident), the sign from 12 KB of LDS.  Default geometry only.
    if (TG && in.perJ && D.uniformJ && !in.generic && W == 4 && K == 4 && D.N <= SSE_CE_MAX_VARS && !in.fields_r && !(flags & ISINGMC_CFG_NO_PM_DECODE)) {
        p.mode = SSE_MODE_PM_GLOBAL_TABLES;
        p.pm_words = D.pm_words = (D.E + 31u) / 32u;
        // the diagonal launch keeps its per-wave spin bytes in LDS when W * N bytes fit next to the small arrays
        const size_t words = diag_lds_words(W, D, 0u, false, D.pm_words, true);
        p.lds_words_pm_diag = (words + 64 <= total_words && !(flags & ISINGMC_CFG_GLOBAL_TABLES)) ? words : 0;
    }
    uint32_t geo[4]; // chunk grid and row stride: one function (also exported for the CPU-side bound checks of tests/test_abi_cpu.py)
    if (isingmc_plan_geometry(D.cap, W, K, Wmax, geo) != ISINGMC_OK) return refuse(ISINGMC_EINVAL, "capacity too large for the row stride");
    p.CH = geo[0]; p.nchunks = geo[1]; p.stride = geo[2];
    p.lds_words_diag = diag_lds_words(W, D, ledges, TG, pm_room);
    p.lds_words_fast = fast_lds_words(D);
    p.fast_diag = CL && !TG && W == 4 && (K == 4 || K == 2) && D.N <= SSE_FAST_MAX_VARS && !p.fused_launch &&
                  !(flags & ISINGMC_CFG_NO_FAST_DIAG) && lds_bytes_of(p.lds_words_fast) <= 40 * 1024; // 4 workgroups per CU
    // the cluster update of that geometry has its own kernel too (16 waves, packed tables; sse_cluster.hip.h)
    p.lean_cluster = CL && !TG && !in.generic && D.N <= 4095u && !p.fused_launch && !in.waves_offdiag && !in.waves_per_replica &&
                     !(flags & ISINGMC_CFG_NO_LEAN_CLUSTER);
    p.defer = p.lean_cluster && p.fast_diag && !(flags & ISINGMC_CFG_NO_DEFERRED_FLIPS);
    // the RVB pass reuses everything from the scan tables on: launches that run it get enough LDS for its scratch
    // and constant-op table (other launches keep the smaller footprint, which decides workgroups per CU)
    p.lds_words_rvb = std::min(rvb_lds_words(W, D, ledges, TG, pm_room), total_words);
    p.rvb_global = (flags & ISINGMC_CFG_RVB_GLOBAL_TABLES) != 0; // (the two-launch form keeps its tables in LDS: never with this flag)
    p.rvb_split = !in.generic && !TG && !p.fused_launch && !(flags & ISINGMC_CFG_RVB_FUSED) && !p.rvb_global;
    // waves of the RVB main launch: as many as keep about 16 waves on a CU (its LDS footprint decides how many replicas share one)
    const size_t w4 = 4 * (size_t)rvb_main_lds_words(4, D, ledges);
    const size_t per_cu = w4 ? (size_t)in.lds_bytes / w4 : 0;
    p.rvb_main_W = per_cu >= 4 ? 4u : (per_cu >= 2 ? 8u : 16u);
    if (in.waves_per_replica == 4 || in.waves_per_replica == 8 || in.waves_per_replica == 16) p.rvb_main_W = in.waves_per_replica; // an explicit geometry is honoured here too
    if (TG) p.tbl_stride = (uint32_t)((((size_t)Wmax * D.N * 4 + D.N) + 15) & ~(size_t)15); // 4-byte scan records per (wave, variable)
    const size_t ids_max = (size_t)Wmax * D.N + D.cap;
    p.ufstride = ids_max + 2 * ((ids_max + 31) / 32);
    const LdsPlan first = plan_lds(LdsNeeds{D, p.mode, total_words, p.uf_ids_limit, 0u}, W); // (prepare() sizes again from the ops seen by then)
    p.lds_words = first.words; p.lds_ufcap = first.ufcap;
    return ISINGMC_OK;
}
// check_config_model, build_tables and plan_batch for a config that passed check_config: what isingmc_create and isingmc_plan_batch share
static int plan_config(const isingmc_config *cfg, uint32_t lds_bytes, DevBatch &D, Tables &T, BatchPlan &p) {
    if (const int rc = check_config_model(cfg)) return rc;
    D = model_of(cfg);
    T = build_tables(cfg, D);
    D.uniformJ = T.uniformJ; D.wJ = T.wJ; D.wtot = T.wtots[0];
    return plan_batch(plan_inputs(cfg, D, lds_bytes), p);
}

// Apply the plan to the batch, make every allocation and every upload, set the initial state
#define CREATE_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)
template <typename T>
static int copy_up(isingmc_batch *b, T *dst, const T *host, size_t count, const char *what) {
    if (hipMemcpy(dst, host, sizeof(T) * count, hipMemcpyHostToDevice) == hipSuccess) return ISINGMC_OK;
    b->err = std::string(what) + " upload failed";
    return ISINGMC_ENODEVICE;
}
// allocate, copy this host array, or fail with "<what> upload failed"
template <typename T, typename P>
static int upload(isingmc_batch *b, P &dst, const std::vector<T> &host, const char *what) {
    T *q = nullptr;
    CREATE_TRY(dalloc(b, &q, host.size(), false));
    dst = q;
    return copy_up(b, q, host.data(), host.size(), what);
}
static int allocate_and_upload(isingmc_batch *b, const isingmc_config *cfg, const DevBatch &model, Tables &T, const BatchPlan &plan) {
    static_cast<BatchGeometry &>(*b) = plan;
    DevBatch &D = b->dev;
    D = model;
    D.CH = plan.CH; D.nchunks = plan.nchunks; D.stride = plan.stride; D.pm_words = plan.pm_words; D.tbl_stride = plan.tbl_stride; D.lds_ufcap = plan.lds_ufcap;
    b->generic = cfg->interactions != nullptr; b->generic_sym = T.generic_sym;
    b->per_replica_J = D.bond_stride != 0; b->offset = T.offset; b->offsets = std::move(T.offsets);
    const size_t R = D.R;
    CREATE_TRY(dalloc(b, &D.ops, R * D.stride));
    CREATE_TRY(dalloc(b, &D.state, R * D.nwords));
    CREATE_TRY(dalloc(b, &D.n, R));
    CREATE_TRY(dalloc(b, &D.ntrans, R));
    CREATE_TRY(dalloc(b, &D.cutoff, R));
    CREATE_TRY(dalloc(b, &D.err, R));
    CREATE_TRY(dalloc(b, &D.aux, R));
    CREATE_TRY(dalloc(b, &D.epoch, R));
    CREATE_TRY(dalloc(b, &D.acc, R * 8));
    b->acc_rows = D.R;
    std::vector<uint32_t> ident(R);
    for (uint32_t i = 0; i < R; ++i) ident[i] = i;
    CREATE_TRY(dalloc(b, &b->d_acc_row, R));
    CREATE_TRY(copy_up(b, b->d_acc_row, ident.data(), R, "acc_row"));
    D.acc_row = b->d_acc_row;
    CREATE_TRY(dalloc(b, &D.chunks, R * 2 * SSE_MAX_CHUNKS));
    CREATE_TRY(dalloc(b, &D.segs, R * D.stride, false));
    if (b->defer) { // flip bytes start (and stay, beyond every cutoff) zero
        CREATE_TRY(dalloc(b, &D.flipb, R * D.stride));
        CREATE_TRY(dalloc(b, &D.pend, R));
    }
    CREATE_TRY(dalloc(b, &D.dbg, R * 16));
    if (D.bond_stride) CREATE_TRY(upload(b, D.wtot_r, T.wtots, "weight"));
    CREATE_TRY(upload(b, D.edge_w, T.edge_w, "edge table"));
    CREATE_TRY(upload(b, D.edges_compact, T.edges_compact, "edge table"));
    if (is_pm(b)) CREATE_TRY(upload(b, D.pm_signs, T.signs, "sign")); // coupling signs of every bond-table row
    CREATE_TRY(upload(b, D.adj_start, T.adj_start, "adjacency"));
    CREATE_TRY(upload(b, D.adj, T.adj, "adjacency"));
    CREATE_TRY(dalloc(b, &D.uf_scratch, R * plan.ufstride, false));
    if (plan.tbl_stride) CREATE_TRY(dalloc(b, &D.tbl, R * D.tbl_stride));
    CREATE_TRY(dalloc(b, &b->d_beta, R));
    CREATE_TRY(dalloc(b, &b->d_out, R));
    CREATE_TRY(dalloc(b, &b->d_vstate, R * D.nwords));
    CREATE_TRY(dalloc(b, &b->d_ok, R));
    CREATE_TRY(upload(b, D.bonds, T.bonds, "table"));
    CREATE_TRY(upload(b, D.cumw, T.cum, "table"));
    if (b->generic) CREATE_TRY(upload(b, D.mats, T.mats, "matrix"));
    b->bonds_host = std::move(T.bonds); b->mats_host = std::move(T.mats); // (import_ops, tempering)
    CREATE_TRY(copy_up(b, D.cutoff, std::vector<uint32_t>(R, cfg->cutoff0).data(), R, "cutoff"));
    if (hipEventCreate(&b->ev0) != hipSuccess || hipEventCreate(&b->ev1) != hipSuccess) { b->err = "hipEventCreate failed"; return ISINGMC_ENODEVICE; }
    if (cfg->init_state) return isingmc_set_state(b, UINT32_MAX, cfg->init_state);
    hipLaunchKernelGGL(init_state_kernel, dim3(D.R), dim3(64), 0, b->stream, D);
    if (hipDeviceSynchronize() != hipSuccess) { b->err = "init_state_kernel failed"; return ISINGMC_ENODEVICE; }
    return ISINGMC_OK;
}
#undef CREATE_TRY

extern "C" {

int isingmc_interaction_at(const isingmc_interaction *it, const uint8_t *inputs, const uint8_t *outputs, double *out) {
    if (!it || !it->mat || !inputs || !outputs || !out || it->nvars == 0 || it->nvars > 2) return ISINGMC_EINVAL;
    // index_from_state (qmc_runner.rs:666-679): outputs then inputs, first variable most significant
    uint32_t iin = 0, iout = 0;
    for (uint32_t k = 0; k < it->nvars; ++k) { iin = (iin << 1) | (inputs[k] ? 1u : 0u); iout = (iout << 1) | (outputs[k] ? 1u : 0u); }
    if (it->diagonal_only) *out = (iin == iout) ? it->mat[iin] : 0.0;
    else *out = it->mat[(iout << it->nvars) | iin];
    return ISINGMC_OK;
}
int isingmc_interaction_sym_under_ising(const isingmc_interaction *it, int *out) {
    if (!it || !it->mat || !out || it->nvars == 0 || it->nvars > 2) return ISINGMC_EINVAL;
    const uint32_t n = it->nvars;
    const uint32_t mask = it->diagonal_only ? ((1u << n) - 1u) : ((1u << (2 * n)) - 1u);
    const uint32_t upto = it->diagonal_only ? (1u << (n >> 1)) : (1u << n);
    int sym = 1;
    for (uint32_t i = 0; i < upto; ++i)
        if (!(std::fabs(it->mat[i] - it->mat[(~i) & mask]) < DBL_EPSILON)) sym = 0;
    *out = sym;
    return ISINGMC_OK;
}

// Chunk grid of the per-chunk counters and the row stride of the op-string (and of every per-slot scratch row) for a batch whose
// kernels run with W waves (diagonal launches) and up to Wmax waves (off-diagonal launches) of K slots per lane.
//   CH      chunk size: <= SSE_MAX_CHUNKS chunks cover the capacity, CH a multiple of 256 (= a wave's tile at K = 4, two at K = 2)
//   stride  whole tiles of EITHER geometry (full-tile loads and stores never leave the row) and at least the chunk-rounded
//           capacity + 256: a cluster-scan wave whose chunk range is empty still prefetches one wave-tile at its range start
int isingmc_plan_geometry(uint32_t capacity, uint32_t W, uint32_t K, uint32_t Wmax, uint32_t out[4]) {
    if (!out || capacity == 0 || W == 0 || K == 0 || Wmax < W) return ISINGMC_EINVAL;
    const size_t CH = (((size_t)capacity + SSE_MAX_CHUNKS - 1) / SSE_MAX_CHUNKS + 255) / 256 * 256;
    const size_t nchunks = ((size_t)capacity + CH - 1) / CH;
    const size_t tile = (Wmax % W == 0 ? (size_t)Wmax : (size_t)Wmax * W) * 64 * K; // whole tiles of either launch geometry
    const size_t need1 = ((size_t)capacity + tile - 1) / tile * tile;
    const size_t need2 = ((size_t)capacity + CH - 1) / CH * CH + 256;
    const size_t need = need1 > need2 ? need1 : need2;
    const size_t stride = (need + tile - 1) / tile * tile;
    if (stride > 0xFFFFFFFFull / 4) return ISINGMC_EINVAL; // byte offsets inside a row are 32-bit (row_ld / row_st)
    out[0] = (uint32_t)CH; out[1] = (uint32_t)nchunks; out[2] = (uint32_t)stride; out[3] = (uint32_t)tile;
    return ISINGMC_OK;
}

int isingmc_create(const isingmc_config *cfg, isingmc_batch **out) {
    if (!cfg || !out || cfg->struct_size != sizeof(isingmc_config)) return refuse(ISINGMC_EINVAL, "bad config pointer or struct_size");
    *out = nullptr;
    if (const int rc = check_config(cfg)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return refuse(ISINGMC_ENODEVICE, "no HIP device available (this library has no CPU fallback)");
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (hipSetDevice(dev) != hipSuccess) return refuse(ISINGMC_ENODEVICE, "hipSetDevice failed");
    int max_lds = 0;
    if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || max_lds <= 0) max_lds = 65536;
    DevBatch model; Tables tables; BatchPlan plan;
    if (const int rc = plan_config(cfg, (uint32_t)max_lds, model, tables, plan)) return rc;
    isingmc_batch *b = new isingmc_batch();
    b->device = dev;
    if (const int rc = allocate_and_upload(b, cfg, model, tables, plan)) { g_create_error = b->err; isingmc_destroy(b); return rc; }
    *out = b;
    return ISINGMC_OK;
}

// The plan isingmc_create would make for cfg on a device whose workgroups have lds_bytes of LDS, or the code and message it would
// refuse cfg with.  Host only: no device is looked for, nothing is allocated.  Slots: include/isingmc_hip.h.
int isingmc_plan_batch(const isingmc_config *cfg, uint32_t lds_bytes, uint32_t out[32]) {
    if (!cfg || !out || cfg->struct_size != sizeof(isingmc_config)) return refuse(ISINGMC_EINVAL, "bad config pointer or struct_size");
    if (const int rc = check_config(cfg)) return rc;
    DevBatch model; Tables tables; BatchPlan p;
    if (const int rc = plan_config(cfg, lds_bytes, model, tables, p)) return rc;
    const uint32_t slots[32] = {p.W, p.K, p.mode, p.W_off, p.Wmax, p.w8_ok, p.CH, p.nchunks, p.stride, p.pm_words, (uint32_t)p.lds_words_pm_diag,
                                (uint32_t)p.lds_words_diag, (uint32_t)p.lds_words_fast, p.fast_diag, p.lean_cluster, p.defer, (uint32_t)p.lds_words_rvb,
                                p.rvb_global, p.rvb_split, p.rvb_main_W, p.tbl_stride, (uint32_t)p.ufstride, (uint32_t)((uint64_t)p.ufstride >> 32),
                                (uint32_t)p.lds_words, p.lds_ufcap, model.nwords, model.Nb};
    std::copy(slots, slots + 32, out);
    return ISINGMC_OK;
}

void isingmc_destroy(isingmc_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    pt_free(b);
    for (void *p : b->allocs) (void)hipFree(p);
    if (b->dev.rvb_prod) (void)hipFree(b->dev.rvb_prod);
    if (b->dev.rvb_tbl) (void)hipFree(b->dev.rvb_tbl);
    for (void *p : {(void *)b->rec, b->obs_groups, b->obs_series, b->obs_out}) if (p) (void)hipFree(p);
    for (hipEvent_t ev : b->evpool) (void)hipEventDestroy(ev);
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    delete b;
}

const char *isingmc_last_error(const isingmc_batch *b) { return b ? b->err.c_str() : g_create_error.c_str(); }

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

int isingmc_get_accumulators(isingmc_batch *b, uint64_t *out) {
    if (!b || !out) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipMemcpy(out, b->dev.acc, sizeof(uint64_t) * 8 * b->acc_rows, hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}
int isingmc_set_accumulators(isingmc_batch *b, const uint64_t *in) {
    if (!b || !in) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    HIP_TRY(b, hipMemcpy(b->dev.acc, in, sizeof(uint64_t) * 8 * b->acc_rows, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}
int isingmc_clear_errors(isingmc_batch *b) {
    if (!b) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    HIP_TRY(b, hipMemset(b->dev.err, 0, sizeof(uint32_t) * b->dev.R));
    b->err.clear();
    return ISINGMC_OK;
}
int isingmc_reset_accumulators(isingmc_batch *b) {
    if (!b) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipMemset(b->dev.acc, 0, sizeof(uint64_t) * 8 * b->acc_rows));
    return ISINGMC_OK;
}
int isingmc_set_accumulator_rows(isingmc_batch *b, uint32_t nrows, const uint32_t *rows) {
    if (!b || !rows || nrows == 0) return ISINGMC_EINVAL;
    for (uint32_t r = 0; r < b->dev.R; ++r) if (rows[r] >= nrows) { b->err = "accumulator row out of range"; return ISINGMC_EINVAL; }
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    if (nrows != b->acc_rows) {
        uint64_t *na = nullptr;
        int rc = dalloc(b, &na, (size_t)nrows * 8);
        if (rc) return rc;
        b->dev.acc = na; // the previous table stays in the allocation list until destroy
        b->acc_rows = nrows;
    }
    HIP_TRY(b, hipMemcpy(b->d_acc_row, rows, sizeof(uint32_t) * b->dev.R, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}
int isingmc_set_cutoffs(isingmc_batch *b, const uint32_t *cutoffs) {
    if (!b || !cutoffs) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    std::vector<uint32_t> cur(b->dev.R);
    HIP_TRY(b, hipMemcpy(cur.data(), b->dev.cutoff, sizeof(uint32_t) * b->dev.R, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < b->dev.R; ++r) {
        if (cutoffs[r] > b->dev.cap) { b->err = "cutoff exceeds capacity"; return ISINGMC_ECAPACITY; }
        if (cutoffs[r] > cur[r]) cur[r] = cutoffs[r]; // fast_ops.rs:1258-1262: only grows
    }
    HIP_TRY(b, hipMemcpy(b->dev.cutoff, cur.data(), sizeof(uint32_t) * b->dev.R, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}
double isingmc_get_offset(const isingmc_batch *b) { return b ? b->offset : 0.0; }
int isingmc_get_offsets(const isingmc_batch *b, double *out) {
    if (!b || !out) return ISINGMC_EINVAL;
    for (uint32_t r = 0; r < b->dev.R; ++r) out[r] = b->per_replica_J ? b->offsets[b->ham_row_host.empty() ? r : b->ham_row_host[r]] : b->offset;
    return ISINGMC_OK;
}
uint32_t isingmc_num_bonds(const isingmc_batch *b) { return b ? b->dev.Nb : 0u; }

int isingmc_get_state(isingmc_batch *b, uint32_t r, uint8_t *out) {
    if (!b || !out || (r != UINT32_MAX && r >= b->dev.R)) { if (b) b->err = "bad replica index"; return ISINGMC_EINVAL; }
    HIP_TRY(b, hipSetDevice(b->device));
    const uint32_t r0 = r == UINT32_MAX ? 0 : r, cnt = r == UINT32_MAX ? b->dev.R : 1;
    std::vector<uint32_t> w((size_t)cnt * b->dev.nwords);
    HIP_TRY(b, hipMemcpy(w.data(), b->dev.state + (size_t)r0 * b->dev.nwords, w.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < cnt; ++i)
        for (uint32_t v = 0; v < b->dev.N; ++v) out[(size_t)i * b->dev.N + v] = (w[(size_t)i * b->dev.nwords + (v >> 5)] >> (v & 31)) & 1u;
    return ISINGMC_OK;
}
int isingmc_set_state(isingmc_batch *b, uint32_t r, const uint8_t *in) {
    if (!b || !in || (r != UINT32_MAX && r >= b->dev.R)) { if (b) b->err = "bad replica index"; return ISINGMC_EINVAL; }
    HIP_TRY(b, hipSetDevice(b->device));
    const uint32_t r0 = r == UINT32_MAX ? 0 : r, cnt = r == UINT32_MAX ? b->dev.R : 1;
    std::vector<uint32_t> w((size_t)cnt * b->dev.nwords, 0u);
    for (uint32_t i = 0; i < cnt; ++i)
        for (uint32_t v = 0; v < b->dev.N; ++v)
            if (in[(size_t)i * b->dev.N + v]) w[(size_t)i * b->dev.nwords + (v >> 5)] |= 1u << (v & 31);
    HIP_TRY(b, hipMemcpy(b->dev.state + (size_t)r0 * b->dev.nwords, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}

static int get_u32(isingmc_batch *b, const uint32_t *src, uint32_t *out) {
    if (!b || !out) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipMemcpy(out, src, sizeof(uint32_t) * b->dev.R, hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}
int isingmc_get_n(isingmc_batch *b, uint32_t *out) { return b ? get_u32(b, b->dev.n, out) : ISINGMC_EINVAL; }
int isingmc_get_cutoff(isingmc_batch *b, uint32_t *out) { return b ? get_u32(b, b->dev.cutoff, out) : ISINGMC_EINVAL; }
int isingmc_get_epoch(isingmc_batch *b, uint64_t *out) {
    if (!b || !out) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipMemcpy(out, b->dev.epoch, sizeof(uint64_t) * b->dev.R, hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}
int isingmc_set_epoch(isingmc_batch *b, const uint64_t *epochs) {
    if (!b || !epochs) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipMemcpy(b->dev.epoch, epochs, sizeof(uint64_t) * b->dev.R, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}
int isingmc_set_cutoff(isingmc_batch *b, uint32_t r, uint32_t cutoff) {
    if (!b || r >= b->dev.R) { if (b) b->err = "bad replica index"; return ISINGMC_EINVAL; }
    if (cutoff > b->dev.cap) { b->err = "cutoff exceeds capacity"; return ISINGMC_ECAPACITY; }
    HIP_TRY(b, hipSetDevice(b->device));
    uint32_t cur = 0;
    HIP_TRY(b, hipMemcpy(&cur, b->dev.cutoff + r, 4, hipMemcpyDeviceToHost));
    if (cutoff > cur) HIP_TRY(b, hipMemcpy(b->dev.cutoff + r, &cutoff, 4, hipMemcpyHostToDevice)); // fast_ops.rs:1258-1262: only grows
    return ISINGMC_OK;
}

int isingmc_export_ops(isingmc_batch *b, uint32_t r, uint32_t *words, uint32_t nwords) {
    if (!b || !words || r >= b->dev.R || nwords > b->dev.cap) { if (b) b->err = "bad arguments to export_ops"; return ISINGMC_EINVAL; }
    HIP_TRY(b, hipSetDevice(b->device));
    { const int rcm = ensure_materialized(b); if (rcm) return rcm; }
    HIP_TRY(b, hipMemcpy(words, b->dev.ops + (size_t)r * b->dev.stride, sizeof(uint32_t) * nwords, hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}
int isingmc_import_ops(isingmc_batch *b, uint32_t r, const uint32_t *words, uint32_t nwords) {
    if (!b || (!words && nwords) || r >= b->dev.R) { if (b) b->err = "bad arguments to import_ops"; return ISINGMC_EINVAL; }
    if (nwords > b->dev.cap) { b->err = "op-string longer than capacity"; return ISINGMC_ECAPACITY; }
    { const int rcm = ensure_materialized(b); if (rcm) return rcm; }
    uint32_t n = 0, ntr = 0;
    const size_t hoff = b->per_replica_J ? (size_t)(b->ham_row_host.empty() ? r : b->ham_row_host[r]) * b->dev.Nb : 0; // this replica's bond table
    std::vector<uint32_t> chunks(2 * SSE_MAX_CHUNKS, 0u);
    for (uint32_t p = 0; p < nwords; ++p) {
        if (!words[p]) continue;
        const uint32_t bond = sse_op_bond(words[p]);
        if (bond >= b->dev.Nb) { b->err = "op refers to a bond outside the model"; return ISINGMC_EINVAL; }
        // Ising bonds: two-site and longitudinal ops have zero off-diagonal weight (qmc_ising.rs:863-888)
        const uint32_t kind = (b->bonds_host[hoff + bond].a_info >> SSE_INFO_SHIFT) & SSE_BOND_KIND_MASK;
        if (b->generic) {
            if (!(b->mats_host[(size_t)bond * 16 + (sse_op_in(words[p]) | (sse_op_out(words[p]) << 2))] > 0.0)) { b->err = "op with zero weight"; return ISINGMC_EINVAL; }
        } else
        if (kind != SSE_BOND_TRANSVERSE && sse_op_in(words[p]) != sse_op_out(words[p])) { b->err = "off-diagonal op on a diagonal-only bond (zero weight)"; return ISINGMC_EINVAL; }
        if (b->bonds_host[hoff + bond].c == SSE_NO_VAR && ((sse_op_in(words[p]) | sse_op_out(words[p])) & 2u)) { b->err = "single-site op with second-variable bits set"; return ISINGMC_EINVAL; }
        n++;
        chunks[p / b->dev.CH]++;
        if (((b->bonds_host[hoff + bond].a_info >> SSE_INFO_SHIFT) & SSE_BOND_KIND_MASK) == SSE_BOND_TRANSVERSE) { ntr++; chunks[SSE_MAX_CHUNKS + p / b->dev.CH]++; }
    }
    HIP_TRY(b, hipSetDevice(b->device));
    uint32_t *dst = b->dev.ops + (size_t)r * b->dev.stride;
    HIP_TRY(b, hipMemset(dst, 0, sizeof(uint32_t) * b->dev.stride));
    if (nwords) HIP_TRY(b, hipMemcpy(dst, words, sizeof(uint32_t) * nwords, hipMemcpyHostToDevice));
    uint32_t cur = 0;
    HIP_TRY(b, hipMemcpy(&cur, b->dev.cutoff + r, 4, hipMemcpyDeviceToHost));
    if (nwords > cur) HIP_TRY(b, hipMemcpy(b->dev.cutoff + r, &nwords, 4, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(b->dev.n + r, &n, 4, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(b->dev.ntrans + r, &ntr, 4, hipMemcpyHostToDevice));
    { const uint32_t zero = 0; HIP_TRY(b, hipMemcpy(b->dev.err + r, &zero, 4, hipMemcpyHostToDevice)); } // a fresh op-string: the replica's sticky error flag no longer applies
    if (ntr > b->max_ntrans) b->max_ntrans = ntr;
    HIP_TRY(b, hipMemcpy(b->dev.chunks + (size_t)r * 2 * SSE_MAX_CHUNKS, chunks.data(), sizeof(uint32_t) * chunks.size(), hipMemcpyHostToDevice));
    return ISINGMC_OK;
}
int isingmc_itime_magnetization(isingmc_batch *b, int64_t *sum_m, uint64_t *sum_m2, uint64_t *sum_abs_m) {
    if (!b || !sum_m || !sum_m2 || !sum_abs_m) { if (b) b->err = "bad arguments to itime_magnetization"; return ISINGMC_EINVAL; }
    HIP_TRY(b, hipSetDevice(b->device));
    { const int rcm = ensure_materialized(b); if (rcm) return rcm; }
    const uint32_t R = b->dev.R;
    long long *d1 = nullptr; unsigned long long *d2 = nullptr, *d3 = nullptr;
    HIP_TRY(b, hipMalloc(&d1, sizeof(long long) * R));
    if (hipMalloc(&d2, sizeof(unsigned long long) * R) != hipSuccess || hipMalloc(&d3, sizeof(unsigned long long) * R) != hipSuccess) {
        (void)hipFree(d1); if (d2) (void)hipFree(d2);
        b->err = "itime_magnetization: allocation failed"; return ISINGMC_ENODEVICE;
    }
    hipLaunchKernelGGL(itime_magnetization_kernel, dim3(R), dim3(256), 0, b->stream, b->dev, d1, d2, d3);
    hipError_t e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(sum_m, d1, sizeof(long long) * R, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(sum_m2, d2, sizeof(unsigned long long) * R, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(sum_abs_m, d3, sizeof(unsigned long long) * R, hipMemcpyDeviceToHost);
    (void)hipFree(d1); (void)hipFree(d2); (void)hipFree(d3);
    if (e != hipSuccess) { b->err = std::string("itime_magnetization: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    return ISINGMC_OK;
}
int isingmc_get_bond_count(isingmc_batch *b, uint32_t r, uint32_t bond, uint32_t *out) {
    if (!b || !out || r >= b->dev.R) { if (b) b->err = "bad arguments to get_bond_count"; return ISINGMC_EINVAL; }
    std::vector<uint32_t> w(b->dev.cap);
    int rc = isingmc_export_ops(b, r, w.data(), b->dev.cap);
    if (rc) return rc;
    uint32_t c = 0;
    for (uint32_t x : w) if (x && sse_op_bond(x) == bond) c++;
    *out = c;
    return ISINGMC_OK;
}

int isingmc_debug_counts(isingmc_batch *b, uint32_t *out) {
    if (!b || !out) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    { const int rcm = ensure_materialized(b); if (rcm) return rcm; }
    uint32_t *d = nullptr;
    HIP_TRY(b, hipMalloc((void **)&d, 12 * (size_t)b->dev.R));
    hipLaunchKernelGGL(debug_counts_kernel, dim3(b->dev.R), dim3(256), 0, b->stream, b->dev, d);
    hipError_t e = hipMemcpyAsync(out, d, 12 * (size_t)b->dev.R, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    (void)hipFree(d);
    if (e != hipSuccess) { b->err = std::string("debug_counts: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    return ISINGMC_OK;
}

int isingmc_verify(isingmc_batch *b, uint8_t *ok) {
    if (!b || !ok) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    { const int rcm = ensure_materialized(b); if (rcm) return rcm; }
    hipLaunchKernelGGL(verify_kernel, dim3((b->dev.R + 63) / 64), dim3(64), 0, b->stream, b->dev, b->d_vstate, b->d_ok);
    HIP_TRY(b, hipGetLastError());
    HIP_TRY(b, hipMemcpyAsync(ok, b->d_ok, b->dev.R, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    return ISINGMC_OK;
}

int isingmc_set_stream(isingmc_batch *b, void *hip_stream) {
    if (!b) return ISINGMC_EINVAL;
    b->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return ISINGMC_OK;
}
int isingmc_debug_phase_ticks(isingmc_batch *b, uint64_t *out /*[R][16]*/, int reset) {
    if (!b || !out) return ISINGMC_EINVAL;
    if (reset >= 16) { b->dev.dbg_flags = (uint32_t)reset >> 4; reset &= 1; } // diagnostic builds: experiment flags
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipMemcpy(out, b->dev.dbg, sizeof(uint64_t) * 16 * b->dev.R, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(b, hipMemset(b->dev.dbg, 0, sizeof(uint64_t) * 16 * b->dev.R));
    return ISINGMC_OK;
}
int isingmc_set_steps_per_launch(isingmc_batch *b, uint64_t steps) {
    if (!b) return ISINGMC_EINVAL;
    b->steps_per_launch = steps;
    return ISINGMC_OK;
}
int isingmc_synchronize(isingmc_batch *b) {
    if (!b) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    return ISINGMC_OK;
}
int isingmc_last_kernel_ms(isingmc_batch *b, float *ms, uint32_t *launches) {
    if (!b) return ISINGMC_EINVAL;
    if (ms) *ms = b->last_ms;
    if (launches) *launches = b->last_launches;
    return ISINGMC_OK;
}
int isingmc_last_pass_ms(isingmc_batch *b, float ms[2], uint32_t launches[2]) {
    if (!b) return ISINGMC_EINVAL;
    if (ms) { ms[0] = b->pass_ms[0]; ms[1] = b->pass_ms[1]; }
    if (launches) { launches[0] = b->pass_launches[0]; launches[1] = b->pass_launches[1]; }
    return ISINGMC_OK;
}
int isingmc_last_rvb_ms(isingmc_batch *b, float *ms, uint32_t *launches) {
    if (!b) return ISINGMC_EINVAL;
    if (ms) *ms = b->pass_ms[2];
    if (launches) *launches = b->pass_launches[2];
    return ISINGMC_OK;
}
int isingmc_get_launch_info(const isingmc_batch *b, uint32_t out[8]) {
    if (!b || !out) return ISINGMC_EINVAL;
    out[0] = b->W; out[1] = (uint32_t)lds_bytes_of(b->lds_words); out[2] = b->dev.lds_ufcap; out[3] = b->dev.nwords;
    out[4] = b->K; out[5] = b->mode == SSE_MODE_LDS_EDGES ? 1u : 0u; out[6] = (b->fused_launch ? 0u : 1u) | (b->last_W_off << 8) | (is_tg(b) ? 2u : 0u) | (b->fast_diag ? 4u : 0u) | (b->last_lean ? 32u : 0u) | (b->last_rvb_split ? 64u : 0u) | (b->last_rvb_global ? 128u : 0u) | ((b->last_rvb_split ? b->rvb_main_W : 0u) << 16); out[7] = (uint32_t)lds_bytes_of(b->lds_words_diag);
    return ISINGMC_OK;
}

} // extern "C"
