// pt.hip — native parallel tempering of the C ABI (include/isingmc_hip.h, isingmc_pt_*)
// (reference: TemperingContainer::tempering_step, parallel_tempering/tempering_container.rs:121-149,
// perform_swaps / swap_on_chunks :241-302, GraphWeights::relative_weight tempering_traits.rs:126-155).
//
// Sharding: rank g of G owns a contiguous block of ntemps/G temperatures for every chain ("walker").  Inside a block a swap
// exchanges temperature LABELS of two local replicas (slot_of); at a block boundary the two ranks exchange the boundary
// walkers' operator counts (4 B per chain and phase, ncclSend / ncclRecv in one group), both evaluate the same Philox-keyed
// decision, and an accepted swap moves the two configurations (op-string up to the cutoff, p=0 state, counters, Philox
// identity) through one more grouped send / receive.  Every rank therefore always holds exactly the configurations of its own
// temperature block, and no collective touches the sweep path.  The transport is RCCL point-to-point on device buffers when a
// communicator is attached (isingmc_pt_attach_nccl), otherwise the caller's host-staged sendrecv (tests: two ranks on one GPU).
#include "batch.hip.h"
#include "sse_core.hip.h" // philox4x32_10

#include <cfloat>
#include <cmath>
#include <utility>
#include <dlfcn.h>
#include <rccl/rccl.h> // types and enum values only (ncclUint32, ncclMax, ncclUniqueId): the library itself is dlopen()ed on first use
static_assert(sizeof(ncclUniqueId) == sizeof(isingmc_nccl_id), "isingmc_nccl_id must carry an ncclUniqueId");

using namespace sse;

struct PtState {
    uint32_t ntemps = 0, nchains = 0, rank = 0, world = 1, tper = 0;
    std::vector<double> betas;
    uint64_t seed = 0, step = 0, total_swaps = 0;
    std::vector<uint32_t> slot_of; // [R] global slot t*nchains + chain labelling local replica r
    std::vector<uint32_t> rid;     // [R] configuration identity (global id it was created with)
    uint32_t *d_rid = nullptr, *d_ham_row = nullptr;
    isingmc_pt_transport tr{};
    bool have_tr = false;
    // RCCL, loaded on first use
    void *nccl_lib = nullptr, *comm = nullptr;
    int (*p_send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*p_recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*p_gstart)() = nullptr;
    int (*p_gend)() = nullptr;
    int (*p_allreduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*p_init)(void **, int, isingmc_nccl_id, int) = nullptr;
    int (*p_destroy)(void *) = nullptr;
    // decisions on the device (single rank, one Hamiltonian for all temperatures): labels, betas per replica and the swap count live
    // in device memory; the host mirrors (slot_of) are refreshed on demand
    bool dev_decide = false, host_stale = false;
    uint32_t *d_slot_of = nullptr, *d_at = nullptr, *d_result = nullptr; // d_result: [0] swaps of the last step, [1] error flag
    double *d_betas = nullptr, *d_beta_r = nullptr;
    unsigned long long *d_total = nullptr; // total swaps since isingmc_pt_create / set_state
    uint32_t *d_items = nullptr; // [3 * nchains] accepted boundary swaps of one turn: (replica, word offset, cutoff)
    uint32_t *d_small = nullptr; // [4][nchains] staging of the boundary operator counts / cutoffs on the device (RCCL path)
    // different Hamiltonians per temperature (per-replica couplings): J rows of the neighbouring ranks' boundary slots
    bool hams_differ = false;
    std::vector<double> J_prev_last, J_next_first; // [nchains][E]
    uint32_t *d_counts = nullptr;                  // [R][Nb] bond counts (only when hams_differ)
    // configuration exchange
    uint32_t *d_pack_s = nullptr, *d_pack_r = nullptr;
    size_t pack_cap_words = 0;
    std::vector<uint32_t> h_pack_s, h_pack_r;
};

void sse::pt_free(isingmc_batch *b) {
    if (!b->pt) return;
    PtState *P = b->pt;
    if (P->comm && P->p_destroy) (void)P->p_destroy(P->comm);
    for (void *q : {(void *)P->d_rid, (void *)P->d_ham_row, (void *)P->d_small, (void *)P->d_counts, (void *)P->d_pack_s, (void *)P->d_pack_r, (void *)P->d_items,
                    (void *)P->d_slot_of, (void *)P->d_at, (void *)P->d_result, (void *)P->d_betas, (void *)P->d_beta_r, (void *)P->d_total})
        if (q) (void)hipFree(q);
    delete P;
    b->pt = nullptr;
}

// Host-side Philox4x32-10 for the tempering decisions (control logic, not the sweep path).
static void host_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// f64::powi as Rust lowers it (compiler-rt __powidf2): squaring sequence, reciprocal for negative exponents.  Multiplications
// and one division only: the host and the device give the same bits (as does the oracle, which multiplies in the same order)
__host__ __device__ static inline double pt_powi(double x, int64_t n) {
    uint64_t m = n < 0 ? (uint64_t)(-n) : (uint64_t)n;
    double r = 1.0;
    while (m) { if (m & 1u) r *= x; x *= x; m >>= 1; }
    return n < 0 ? 1.0 / r : r;
}
// The swap test of a pair of neighbouring temperatures t, t + 1 (swap_on_chunks, tempering_container.rs:296-298): the walker at t
// holds n_a ops, the one at t + 1 n_b; rel = the product of their relative weights under each other's Hamiltonian (1 when the
// Hamiltonians are equal: a multiplication by 1.0 changes no bit); u uniform in [0, 1)
__host__ __device__ static inline bool pt_accept(double beta_t, double beta_t1, uint32_t n_a, uint32_t n_b, double rel, double u) {
    return pt_powi(beta_t / beta_t1, (int64_t)n_b - (int64_t)n_a) * rel > u;
}

// pack / unpack one configuration per workgroup: header (n, ntrans, cutoff, err, epoch lo/hi, rid, 0), p=0 state, chunk counters, op words
#define PT_HDR 8u
__global__ void pt_pack_kernel(DevBatch B, const uint32_t *rid, const uint32_t *items /*[nitems][3]: replica, word offset, cutoff*/, uint32_t *buf) {
    const uint32_t r = items[3 * blockIdx.x], off = items[3 * blockIdx.x + 1], cut = items[3 * blockIdx.x + 2];
    uint32_t *o = buf + off;
    if (threadIdx.x == 0) {
        o[0] = B.n[r]; o[1] = B.ntrans[r]; o[2] = B.cutoff[r]; o[3] = B.err[r];
        o[4] = (uint32_t)B.epoch[r]; o[5] = (uint32_t)(B.epoch[r] >> 32); o[6] = rid[r]; o[7] = 0u;
    }
    for (uint32_t i = threadIdx.x; i < B.nwords; i += blockDim.x) o[PT_HDR + i] = B.state[(size_t)r * B.nwords + i];
    for (uint32_t i = threadIdx.x; i < 2 * SSE_MAX_CHUNKS; i += blockDim.x) o[PT_HDR + B.nwords + i] = B.chunks[(size_t)r * 2 * SSE_MAX_CHUNKS + i];
    const uint32_t *ops = B.ops + (size_t)r * B.stride;
    for (uint32_t i = threadIdx.x; i < cut; i += blockDim.x) o[PT_HDR + B.nwords + 2 * SSE_MAX_CHUNKS + i] = ops[i];
}
__global__ void pt_unpack_kernel(DevBatch B, uint32_t *rid, const uint32_t *items, const uint32_t *buf) {
    const uint32_t r = items[3 * blockIdx.x], off = items[3 * blockIdx.x + 1], cut = items[3 * blockIdx.x + 2];
    const uint32_t *o = buf + off;
    if (threadIdx.x == 0) {
        B.n[r] = o[0]; B.ntrans[r] = o[1]; B.cutoff[r] = o[2]; B.err[r] = o[3];
        B.epoch[r] = (uint64_t)o[4] | ((uint64_t)o[5] << 32); rid[r] = o[6];
    }
    for (uint32_t i = threadIdx.x; i < B.nwords; i += blockDim.x) B.state[(size_t)r * B.nwords + i] = o[PT_HDR + i];
    for (uint32_t i = threadIdx.x; i < 2 * SSE_MAX_CHUNKS; i += blockDim.x) B.chunks[(size_t)r * 2 * SSE_MAX_CHUNKS + i] = o[PT_HDR + B.nwords + i];
    uint32_t *ops = B.ops + (size_t)r * B.stride;
    for (uint32_t i = threadIdx.x; i < cut; i += blockDim.x) ops[i] = o[PT_HDR + B.nwords + 2 * SSE_MAX_CHUNKS + i];
}
// OpContainer::get_count for every bond of every replica (op_container.rs:129): counts[r][bond]
__global__ void pt_bond_count_kernel(DevBatch B, uint32_t *counts) {
    const uint32_t r = blockIdx.x;
    const uint32_t *ops = B.ops + (size_t)r * B.stride;
    uint32_t *c = counts + (size_t)r * B.Nb;
    for (uint32_t i = threadIdx.x; i < B.Nb; i += blockDim.x) c[i] = 0u;
    __syncthreads();
    const uint32_t M = B.cutoff[r];
    for (uint32_t p = threadIdx.x; p < M; p += blockDim.x) { const uint32_t w = ops[p]; if (w) atomicAdd(&c[sse_op_bond(w)], 1u); }
}

struct PtDev {
    uint32_t *slot_of, *at, *result, *acc_row;
    const double *betas;
    double *beta_r;
    unsigned long long *total;
    uint32_t K, T, key0, key1;
    uint64_t step;
};
// One tempering step of a rank that owns all temperatures (tempering_container.rs:121-149; the decisions of isingmc_pt_step's host
// path, same Philox counters): thread k takes chain k — equalise its cutoffs, draw the order coin, walk the two sets of pairs.
__global__ void pt_decide_kernel(DevBatch B, PtDev P) {
    __shared__ unsigned int s_swaps;
    if (threadIdx.x == 0) s_swaps = 0u;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < P.K; k += blockDim.x) {
        uint32_t maxcut = 0;
        for (uint32_t t = 0; t < P.T; ++t) { const uint32_t c = B.cutoff[P.at[t * P.K + k]]; maxcut = c > maxcut ? c : maxcut; }
        if (maxcut > B.cap) { P.result[1] = 1u; continue; }
        for (uint32_t t = 0; t < P.T; ++t) B.cutoff[P.at[t * P.K + k]] = maxcut;
        const uint32_t c3 = (SSE_TAG_PT << 24) | (uint32_t)((P.step >> 32) & 0xFFFFFFu);
        const bool a_first = (philox4x32_10(0u, (uint32_t)P.step, k, c3, P.key0, P.key1).x >> 31) != 0u;
        uint32_t swaps = 0;
        for (int phase = 0; phase < 2; ++phase) {
            const bool set_a = (phase == 0) ? a_first : !a_first;
            for (uint32_t t = 0; t + 1 < P.T; ++t) {
                if ((((t & 1u) == 0u) != set_a)) continue;
                const uint32_t la = t * P.K + k, lb = la + P.K;
                const uint32_t ra = P.at[la], rb = P.at[lb];
                const double u = (double)philox4x32_10(1u + t, (uint32_t)P.step, k, c3, P.key0, P.key1).x * (1.0 / 4294967296.0);
                if (pt_accept(P.betas[t], P.betas[t + 1], B.n[ra], B.n[rb], 1.0, u)) { P.slot_of[ra] = lb; P.slot_of[rb] = la; P.at[la] = rb; P.at[lb] = ra; swaps++; }
            }
        }
        for (uint32_t t = 0; t < P.T; ++t) {
            const uint32_t r = P.at[t * P.K + k];
            P.beta_r[r] = P.betas[t];
            if (P.acc_row) P.acc_row[r] = t * P.K + k;
        }
        if (swaps) atomicAdd(&s_swaps, swaps);
    }
    __syncthreads();
    if (threadIdx.x == 0) { P.result[0] = s_swaps; *P.total += s_swaps; }
}

// GraphWeights::relative_weight (tempering_traits.rs:126-155): the weight of a configuration under the Hamiltonian `to` relative
// to the one it lives in (`from`).  Rows are [E] couplings, then Gamma, then h: product over the edges of (J_to / J_from)^count in
// edge order, times (Gamma_to / Gamma_from)^(transverse ops), times (h_to / h_from)^(longitudinal ops) when h_from != 0
static double pt_relative_weight(const double *from, const double *to, const uint32_t *counts, uint32_t E, uint32_t N, bool has_long) {
    double w = 1.0;
    for (uint32_t e = 0; e < E; ++e) w *= pt_powi(to[e] / from[e], counts[e]);
    uint32_t tc = 0;
    for (uint32_t v = 0; v < N; ++v) tc += counts[E + v];
    w *= pt_powi(to[E] / from[E], tc);
    if (has_long && std::fabs(from[E + 1]) > DBL_EPSILON) {
        uint32_t lc = 0;
        for (uint32_t v = 0; v < N; ++v) lc += counts[E + N + v];
        w *= pt_powi(to[E + 1] / from[E + 1], lc);
    }
    return w;
}

// the Hamiltonian of bond-table row `row` as relative_weight needs it: J of every edge (weight 2|J|, "prefers aligned" = J < 0),
// Gamma (weight of the transverse bonds), h (weight 2|h|, "prefers up" = h > 0; 0 without longitudinal bonds)
static void pt_ham_row(const isingmc_batch *b, uint32_t row, double *out) {
    const uint32_t E = b->dev.E, N = b->dev.N, Nb = b->dev.Nb;
    const BondRec *t0 = b->bonds_host.data() + (size_t)row * Nb;
    for (uint32_t e = 0; e < E; ++e) out[e] = (((t0[e].a_info >> (SSE_INFO_SHIFT + 2)) & 1u) ? -0.5 : 0.5) * t0[e].w;
    out[E] = t0[E].w;
    out[E + 1] = b->dev.has_long ? (((t0[E + N].a_info >> (SSE_INFO_SHIFT + 2)) & 1u) ? 0.5 : -0.5) * t0[E + N].w : 0.0;
}

static int pt_exchange_small(isingmc_batch *b, int peer, const uint32_t *s, uint32_t *r, size_t count) {
    PtState *P = b->pt;
    if (peer < 0 || peer >= (int)P->world) return ISINGMC_OK;
    if (P->comm) { // RCCL point-to-point on device buffers, one group call
        uint32_t *ds = P->d_small, *dr = P->d_small + count;
        HIP_TRY(b, hipMemcpyAsync(ds, s, 4 * count, hipMemcpyHostToDevice, b->stream));
        if (P->p_gstart() || P->p_send(ds, count, (int)ncclUint32, peer, P->comm, b->stream) || P->p_recv(dr, count, (int)ncclUint32, peer, P->comm, b->stream) || P->p_gend()) {
            b->err = "RCCL send/recv failed"; return ISINGMC_ENODEVICE;
        }
        HIP_TRY(b, hipMemcpyAsync(r, dr, 4 * count, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        return ISINGMC_OK;
    }
    if (!P->have_tr || P->tr.sendrecv(P->tr.ctx, peer, s, 4 * count, r, 4 * count)) { b->err = "tempering transport failed"; return ISINGMC_EINVAL; }
    return ISINGMC_OK;
}

extern "C" {

int isingmc_pt_decide(uint64_t seed, uint64_t step, uint32_t nchains, uint32_t ntemps, const double *betas,
                      const uint32_t *n_of_config, uint32_t *config_at, uint64_t *nswaps) {
    if (!betas || !n_of_config || !config_at || nchains == 0 || ntemps == 0) return ISINGMC_EINVAL;
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint64_t swaps = 0;
    for (uint32_t chain = 0; chain < nchains && ntemps > 1; ++chain) {
        uint32_t ctr[4] = {0u, (uint32_t)step, chain, (SSE_TAG_PT << 24) | (uint32_t)((step >> 32) & 0xFFFFFFu)};
        uint32_t o[4];
        host_philox(ctr, key, o);
        const bool a_first = (o[0] >> 31) != 0u; // gen_bool(0.5) (tempering_container.rs:140)
        for (int phase = 0; phase < 2; ++phase) {
            const bool set_a = (phase == 0) ? a_first : !a_first;
            for (uint32_t t = set_a ? 0u : 1u; t + 1 < ntemps; t += 2) { // make_first/second_subgraphs (:83-99)
                ctr[0] = 1u + t;
                host_philox(ctr, key, o);
                const double u = (double)o[0] * (1.0 / 4294967296.0);
                uint32_t &ca = config_at[(size_t)t * nchains + chain], &cb = config_at[(size_t)(t + 1) * nchains + chain];
                if (pt_accept(betas[t], betas[t + 1], n_of_config[ca], n_of_config[cb], 1.0, u)) { // (equal Hamiltonians)
                    const uint32_t tmp = ca; ca = cb; cb = tmp;
                    swaps++;
                }
            }
        }
    }
    if (nswaps) *nswaps += swaps;
    return ISINGMC_OK;
}

// device-side decisions: push the host's labels to the device / pull them back
static int pt_upload_labels(isingmc_batch *b) {
    PtState *P = b->pt;
    const uint32_t R = b->dev.R, K = P->nchains;
    std::vector<uint32_t> at(R);
    std::vector<double> br(R);
    for (uint32_t r = 0; r < R; ++r) { at[P->slot_of[r] - P->rank * R] = r; br[r] = P->betas[P->slot_of[r] / K]; }
    const unsigned long long tot = P->total_swaps;
    const uint32_t zero[2] = {0u, 0u};
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    HIP_TRY(b, hipMemcpy(P->d_slot_of, P->slot_of.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(P->d_at, at.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(P->d_beta_r, br.data(), 8 * (size_t)R, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(P->d_total, &tot, 8, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(P->d_result, zero, 8, hipMemcpyHostToDevice));
    P->host_stale = false;
    return ISINGMC_OK;
}
static int pt_sync_host(isingmc_batch *b) {
    PtState *P = b->pt;
    if (!P->dev_decide || !P->host_stale) return ISINGMC_OK;
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    unsigned long long tot = 0;
    uint32_t res[2] = {0u, 0u};
    HIP_TRY(b, hipMemcpy(P->slot_of.data(), P->d_slot_of, 4 * (size_t)b->dev.R, hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(&tot, P->d_total, 8, hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(res, P->d_result, 8, hipMemcpyDeviceToHost));
    P->total_swaps = tot;
    P->host_stale = false;
    if (res[1]) { b->err = "cutoff exceeds capacity"; return ISINGMC_ECAPACITY; }
    return ISINGMC_OK;
}

int isingmc_pt_create(isingmc_batch *b, const isingmc_pt_layout *lay) {
    if (!b || !lay || lay->struct_size != sizeof(isingmc_pt_layout) || !lay->betas || lay->ntemps == 0 || lay->nchains == 0 || lay->world == 0 ||
        lay->rank >= lay->world || lay->ntemps % lay->world) { if (b) b->err = "bad tempering layout (temperatures must divide evenly over the ranks)"; return ISINGMC_EINVAL; }
    const uint32_t tper = lay->ntemps / lay->world;
    if ((size_t)tper * lay->nchains != b->dev.R) { b->err = "the batch must hold ntemps/world * nchains replicas"; return ISINGMC_EINVAL; }
    if (lay->world > 1 && !lay->transport) { b->err = "a transport (or isingmc_pt_attach_nccl) is needed for more than one rank"; return ISINGMC_EINVAL; }
    HIP_TRY(b, hipSetDevice(b->device));
    pt_free(b);
    b->acc_follow_slots = false; // until the caller passes this layout's slots to isingmc_set_accumulator_rows
    PtState *P = new PtState();
    b->pt = P;
    P->ntemps = lay->ntemps; P->nchains = lay->nchains; P->rank = lay->rank; P->world = lay->world; P->tper = tper;
    P->betas.assign(lay->betas, lay->betas + lay->ntemps);
    P->seed = lay->seed;
    if (lay->transport) { P->tr = *lay->transport; P->have_tr = true; }
    const uint32_t R = b->dev.R;
    P->slot_of.resize(R); P->rid.resize(R);
    for (uint32_t r = 0; r < R; ++r) { P->slot_of[r] = P->rank * R + r; P->rid[r] = b->dev.replica_offset + r; }
    HIP_TRY(b, hipMalloc((void **)&P->d_rid, 4 * (size_t)R));
    HIP_TRY(b, hipMemcpy(P->d_rid, P->rid.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    b->dev.rid = P->d_rid;
    HIP_TRY(b, hipMalloc((void **)&P->d_small, 4 * 4 * (size_t)(P->nchains * 2 + 2)));
    HIP_TRY(b, hipMalloc((void **)&P->d_items, 4 * 3 * (size_t)P->nchains));
    P->pack_cap_words = (size_t)P->nchains * (PT_HDR + b->dev.nwords + 2 * SSE_MAX_CHUNKS + b->dev.cap);
    HIP_TRY(b, hipMalloc((void **)&P->d_pack_s, 4 * P->pack_cap_words));
    HIP_TRY(b, hipMalloc((void **)&P->d_pack_r, 4 * P->pack_cap_words));
    if (b->per_replica_J) {
        // different Hamiltonians between temperatures: the bond-table row belongs to the slot; neighbours' boundary rows once
        P->hams_differ = true;
        b->ham_row_host.resize(R);
        for (uint32_t r = 0; r < R; ++r) b->ham_row_host[r] = r;
        HIP_TRY(b, hipMalloc((void **)&P->d_ham_row, 4 * (size_t)R));
        HIP_TRY(b, hipMemcpy(P->d_ham_row, b->ham_row_host.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
        b->dev.ham_row = P->d_ham_row;
        HIP_TRY(b, hipMalloc((void **)&P->d_counts, 4 * (size_t)R * b->dev.Nb));
        const uint32_t E = b->dev.E, K = P->nchains, HS = E + 2; // a Hamiltonian row: [E] couplings, Gamma, h
        auto Jrow = [&](uint32_t row, std::vector<double> &out, size_t at) { pt_ham_row(b, row, out.data() + at); };
        std::vector<double> first((size_t)K * HS), last((size_t)K * HS);
        for (uint32_t k = 0; k < K; ++k) { Jrow(k, first, (size_t)k * HS); Jrow((tper - 1) * K + k, last, (size_t)k * HS); }
        P->J_prev_last.assign((size_t)K * HS, 0.0); P->J_next_first.assign((size_t)K * HS, 0.0);
        if (P->world > 1) {
            const int prev = (int)P->rank - 1, next = (int)P->rank + 1;
            if (prev >= 0 && P->tr.sendrecv(P->tr.ctx, prev, first.data(), 8 * first.size(), P->J_prev_last.data(), 8 * first.size())) { b->err = "tempering transport failed"; return ISINGMC_EINVAL; }
            if (next < (int)P->world && P->tr.sendrecv(P->tr.ctx, next, last.data(), 8 * last.size(), P->J_next_first.data(), 8 * last.size())) { b->err = "tempering transport failed"; return ISINGMC_EINVAL; }
        }
    }
    if (P->world == 1 && !P->hams_differ) { // every pair is interior and weighs one Hamiltonian: the decisions run on the device
        HIP_TRY(b, hipMalloc((void **)&P->d_slot_of, 4 * (size_t)R));
        HIP_TRY(b, hipMalloc((void **)&P->d_at, 4 * (size_t)R));
        HIP_TRY(b, hipMalloc((void **)&P->d_result, 8));
        HIP_TRY(b, hipMalloc((void **)&P->d_betas, 8 * (size_t)P->ntemps));
        HIP_TRY(b, hipMalloc((void **)&P->d_beta_r, 8 * (size_t)R));
        HIP_TRY(b, hipMalloc((void **)&P->d_total, 8));
        HIP_TRY(b, hipMemcpy(P->d_betas, P->betas.data(), 8 * (size_t)P->ntemps, hipMemcpyHostToDevice));
        const int rcu = pt_upload_labels(b);
        if (rcu) return rcu;
        P->dev_decide = true;
    }
    return ISINGMC_OK;
}
int isingmc_pt_set_device_decisions(isingmc_batch *b, int on) {
    if (!b || !b->pt) { if (b) b->err = "isingmc_pt_create first"; return ISINGMC_EINVAL; }
    PtState *P = b->pt;
    HIP_TRY(b, hipSetDevice(b->device));
    if (on && !P->d_slot_of) { b->err = "device-side tempering decisions need a single rank and one Hamiltonian for all temperatures"; return ISINGMC_ENOTIMPL; }
    if (!on && P->dev_decide) { const int rc = pt_sync_host(b); if (rc) return rc; P->dev_decide = false; }
    else if (on && !P->dev_decide) { const int rc = pt_upload_labels(b); if (rc) return rc; P->dev_decide = true; }
    return ISINGMC_OK;
}
int isingmc_pt_get_device_decisions(const isingmc_batch *b, int *on) {
    if (!b || !b->pt || !on) return ISINGMC_EINVAL;
    *on = b->pt->dev_decide ? 1 : 0;
    return ISINGMC_OK;
}
// Sweeps at the temperatures of the current labels.  With device-side decisions the betas never visit the host.
int isingmc_pt_timesteps(isingmc_batch *b, uint64_t t, uint32_t sampling_freq, uint32_t flags) {
    if (!b || !b->pt) { if (b) b->err = "isingmc_pt_create first"; return ISINGMC_EINVAL; }
    PtState *P = b->pt;
    if (P->dev_decide) {
        b->beta_dev = P->d_beta_r;
        const int rc = isingmc_timesteps(b, t, nullptr, sampling_freq, flags);
        b->beta_dev = nullptr;
        return rc;
    }
    std::vector<double> br(b->dev.R);
    for (uint32_t r = 0; r < b->dev.R; ++r) br[r] = P->betas[P->slot_of[r] / P->nchains];
    return isingmc_timesteps(b, t, br.data(), sampling_freq, flags);
}

int isingmc_pt_nccl_unique_id(isingmc_nccl_id *out) {
    if (!out) return ISINGMC_EINVAL;
    void *lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) return ISINGMC_ENODEVICE;
    auto f = reinterpret_cast<int (*)(isingmc_nccl_id *)>(dlsym(lib, "ncclGetUniqueId"));
    return (f && f(out) == 0) ? ISINGMC_OK : ISINGMC_ENODEVICE;
}

int isingmc_pt_attach_nccl(isingmc_batch *b, const isingmc_nccl_id *id) {
    if (!b || !b->pt || !id) { if (b) b->err = "isingmc_pt_create first"; return ISINGMC_EINVAL; }
    PtState *P = b->pt;
    HIP_TRY(b, hipSetDevice(b->device));
    void *lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD); // the copy the process already uses (e.g. torch's), if any
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) { b->err = "librccl.so not found"; return ISINGMC_ENODEVICE; }
    P->nccl_lib = lib;
    P->p_send = reinterpret_cast<decltype(P->p_send)>(dlsym(lib, "ncclSend"));
    P->p_recv = reinterpret_cast<decltype(P->p_recv)>(dlsym(lib, "ncclRecv"));
    P->p_gstart = reinterpret_cast<decltype(P->p_gstart)>(dlsym(lib, "ncclGroupStart"));
    P->p_gend = reinterpret_cast<decltype(P->p_gend)>(dlsym(lib, "ncclGroupEnd"));
    P->p_allreduce = reinterpret_cast<decltype(P->p_allreduce)>(dlsym(lib, "ncclAllReduce"));
    P->p_init = reinterpret_cast<decltype(P->p_init)>(dlsym(lib, "ncclCommInitRank"));
    P->p_destroy = reinterpret_cast<decltype(P->p_destroy)>(dlsym(lib, "ncclCommDestroy"));
    if (!P->p_send || !P->p_recv || !P->p_gstart || !P->p_gend || !P->p_allreduce || !P->p_init) { b->err = "RCCL symbols missing"; return ISINGMC_ENODEVICE; }
    if (P->p_init(&P->comm, (int)P->world, *id, (int)P->rank) != 0) { P->comm = nullptr; b->err = "ncclCommInitRank failed"; return ISINGMC_ENODEVICE; }
    return ISINGMC_OK;
}

int isingmc_pt_get_slots(isingmc_batch *b, uint32_t *slot_of_replica, double *beta_of_replica, uint32_t *config_id_of_replica) {
    if (!b || !b->pt) { if (b) b->err = "isingmc_pt_create first"; return ISINGMC_EINVAL; }
    { const int rcs = pt_sync_host(b); if (rcs) return rcs; }
    const PtState *P = b->pt;
    for (uint32_t r = 0; r < b->dev.R; ++r) {
        if (slot_of_replica) slot_of_replica[r] = P->slot_of[r];
        if (beta_of_replica) beta_of_replica[r] = P->betas[P->slot_of[r] / P->nchains];
        if (config_id_of_replica) config_id_of_replica[r] = P->rid[r];
    }
    return ISINGMC_OK;
}

// Container-level save / load (the reference serialises the whole TemperingContainer, tempering_container.rs:683-792): the labels,
// the configurations' identities and the step counter; the replicas themselves go through the batch's own checkpoint.
int isingmc_pt_get_state(isingmc_batch *b, uint64_t *step, uint64_t *total_swaps) {
    if (!b || !b->pt) { if (b) b->err = "isingmc_pt_create first"; return ISINGMC_EINVAL; }
    { const int rcs = pt_sync_host(b); if (rcs) return rcs; }
    if (step) *step = b->pt->step;
    if (total_swaps) *total_swaps = b->pt->total_swaps;
    return ISINGMC_OK;
}
int isingmc_pt_set_state(isingmc_batch *b, const uint32_t *slot_of_replica, const uint32_t *config_id_of_replica, uint64_t step, uint64_t total_swaps) {
    if (!b || !b->pt || !slot_of_replica || !config_id_of_replica) { if (b) b->err = "isingmc_pt_create first"; return ISINGMC_EINVAL; }
    PtState *P = b->pt;
    const uint32_t R = b->dev.R, lo = P->rank * R;
    std::vector<uint8_t> seen(R, 0);
    for (uint32_t r = 0; r < R; ++r) {
        if (slot_of_replica[r] < lo || slot_of_replica[r] >= lo + R || seen[slot_of_replica[r] - lo]) { b->err = "slots must be a permutation of this rank's temperature block"; return ISINGMC_EINVAL; }
        seen[slot_of_replica[r] - lo] = 1;
    }
    HIP_TRY(b, hipSetDevice(b->device));
    for (uint32_t r = 0; r < R; ++r) { P->slot_of[r] = slot_of_replica[r]; P->rid[r] = config_id_of_replica[r]; }
    HIP_TRY(b, hipMemcpy(P->d_rid, P->rid.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    if (P->hams_differ) {
        for (uint32_t r = 0; r < R; ++r) b->ham_row_host[r] = P->slot_of[r] - lo;
        HIP_TRY(b, hipMemcpy(P->d_ham_row, b->ham_row_host.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    }
    P->step = step; P->total_swaps = total_swaps;
    if (b->acc_follow_slots) HIP_TRY(b, hipMemcpy(b->d_acc_row, P->slot_of.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    if (P->dev_decide) return pt_upload_labels(b);
    return ISINGMC_OK;
}

// One tempering step of every chain (tempering_container.rs:121-149).  Adds the number of swaps this rank took part in
// as the LOWER temperature's owner (so that the sum over ranks counts every swap once) to *nswaps.
int isingmc_pt_step(isingmc_batch *b, uint64_t *nswaps) {
    if (!b || !b->pt) { if (b) b->err = "isingmc_pt_create first"; return ISINGMC_EINVAL; }
    PtState *P = b->pt;
    HIP_TRY(b, hipSetDevice(b->device));
    const uint32_t R = b->dev.R, K = P->nchains, T = P->ntemps, tper = P->tper, E = b->dev.E, Nb = b->dev.Nb;
    if (P->dev_decide) { // label swaps only: the op-strings (and any flip bytes still pending on them) are not touched
        if (T <= 1) { P->step++; return ISINGMC_OK; }
        PtDev D{};
        D.slot_of = P->d_slot_of; D.at = P->d_at; D.result = P->d_result; D.betas = P->d_betas; D.beta_r = P->d_beta_r; D.total = P->d_total;
        D.acc_row = b->acc_follow_slots ? b->d_acc_row : nullptr; // per-slot accumulators (isingmc_set_accumulator_rows with the slots) follow the labels
        D.K = K; D.T = T; D.key0 = (uint32_t)P->seed; D.key1 = (uint32_t)(P->seed >> 32); D.step = P->step;
        hipLaunchKernelGGL(pt_decide_kernel, dim3(1), dim3(K < 256 ? ((K + 63) / 64) * 64 : 256), 0, b->stream, b->dev, D);
        HIP_TRY(b, hipGetLastError());
        P->step++;
        P->host_stale = true;
        if (nswaps) { // the caller wants this step's count: one small read-back
            uint32_t res[2] = {0u, 0u};
            HIP_TRY(b, hipStreamSynchronize(b->stream));
            HIP_TRY(b, hipMemcpy(res, P->d_result, 8, hipMemcpyDeviceToHost));
            if (res[1]) { b->err = "cutoff exceeds capacity"; return ISINGMC_ECAPACITY; }
            *nswaps += res[0];
        }
        return ISINGMC_OK;
    }
    { const int rcm = ensure_materialized(b); if (rcm) return rcm; }
    const uint32_t t_lo = P->rank * tper, t_hi = t_lo + tper; // my temperature block [t_lo, t_hi)
    const int prev = P->rank > 0 ? (int)P->rank - 1 : -1, next = P->rank + 1 < P->world ? (int)P->rank + 1 : -1;
    uint64_t swaps = 0;
    if (T <= 1) { P->step++; return ISINGMC_OK; }
    std::vector<uint32_t> n(R), cut(R);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    HIP_TRY(b, hipMemcpy(n.data(), b->dev.n, 4 * (size_t)R, hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(cut.data(), b->dev.cutoff, 4 * (size_t)R, hipMemcpyDeviceToHost));
    // replica at a local slot
    std::vector<uint32_t> at(R);
    auto rebuild_at = [&]() { for (uint32_t r = 0; r < R; ++r) at[P->slot_of[r] - t_lo * K] = r; };
    rebuild_at();
    // ---- equalise the cutoffs of every chain over all temperatures (:129-137): max over the ranks ----
    std::vector<uint32_t> maxcut(K, 0u);
    for (uint32_t r = 0; r < R; ++r) { const uint32_t k = P->slot_of[r] % K; if (cut[r] > maxcut[k]) maxcut[k] = cut[r]; }
    if (P->world > 1) {
        if (P->comm) {
            HIP_TRY(b, hipMemcpyAsync(P->d_small, maxcut.data(), 4 * (size_t)K, hipMemcpyHostToDevice, b->stream));
            if (P->p_allreduce(P->d_small, P->d_small, K, (int)ncclUint32, (int)ncclMax, P->comm, b->stream)) { b->err = "ncclAllReduce failed"; return ISINGMC_ENODEVICE; }
            HIP_TRY(b, hipMemcpyAsync(maxcut.data(), P->d_small, 4 * (size_t)K, hipMemcpyDeviceToHost, b->stream));
            HIP_TRY(b, hipStreamSynchronize(b->stream));
        } else if (P->tr.allreduce_max_u32(P->tr.ctx, maxcut.data(), K)) { b->err = "tempering transport failed"; return ISINGMC_EINVAL; }
    }
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t k = P->slot_of[r] % K;
        if (maxcut[k] > b->dev.cap) { b->err = "cutoff exceeds capacity"; return ISINGMC_ECAPACITY; }
        cut[r] = maxcut[k];
    }
    HIP_TRY(b, hipMemcpy(b->dev.cutoff, cut.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    std::vector<uint32_t> counts; // bond counts of every local configuration (only when the Hamiltonians differ between temperatures)
    const uint32_t HS = E + 2;
    std::vector<double> Ja(HS), Jb(HS);
    // relative weight of local replica r (at local slot ls) towards the Hamiltonian of the slot above (+1) or below (-1)
    auto relw = [&](uint32_t r, uint32_t ls, int dir) -> double {
        if (!P->hams_differ) return 1.0;
        const uint32_t k = ls % K, tl = ls / K;
        pt_ham_row(b, ls, Ja.data());
        if (dir > 0) { if (tl + 1 < tper) pt_ham_row(b, ls + K, Jb.data()); else for (uint32_t e = 0; e < HS; ++e) Jb[e] = P->J_next_first[(size_t)k * HS + e]; }
        else { if (tl > 0) pt_ham_row(b, ls - K, Jb.data()); else for (uint32_t e = 0; e < HS; ++e) Jb[e] = P->J_prev_last[(size_t)k * HS + e]; }
        return pt_relative_weight(Ja.data(), Jb.data(), counts.data() + (size_t)r * Nb, E, b->dev.N, b->dev.has_long != 0u);
    };
    // order coin per chain (gen_bool(0.5), :140)
    const uint32_t key[2] = {(uint32_t)P->seed, (uint32_t)(P->seed >> 32)};
    std::vector<uint8_t> a_first(K);
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t ctr[4] = {0u, (uint32_t)P->step, k, (SSE_TAG_PT << 24) | (uint32_t)((P->step >> 32) & 0xFFFFFFu)};
        uint32_t o[4];
        host_philox(ctr, key, o);
        a_first[k] = (o[0] >> 31) != 0u;
    }
    auto decide = [&](uint32_t k, uint32_t t, uint32_t na, uint32_t nb2, double ra, double rb) -> bool {
        const uint32_t ctr[4] = {1u + t, (uint32_t)P->step, k, (SSE_TAG_PT << 24) | (uint32_t)((P->step >> 32) & 0xFFFFFFu)};
        uint32_t o[4];
        host_philox(ctr, key, o);
        const double u = (double)o[0] * (1.0 / 4294967296.0);
        return pt_accept(P->betas[t], P->betas[t + 1], na, nb2, P->hams_differ ? ra * rb : 1.0, u);
    };
    struct Wire { uint32_t n; uint32_t pad; double rel; };
    for (int phase = 0; phase < 2; ++phase) {
        if (P->hams_differ) { // (again in the second phase: a boundary swap of the first one replaced configurations)
            hipLaunchKernelGGL(pt_bond_count_kernel, dim3(R), dim3(256), 0, b->stream, b->dev, P->d_counts);
            counts.resize((size_t)R * Nb);
            HIP_TRY(b, hipMemcpyAsync(counts.data(), P->d_counts, 4 * counts.size(), hipMemcpyDeviceToHost, b->stream));
            HIP_TRY(b, hipStreamSynchronize(b->stream));
        }
        // boundary walkers of this phase: for chain k the pair (t, t+1) is in the phase's set iff (t even) == (set a)
        auto in_set = [&](uint32_t k, uint32_t t) { const bool set_a = (phase == 0) ? a_first[k] : !a_first[k]; return ((t & 1u) == 0u) == set_a; };
        // ---- exchange the operator counts (and relative weights) of the boundary walkers with both neighbours ----
        std::vector<Wire> s_prev(K), r_prev(K), s_next(K), r_next(K);
        for (uint32_t k = 0; k < K; ++k) {
            const uint32_t rf = at[k], rl = at[(tper - 1) * K + k];
            s_prev[k] = {n[rf], 0u, prev >= 0 ? relw(rf, k, -1) : 1.0};
            s_next[k] = {n[rl], 0u, next >= 0 ? relw(rl, (tper - 1) * K + k, +1) : 1.0};
        }
        static_assert(sizeof(Wire) == 16, "wire format");
        int rc;
        // (even ranks talk to their upper neighbour first: the host-staged transport is blocking)
        for (int turn = 0; turn < 2; ++turn) {
            const bool up = ((P->rank & 1u) == 0u) == (turn == 0);
            if (up) { if ((rc = pt_exchange_small(b, next, reinterpret_cast<const uint32_t *>(s_next.data()), reinterpret_cast<uint32_t *>(r_next.data()), 4 * (size_t)K))) return rc; }
            else if ((rc = pt_exchange_small(b, prev, reinterpret_cast<const uint32_t *>(s_prev.data()), reinterpret_cast<uint32_t *>(r_prev.data()), 4 * (size_t)K))) return rc;
        }
        // ---- decisions ----
        std::vector<uint32_t> items_next, items_prev; // accepted boundary swaps: (replica, word offset in the message, cutoff)
        size_t off_next = 0, off_prev = 0;
        for (uint32_t k = 0; k < K; ++k) {
            // interior pairs
            for (uint32_t t = t_lo; t + 1 < t_hi; ++t) {
                if (!in_set(k, t)) continue;
                const uint32_t la = (t - t_lo) * K + k, lb = la + K;
                const uint32_t ra_ = at[la], rb_ = at[lb];
                if (decide(k, t, n[ra_], n[rb_], relw(ra_, la, +1), relw(rb_, lb, -1))) {
                    std::swap(P->slot_of[ra_], P->slot_of[rb_]);
                    at[la] = rb_; at[lb] = ra_;
                    swaps++;
                }
            }
            const size_t words = PT_HDR + b->dev.nwords + 2 * SSE_MAX_CHUNKS + maxcut[k];
            // boundary pair with the next rank: (t_hi - 1, t_hi)
            if (next >= 0 && in_set(k, t_hi - 1)) {
                const uint32_t la = (tper - 1) * K + k, ra_ = at[la];
                if (decide(k, t_hi - 1, n[ra_], r_next[k].n, s_next[k].rel, r_next[k].rel)) {
                    items_next.insert(items_next.end(), {ra_, (uint32_t)off_next, maxcut[k]});
                    off_next += words;
                    n[ra_] = r_next[k].n;
                    swaps++; // counted by the owner of the lower temperature
                }
            }
            // boundary pair with the previous rank: (t_lo - 1, t_lo)
            if (prev >= 0 && in_set(k, t_lo - 1)) {
                const uint32_t rb_ = at[k];
                if (decide(k, t_lo - 1, r_prev[k].n, n[rb_], r_prev[k].rel, s_prev[k].rel)) {
                    items_prev.insert(items_prev.end(), {rb_, (uint32_t)off_prev, maxcut[k]});
                    off_prev += words;
                    n[rb_] = r_prev[k].n;
                }
            }
        }
        // ---- accepted boundary swaps: the two configurations change ranks ----
        for (int turn = 0; turn < 2; ++turn) {
            const bool up = ((P->rank & 1u) == 0u) == (turn == 0);
            const std::vector<uint32_t> &items = up ? items_next : items_prev;
            const size_t words = up ? off_next : off_prev;
            const int peer = up ? next : prev;
            if (peer < 0 || items.empty()) continue;
            const uint32_t nitems = (uint32_t)(items.size() / 3);
            uint32_t *d_it = P->d_items; // (at most one item per chain and turn)
            HIP_TRY(b, hipMemcpyAsync(d_it, items.data(), 4 * items.size(), hipMemcpyHostToDevice, b->stream));
            hipLaunchKernelGGL(pt_pack_kernel, dim3(nitems), dim3(256), 0, b->stream, b->dev, P->d_rid, d_it, P->d_pack_s);
            if (P->comm) {
                if (P->p_gstart() || P->p_send(P->d_pack_s, words, (int)ncclUint32, peer, P->comm, b->stream) || P->p_recv(P->d_pack_r, words, (int)ncclUint32, peer, P->comm, b->stream) || P->p_gend()) {
                    b->err = "RCCL send/recv failed"; return ISINGMC_ENODEVICE;
                }
            } else {
                P->h_pack_s.resize(words); P->h_pack_r.resize(words);
                HIP_TRY(b, hipMemcpyAsync(P->h_pack_s.data(), P->d_pack_s, 4 * words, hipMemcpyDeviceToHost, b->stream));
                HIP_TRY(b, hipStreamSynchronize(b->stream));
                if (P->tr.sendrecv(P->tr.ctx, peer, P->h_pack_s.data(), 4 * words, P->h_pack_r.data(), 4 * words)) { b->err = "tempering transport failed"; return ISINGMC_EINVAL; }
                HIP_TRY(b, hipMemcpyAsync(P->d_pack_r, P->h_pack_r.data(), 4 * words, hipMemcpyHostToDevice, b->stream));
            }
            hipLaunchKernelGGL(pt_unpack_kernel, dim3(nitems), dim3(256), 0, b->stream, b->dev, P->d_rid, d_it, P->d_pack_r);
            HIP_TRY(b, hipStreamSynchronize(b->stream));
        }
        if (!items_next.empty() || !items_prev.empty()) HIP_TRY(b, hipMemcpy(P->rid.data(), P->d_rid, 4 * (size_t)R, hipMemcpyDeviceToHost));
    }
    if (P->hams_differ) { // the bond-table row follows the slot
        for (uint32_t r = 0; r < R; ++r) b->ham_row_host[r] = P->slot_of[r] - t_lo * K;
        HIP_TRY(b, hipMemcpy(P->d_ham_row, b->ham_row_host.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    }
    if (b->acc_follow_slots) HIP_TRY(b, hipMemcpy(b->d_acc_row, P->slot_of.data(), 4 * (size_t)R, hipMemcpyHostToDevice)); // as the decision kernel does
    P->step++;
    P->total_swaps += swaps;
    if (nswaps) *nswaps += swaps;
    return ISINGMC_OK;
}

} // extern "C"

// isingmc_set_accumulator_rows asks: did the caller pass the tempering slots (an [ntemps * nchains] table, row of replica r = its slot)?
// Only then do the rows follow the labels in isingmc_pt_step, on the device path and on the host path alike.
int sse::pt_rows_are_slots(isingmc_batch *b, uint32_t nrows, const uint32_t *rows, bool *yes) {
    *yes = false;
    PtState *P = b->pt;
    if (!P || nrows != P->ntemps * P->nchains) return ISINGMC_OK;
    if (const int rc = pt_sync_host(b)) return rc;
    for (uint32_t r = 0; r < b->dev.R; ++r) if (rows[r] != P->slot_of[r]) return ISINGMC_OK;
    *yes = true;
    return ISINGMC_OK;
}
