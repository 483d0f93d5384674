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
//
// The swap rule itself is pt_rule.h.  This file applies it three times: isingmc_pt_decide (a whole ladder on the host),
// pt_decide_kernel (a rank that owns every temperature) and isingmc_pt_plan_phase (one rank's share of a phase, from plain data:
// the host leg of isingmc_pt_step calls it, and so do tests that simulate ranks without a device).
#include "batch.hip.h"
#include "pt_rule.h"      // the swap rule: decision stream, pt_accept, the walk of a phase
#include "sse_core.hip.h" // philox4x32_10

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <utility>
#include <dlfcn.h>
#include <rccl/rccl.h> // types and enum values only (ncclUint32, ncclMax, ncclUniqueId): the library itself is dlopen()ed on first use
static_assert(sizeof(ncclUniqueId) == sizeof(isingmc_nccl_id), "isingmc_nccl_id must carry an ncclUniqueId");

using namespace sse;

// A rank's two neighbours, [0] the lower and [1] the upper one: what one phase exchanges with each.  (The neighbour's boundary
// Hamiltonian rows are the halo of PtState::ham.)
struct PtSide {
    int peer = -1;                          // rank, -1 = none
    std::vector<isingmc_pt_wire> sent, got; // [nchains] boundary walkers' operator counts and relative weights
    std::vector<uint32_t> items;            // [3 * nchains] accepted boundary swaps: (replica, word offset in the message, cutoff)
    uint32_t nitems = 0;
    uint64_t words = 0;                     // words of the configuration message
};
static_assert(sizeof(isingmc_pt_wire) == 16 && offsetof(isingmc_pt_wire, rel) == 8, "wire format");

struct PtState {
    uint32_t ntemps = 0, nchains = 0, rank = 0, world = 1, tper = 0;
    std::vector<double> betas;
    uint64_t seed = 0, step = 0, total_swaps = 0;
    std::vector<uint32_t> slot_of; // [R] global slot t*nchains + chain labelling local replica r
    std::vector<uint32_t> rid;     // [R] configuration identity (global id it was created with)
    DevBuf d_rid, d_ham_row;       // [R] u32 each: the device copies of rid and of the batch's ham_row_host
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
    DevBuf d_slot_of, d_at, d_result; // u32: [R], [R]; d_result: [0] swaps of the last step, [1] error flag
    DevBuf d_betas, d_beta_r;         // double: [ntemps], [R]
    DevBuf d_total;                   // unsigned long long: total swaps since isingmc_pt_create / set_state
    DevBuf d_items; // u32 [3 * nchains] accepted boundary swaps of one turn: (replica, word offset, cutoff)
    DevBuf d_small; // u32 [4][nchains] staging of the boundary operator counts / cutoffs on the device (RCCL path)
    // different Hamiltonians per temperature (per-replica couplings)
    bool hams_differ = false;
    std::vector<double> ham;      // [nchains + R + nchains][E + 2] Hamiltonian row (pt_ham_row) of local slot ls at row nchains + ls; the halo
                                  // rows are the lower neighbour's last and the upper neighbour's first temperature
    DevBuf d_counts;              // u32 [R][Nb] bond counts (only when hams_differ)
    PtSide side[2];
    // configuration exchange
    DevBuf d_pack_s, d_pack_r;    // u32 [pack_cap_words] each
    size_t pack_cap_words = 0;
    std::vector<uint32_t> h_pack_s, h_pack_r;
};

void sse::pt_free(isingmc_batch *b) {
    if (!b->pt) return;
    PtState *P = b->pt;
    if (P->comm && P->p_destroy) (void)P->p_destroy(P->comm);
    delete P;
    b->pt = nullptr;
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
    uint32_t K, T;
    uint64_t seed, step;
};
// the draw of pt_rule.h's decision stream in a kernel: the same integers as pt_philox_word
struct PtKernelDraw {
    __device__ uint32_t operator()(const PtChain &c, uint32_t index) const { return philox4x32_10(index, c.step_lo, c.chain, c.tag_step_hi, c.key0, c.key1).x; }
};
// One tempering step of a rank that owns all temperatures (tempering_container.rs:121-149; pt_rule.h): thread k takes chain k — equalise
// its cutoffs, draw the order coin, walk the two phases.
__global__ void pt_decide_kernel(DevBatch B, PtDev P) {
    __shared__ unsigned int s_swaps;
    if (threadIdx.x == 0) s_swaps = 0u;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < P.K; k += blockDim.x) {
        uint32_t maxcut = 0;
        for (uint32_t t = 0; t < P.T; ++t) { const uint32_t c = B.cutoff[P.at[t * P.K + k]]; maxcut = c > maxcut ? c : maxcut; }
        if (maxcut > B.cap) { P.result[1] = 1u; continue; }
        for (uint32_t t = 0; t < P.T; ++t) B.cutoff[P.at[t * P.K + k]] = maxcut;
        const PtChain c = pt_chain(P.seed, P.step, k);
        const bool a_first = pt_a_first(c, PtKernelDraw{});
        uint32_t swaps = 0;
        for (int phase = 0; phase < 2; ++phase)
            pt_walk_phase(c, a_first, phase, 0u, P.T - 1u, PtKernelDraw{}, [&](uint32_t t, double u) {
                const uint32_t la = t * P.K + k, lb = la + P.K;
                const uint32_t ra = P.at[la], rb = P.at[lb];
                if (pt_accept(P.betas[t], P.betas[t + 1], B.n[ra], B.n[rb], 1.0, u)) { P.slot_of[ra] = lb; P.slot_of[rb] = la; P.at[la] = rb; P.at[lb] = ra; swaps++; }
            });
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

// ---- transport: RCCL on device buffers once a communicator is attached, otherwise the caller's host-staged functions ----
// `words` u32 to and from `peer` in one exchange: an RCCL group call on the device buffers, or the caller's blocking sendrecv on the
// host buffers.  The callers stage between host and device on the side that needs it.
static int pt_sendrecv(isingmc_batch *b, int peer, const uint32_t *dev_s, uint32_t *dev_r, const void *host_s, void *host_r, size_t words) {
    PtState *P = b->pt;
    if (P->comm) {
        if (P->p_gstart() || P->p_send(dev_s, words, (int)ncclUint32, peer, P->comm, b->stream) || P->p_recv(dev_r, words, (int)ncclUint32, peer, P->comm, b->stream) || P->p_gend()) {
            b->err = "RCCL send/recv failed"; return ISINGMC_ENODEVICE;
        }
        return ISINGMC_OK;
    }
    if (!P->have_tr || P->tr.sendrecv(P->tr.ctx, peer, host_s, 4 * words, host_r, 4 * words)) { b->err = "tempering transport failed"; return ISINGMC_EINVAL; }
    return ISINGMC_OK;
}
// element-wise maximum of v over all ranks, in place
static int pt_allreduce_max(isingmc_batch *b, std::vector<uint32_t> &v) {
    PtState *P = b->pt;
    if (P->comm) {
        HIP_TRY(b, hipMemcpyAsync(P->d_small.as<uint32_t>(), v.data(), 4 * v.size(), hipMemcpyHostToDevice, b->stream));
        if (P->p_allreduce(P->d_small.as<uint32_t>(), P->d_small.as<uint32_t>(), v.size(), (int)ncclUint32, (int)ncclMax, P->comm, b->stream)) { b->err = "ncclAllReduce failed"; return ISINGMC_ENODEVICE; }
        HIP_TRY(b, hipMemcpyAsync(v.data(), P->d_small.as<uint32_t>(), 4 * v.size(), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(b, hipStreamSynchronize(b->stream));
    } else if (P->tr.allreduce_max_u32(P->tr.ctx, v.data(), v.size())) { b->err = "tempering transport failed"; return ISINGMC_EINVAL; }
    return ISINGMC_OK;
}
// the side a rank talks to in turn 0 and 1 of an exchange: even ranks talk to their upper neighbour first (the host-staged transport is blocking)
static PtSide &pt_turn_side(PtState *P, int turn) { return P->side[(((P->rank & 1u) == 0u) == (turn == 0)) ? 1 : 0]; }

extern "C" {

int isingmc_pt_decide(uint64_t seed, uint64_t step, uint32_t nchains, uint32_t ntemps, const double *betas,
                      const uint32_t *n_of_config, uint32_t *config_at, uint64_t *nswaps) {
    if (!betas || !n_of_config || !config_at || nchains == 0 || ntemps == 0) return ISINGMC_EINVAL;
    uint64_t swaps = 0;
    for (uint32_t chain = 0; chain < nchains && ntemps > 1; ++chain) {
        const PtChain c = pt_chain(seed, step, chain);
        const bool a_first = pt_a_first(c, PtHostDraw{});
        for (int phase = 0; phase < 2; ++phase)
            pt_walk_phase(c, a_first, phase, 0u, ntemps - 1u, PtHostDraw{}, [&](uint32_t t, double u) {
                uint32_t &ca = config_at[(size_t)t * nchains + chain], &cb = config_at[(size_t)(t + 1) * nchains + chain];
                if (pt_accept(betas[t], betas[t + 1], n_of_config[ca], n_of_config[cb], 1.0, u)) { std::swap(ca, cb); swaps++; } // (equal Hamiltonians)
            });
    }
    if (nswaps) *nswaps += swaps;
    return ISINGMC_OK;
}

// One rank's decisions of one phase from plain data (include/isingmc_hip.h): no device, no batch.  Chain k walks the pairs (t, t + 1)
// that touch this rank's block [t_lo, t_hi): the pair below the block when there is a lower neighbour, the interior pairs, the pair
// above it when there is an upper one.  A walker that is not local comes from the neighbour's wire.
int isingmc_pt_plan_phase(isingmc_pt_phase *v) {
    if (!v || v->struct_size != sizeof(isingmc_pt_phase) || v->world == 0 || v->rank >= v->world || v->tper == 0 || v->nchains == 0 || v->phase > 1 ||
        !v->betas || !v->n || !v->cutoff || !v->slot_of || !v->at) return ISINGMC_EINVAL;
    const bool has[2] = {v->rank > 0, v->rank + 1 < v->world};
    for (int s = 0; s < 2; ++s) if (has[s] && (!v->from[s] || !v->items[s])) return ISINGMC_EINVAL;
    const uint32_t K = v->nchains, t_lo = v->rank * v->tper, t_hi = t_lo + v->tper;
    size_t off[2] = {0, 0};
    v->nitems[0] = v->nitems[1] = 0;
    v->nswaps = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const PtChain c = pt_chain(v->seed, v->step, k);
        pt_walk_phase(c, pt_a_first(c, PtHostDraw{}), (int)v->phase, t_lo - (has[0] ? 1u : 0u), t_hi - (has[1] ? 0u : 1u), PtHostDraw{}, [&](uint32_t t, double u) {
            const bool a_here = t >= t_lo, b_here = t + 1 < t_hi; // the walkers at t and at t + 1: local, or the neighbour's
            const uint32_t la = (t - t_lo) * K + k, lb = la + K, ra = a_here ? v->at[la] : 0u, rb = b_here ? v->at[lb] : 0u;
            const uint32_t n_a = a_here ? v->n[ra] : v->from[0][k].n, n_b = b_here ? v->n[rb] : v->from[1][k].n;
            const double rel_a = !a_here ? v->from[0][k].rel : v->rel ? v->rel[ra] : 1.0, rel_b = !b_here ? v->from[1][k].rel : v->rel ? v->rel[rb] : 1.0;
            if (!pt_accept(v->betas[t], v->betas[t + 1], n_a, n_b, rel_a * rel_b, u)) return;
            if (a_here && b_here) { // labels change hands
                std::swap(v->slot_of[ra], v->slot_of[rb]);
                v->at[la] = rb; v->at[lb] = ra;
            } else { // the two configurations change ranks
                const int s = a_here ? 1 : 0;
                uint32_t *it = v->items[s] + 3 * v->nitems[s]++;
                it[0] = a_here ? ra : rb; it[1] = (uint32_t)off[s]; it[2] = v->cutoff[k];
                off[s] += (size_t)v->fixed_words + v->cutoff[k];
            }
            if (a_here) v->nswaps++; // counted by the owner of the lower temperature
        });
    }
    v->words[0] = off[0]; v->words[1] = off[1];
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
    HIP_TRY(b, hipMemcpy(P->d_slot_of.as<uint32_t>(), P->slot_of.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(P->d_at.as<uint32_t>(), at.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(P->d_beta_r.as<double>(), br.data(), 8 * (size_t)R, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(P->d_total.as<unsigned long long>(), &tot, 8, hipMemcpyHostToDevice));
    HIP_TRY(b, hipMemcpy(P->d_result.as<uint32_t>(), zero, 8, hipMemcpyHostToDevice));
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
    HIP_TRY(b, hipMemcpy(P->slot_of.data(), P->d_slot_of.as<uint32_t>(), 4 * (size_t)b->dev.R, hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(&tot, P->d_total.as<unsigned long long>(), 8, hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(res, P->d_result.as<uint32_t>(), 8, hipMemcpyDeviceToHost));
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
    HIP_TRY(b, P->d_rid.alloc(4 * (size_t)R));
    HIP_TRY(b, hipMemcpy(P->d_rid.as<uint32_t>(), P->rid.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    b->dev.rid = P->d_rid.as<uint32_t>();
    HIP_TRY(b, P->d_small.alloc(4 * 4 * (size_t)(P->nchains * 2 + 2)));
    HIP_TRY(b, P->d_items.alloc(4 * 3 * (size_t)P->nchains));
    P->side[0].peer = P->rank > 0 ? (int)P->rank - 1 : -1;
    P->side[1].peer = P->rank + 1 < P->world ? (int)P->rank + 1 : -1;
    for (PtSide &S : P->side) { S.sent.resize(P->nchains); S.got.resize(P->nchains); S.items.resize(3 * (size_t)P->nchains); }
    P->pack_cap_words = (size_t)P->nchains * (PT_HDR + b->dev.nwords + 2 * SSE_MAX_CHUNKS + b->dev.cap);
    HIP_TRY(b, P->d_pack_s.alloc(4 * P->pack_cap_words));
    HIP_TRY(b, P->d_pack_r.alloc(4 * P->pack_cap_words));
    if (b->per_replica_J) {
        // different Hamiltonians between temperatures: the bond-table row belongs to the slot; neighbours' boundary rows once
        P->hams_differ = true;
        b->ham_row_host.resize(R);
        for (uint32_t r = 0; r < R; ++r) b->ham_row_host[r] = r;
        HIP_TRY(b, P->d_ham_row.alloc(4 * (size_t)R));
        HIP_TRY(b, hipMemcpy(P->d_ham_row.as<uint32_t>(), b->ham_row_host.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
        b->dev.ham_row = P->d_ham_row.as<uint32_t>();
        HIP_TRY(b, P->d_counts.alloc(4 * (size_t)R * b->dev.Nb));
        const uint32_t K = P->nchains, HS = b->dev.E + 2; // a Hamiltonian row: [E] couplings, Gamma, h
        const size_t edge = (size_t)K * HS;               // one temperature's rows: what a neighbour needs
        P->ham.assign((size_t)(R + 2 * K) * HS, 0.0);
        for (uint32_t ls = 0; ls < R; ++ls) pt_ham_row(b, ls, P->ham.data() + (size_t)(K + ls) * HS);
        // my first temperature goes to the lower neighbour, my last to the upper one; theirs fill the halo
        const size_t mine[2] = {edge, (size_t)R * HS}, halo[2] = {0, (size_t)(R + K) * HS};
        for (int s = 0; s < 2; ++s)
            if (P->side[s].peer >= 0 && P->tr.sendrecv(P->tr.ctx, P->side[s].peer, P->ham.data() + mine[s], 8 * edge, P->ham.data() + halo[s], 8 * edge)) { b->err = "tempering transport failed"; return ISINGMC_EINVAL; }
    }
    if (P->world == 1 && !P->hams_differ) { // every pair is interior and weighs one Hamiltonian: the decisions run on the device
        HIP_TRY(b, P->d_slot_of.alloc(4 * (size_t)R));
        HIP_TRY(b, P->d_at.alloc(4 * (size_t)R));
        HIP_TRY(b, P->d_result.alloc(8));
        HIP_TRY(b, P->d_betas.alloc(8 * (size_t)P->ntemps));
        HIP_TRY(b, P->d_beta_r.alloc(8 * (size_t)R));
        HIP_TRY(b, P->d_total.alloc(8));
        HIP_TRY(b, hipMemcpy(P->d_betas.as<double>(), P->betas.data(), 8 * (size_t)P->ntemps, hipMemcpyHostToDevice));
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
        b->beta_dev = P->d_beta_r.as<double>();
        const int rc = isingmc_timesteps(b, t, nullptr, sampling_freq, flags);
        b->beta_dev = nullptr;
        return rc;
    }
    std::vector<double> br(b->dev.R);
    for (uint32_t r = 0; r < b->dev.R; ++r) br[r] = P->betas[P->slot_of[r] / P->nchains];
    return isingmc_timesteps(b, t, br.data(), sampling_freq, flags);
}

// RCCL: the copy the process already uses (e.g. torch's), if any, then the loader's, then ROCm's
static void *pt_open_rccl() {
    void *lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    return lib;
}

int isingmc_pt_nccl_unique_id(isingmc_nccl_id *out) {
    if (!out) return ISINGMC_EINVAL;
    void *lib = pt_open_rccl();
    if (!lib) return ISINGMC_ENODEVICE;
    auto f = reinterpret_cast<int (*)(isingmc_nccl_id *)>(dlsym(lib, "ncclGetUniqueId"));
    return (f && f(out) == 0) ? ISINGMC_OK : ISINGMC_ENODEVICE;
}

int isingmc_pt_attach_nccl(isingmc_batch *b, const isingmc_nccl_id *id) {
    if (!b || !b->pt || !id) { if (b) b->err = "isingmc_pt_create first"; return ISINGMC_EINVAL; }
    PtState *P = b->pt;
    HIP_TRY(b, hipSetDevice(b->device));
    void *lib = pt_open_rccl();
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
    HIP_TRY(b, hipMemcpy(P->d_rid.as<uint32_t>(), P->rid.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    if (P->hams_differ) {
        for (uint32_t r = 0; r < R; ++r) b->ham_row_host[r] = P->slot_of[r] - lo;
        HIP_TRY(b, hipMemcpy(P->d_ham_row.as<uint32_t>(), b->ham_row_host.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    }
    P->step = step; P->total_swaps = total_swaps;
    if (b->acc_follow_slots) HIP_TRY(b, hipMemcpy(b->d_acc_row, P->slot_of.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    if (P->dev_decide) return pt_upload_labels(b);
    return ISINGMC_OK;
}

// ---- isingmc_pt_step in parts: the device leg, or the host leg's read, equalise, two phases (counts, decisions, moves), finish ----

// The device leg: label swaps only, the op-strings (and any flip bytes still pending on them) are not touched.  Nothing is read back
// unless the caller wants this step's count.
static int pt_step_on_device(isingmc_batch *b, uint64_t *nswaps) {
    PtState *P = b->pt;
    const uint32_t K = P->nchains;
    if (P->ntemps <= 1) { P->step++; return ISINGMC_OK; }
    PtDev D{};
    D.slot_of = P->d_slot_of.as<uint32_t>(); D.at = P->d_at.as<uint32_t>(); D.result = P->d_result.as<uint32_t>(); D.betas = P->d_betas.as<double>(); D.beta_r = P->d_beta_r.as<double>(); D.total = P->d_total.as<unsigned long long>();
    D.acc_row = b->acc_follow_slots ? b->d_acc_row : nullptr; // per-slot accumulators (isingmc_set_accumulator_rows with the slots) follow the labels
    D.K = K; D.T = P->ntemps; D.seed = P->seed; D.step = P->step;
    hipLaunchKernelGGL(pt_decide_kernel, dim3(1), dim3(K < 256 ? ((K + 63) / 64) * 64 : 256), 0, b->stream, b->dev, D);
    HIP_TRY(b, hipGetLastError());
    P->step++;
    P->host_stale = true;
    if (nswaps) { // one small read-back
        uint32_t res[2] = {0u, 0u};
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        HIP_TRY(b, hipMemcpy(res, P->d_result.as<uint32_t>(), 8, hipMemcpyDeviceToHost));
        if (res[1]) { b->err = "cutoff exceeds capacity"; return ISINGMC_ECAPACITY; }
        *nswaps += res[0];
    }
    return ISINGMC_OK;
}

// what the host leg carries from part to part
struct PtHostStep {
    std::vector<uint32_t> n, cut; // [R] operator count and cutoff of local replica r
    std::vector<uint32_t> at;     // [R] replica at local slot ls (the inverse of slot_of)
    std::vector<uint32_t> maxcut; // [nchains] the chain's cutoff after equalising
    std::vector<uint32_t> counts; // [R][Nb] bond counts            } only when the Hamiltonians differ between temperatures
    std::vector<double> rel;      // [R] see pt_relative_weights    }
    uint64_t swaps = 0;
};

static int pt_read_counts(isingmc_batch *b, PtHostStep &S) {
    const PtState *P = b->pt;
    const uint32_t R = b->dev.R;
    S.n.resize(R); S.cut.resize(R); S.at.resize(R);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    HIP_TRY(b, hipMemcpy(S.n.data(), b->dev.n, 4 * (size_t)R, hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(S.cut.data(), b->dev.cutoff, 4 * (size_t)R, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < R; ++r) S.at[P->slot_of[r] - P->rank * R] = r;
    return ISINGMC_OK;
}

// every chain gets one cutoff over all its temperatures (:129-137): the maximum, over the ranks too
static int pt_equalise_cutoffs(isingmc_batch *b, PtHostStep &S) {
    PtState *P = b->pt;
    const uint32_t R = b->dev.R, K = P->nchains;
    S.maxcut.assign(K, 0u);
    for (uint32_t r = 0; r < R; ++r) { const uint32_t k = P->slot_of[r] % K; if (S.cut[r] > S.maxcut[k]) S.maxcut[k] = S.cut[r]; }
    if (P->world > 1) if (const int rc = pt_allreduce_max(b, S.maxcut)) return rc;
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t k = P->slot_of[r] % K;
        if (S.maxcut[k] > b->dev.cap) { b->err = "cutoff exceeds capacity"; return ISINGMC_ECAPACITY; }
        S.cut[r] = S.maxcut[k];
    }
    HIP_TRY(b, hipMemcpy(b->dev.cutoff, S.cut.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}

// bond counts of every local configuration (again in the second phase: a boundary swap of the first one replaced configurations)
static int pt_bond_counts(isingmc_batch *b, PtHostStep &S) {
    const uint32_t R = b->dev.R;
    hipLaunchKernelGGL(pt_bond_count_kernel, dim3(R), dim3(256), 0, b->stream, b->dev, b->pt->d_counts.as<uint32_t>());
    S.counts.resize((size_t)R * b->dev.Nb);
    HIP_TRY(b, hipMemcpyAsync(S.counts.data(), b->pt->d_counts.as<uint32_t>(), 4 * S.counts.size(), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    return ISINGMC_OK;
}

// rel[r]: the weight of local replica r under the Hamiltonian of the partner of its pair in this phase, relative to its own slot's
// (1 at an end of the ladder).  Pairs of a phase are disjoint: one weight per replica.
static void pt_relative_weights(const isingmc_batch *b, int phase, PtHostStep &S) {
    const PtState *P = b->pt;
    const uint32_t R = b->dev.R, K = P->nchains, HS = b->dev.E + 2;
    S.rel.resize(R);
    for (uint32_t ls = 0; ls < R; ++ls) {
        const uint32_t r = S.at[ls], t = P->rank * P->tper + ls / K;
        const bool up = pt_in_phase(pt_a_first(pt_chain(P->seed, P->step, ls % K), PtHostDraw{}), phase, t); // the partner sits above
        const double *own = P->ham.data() + (size_t)(K + ls) * HS, *partner = up ? own + (size_t)K * HS : own - (size_t)K * HS;
        S.rel[r] = (up ? t + 1 < P->ntemps : t > 0) ? pt_relative_weight(own, partner, S.counts.data() + (size_t)r * b->dev.Nb, b->dev.E, b->dev.N, b->dev.has_long != 0u) : 1.0;
    }
}

// the boundary walkers' operator counts (and relative weights) go to both neighbours, theirs come back
static int pt_exchange_counts(isingmc_batch *b, const PtHostStep &S) {
    PtState *P = b->pt;
    const uint32_t K = P->nchains;
    for (int s = 0; s < 2; ++s)
        for (uint32_t k = 0; k < K && P->side[s].peer >= 0; ++k) {
            const uint32_t r = S.at[(s ? (P->tper - 1) * K : 0u) + k];
            P->side[s].sent[k] = {S.n[r], 0u, P->hams_differ ? S.rel[r] : 1.0};
        }
    const size_t words = 4 * (size_t)K;
    uint32_t *ds = P->d_small.as<uint32_t>(), *dr = P->d_small.as<uint32_t>() + words;
    for (int turn = 0; turn < 2; ++turn) {
        PtSide &N = pt_turn_side(P, turn);
        if (N.peer < 0) continue;
        if (P->comm) HIP_TRY(b, hipMemcpyAsync(ds, N.sent.data(), 4 * words, hipMemcpyHostToDevice, b->stream));
        if (const int rc = pt_sendrecv(b, N.peer, ds, dr, N.sent.data(), N.got.data(), words)) return rc;
        if (P->comm) {
            HIP_TRY(b, hipMemcpyAsync(N.got.data(), dr, 4 * words, hipMemcpyDeviceToHost, b->stream));
            HIP_TRY(b, hipStreamSynchronize(b->stream));
        }
    }
    return ISINGMC_OK;
}

// isingmc_pt_plan_phase on this rank's view; a walker that is about to arrive brings its operator count
static int pt_decide_phase(isingmc_batch *b, int phase, PtHostStep &S) {
    PtState *P = b->pt;
    isingmc_pt_phase v{};
    v.struct_size = sizeof(v);
    v.rank = P->rank; v.world = P->world; v.tper = P->tper; v.nchains = P->nchains; v.phase = (uint32_t)phase;
    v.betas = P->betas.data(); v.seed = P->seed; v.step = P->step;
    v.n = S.n.data(); v.rel = P->hams_differ ? S.rel.data() : nullptr;
    v.cutoff = S.maxcut.data(); v.fixed_words = PT_HDR + b->dev.nwords + 2 * SSE_MAX_CHUNKS;
    v.slot_of = P->slot_of.data(); v.at = S.at.data();
    for (int s = 0; s < 2; ++s) { v.from[s] = P->side[s].got.data(); v.items[s] = P->side[s].items.data(); }
    if (isingmc_pt_plan_phase(&v)) { b->err = "bad tempering phase"; return ISINGMC_EINVAL; }
    S.swaps += v.nswaps;
    for (int s = 0; s < 2; ++s) {
        PtSide &N = P->side[s];
        N.nitems = v.nitems[s]; N.words = v.words[s];
        for (uint32_t i = 0; i < N.nitems; ++i) { const uint32_t r = N.items[3 * i]; S.n[r] = N.got[P->slot_of[r] % P->nchains].n; }
    }
    return ISINGMC_OK;
}

// accepted boundary swaps: the two configurations change ranks
static int pt_move_configurations(isingmc_batch *b) {
    PtState *P = b->pt;
    for (int turn = 0; turn < 2; ++turn) {
        const PtSide &N = pt_turn_side(P, turn);
        if (N.peer < 0 || N.nitems == 0) continue;
        const size_t words = N.words;
        uint32_t *d_it = P->d_items.as<uint32_t>(); // (at most one item per chain and turn)
        HIP_TRY(b, hipMemcpyAsync(d_it, N.items.data(), 4 * 3 * (size_t)N.nitems, hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(pt_pack_kernel, dim3(N.nitems), dim3(256), 0, b->stream, b->dev, P->d_rid.as<uint32_t>(), d_it, P->d_pack_s.as<uint32_t>());
        if (!P->comm) {
            P->h_pack_s.resize(words); P->h_pack_r.resize(words);
            HIP_TRY(b, hipMemcpyAsync(P->h_pack_s.data(), P->d_pack_s.as<uint32_t>(), 4 * words, hipMemcpyDeviceToHost, b->stream));
            HIP_TRY(b, hipStreamSynchronize(b->stream));
        }
        if (const int rc = pt_sendrecv(b, N.peer, P->d_pack_s.as<uint32_t>(), P->d_pack_r.as<uint32_t>(), P->h_pack_s.data(), P->h_pack_r.data(), words)) return rc;
        if (!P->comm) HIP_TRY(b, hipMemcpyAsync(P->d_pack_r.as<uint32_t>(), P->h_pack_r.data(), 4 * words, hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(pt_unpack_kernel, dim3(N.nitems), dim3(256), 0, b->stream, b->dev, P->d_rid.as<uint32_t>(), d_it, P->d_pack_r.as<uint32_t>());
        HIP_TRY(b, hipStreamSynchronize(b->stream));
    }
    if (P->side[0].nitems || P->side[1].nitems) HIP_TRY(b, hipMemcpy(P->rid.data(), P->d_rid.as<uint32_t>(), 4 * (size_t)b->dev.R, hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}

// the bond-table rows and the accumulator rows follow the slots (as the decision kernel does), then the counters
static int pt_finish(isingmc_batch *b, uint64_t swaps, uint64_t *nswaps) {
    PtState *P = b->pt;
    const uint32_t R = b->dev.R;
    if (P->hams_differ) {
        for (uint32_t r = 0; r < R; ++r) b->ham_row_host[r] = P->slot_of[r] - P->rank * R;
        HIP_TRY(b, hipMemcpy(P->d_ham_row.as<uint32_t>(), b->ham_row_host.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    }
    if (b->acc_follow_slots) HIP_TRY(b, hipMemcpy(b->d_acc_row, P->slot_of.data(), 4 * (size_t)R, hipMemcpyHostToDevice));
    P->step++;
    P->total_swaps += swaps;
    if (nswaps) *nswaps += swaps;
    return ISINGMC_OK;
}

// One tempering step of every chain (tempering_container.rs:121-149).  Adds the number of swaps this rank took part in
// as the LOWER temperature's owner (so that the sum over ranks counts every swap once) to *nswaps.
int isingmc_pt_step(isingmc_batch *b, uint64_t *nswaps) {
    if (!b || !b->pt) { if (b) b->err = "isingmc_pt_create first"; return ISINGMC_EINVAL; }
    PtState *P = b->pt;
    HIP_TRY(b, hipSetDevice(b->device));
    if (P->dev_decide) return pt_step_on_device(b, nswaps);
    int rc = ensure_materialized(b);
    if (rc) return rc;
    if (P->ntemps <= 1) { P->step++; return ISINGMC_OK; }
    PtHostStep S;
    if ((rc = pt_read_counts(b, S)) || (rc = pt_equalise_cutoffs(b, S))) return rc;
    for (int phase = 0; phase < 2; ++phase) {
        if (P->hams_differ) {
            if ((rc = pt_bond_counts(b, S))) return rc;
            pt_relative_weights(b, phase, S);
        }
        if ((rc = pt_exchange_counts(b, S)) || (rc = pt_decide_phase(b, phase, S)) || (rc = pt_move_configurations(b))) return rc;
    }
    return pt_finish(b, S.swaps, nswaps);
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
