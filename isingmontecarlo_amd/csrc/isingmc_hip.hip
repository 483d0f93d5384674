// isingmc_hip.hip — the accessors of the C ABI (include/isingmc_hip.h) and their three kernels; the imaginary-time folds of group observables
// and the bond counts are checked and staged here and launch itime.hip's kernel.  Creation lives in create.hip, the sweep driver in
// driver.hip, parallel tempering in pt.hip, the sample record in record.hip.  There is no CPU compute fallback.
#include "batch.hip.h"
#include "sse_core.hip.h" // op_weight, the op-word fields
#include "sse_launch.h"   // launch_itime and its LDS plan

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

using namespace sse;

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

// The launch behind isingmc_itime_groups (ngroups checked groups -> sum_all / sum_occ [R][ngroups]) and isingmc_bond_counts (ngroups = 0,
// counts [R][Nb]): what LDS cannot serve is refused before anything is launched; then the pending flip bytes are brought in, the groups and
// the variable -> groups lists built from them go up, itime_kernel runs on the batch's stream and the results come down.
static int itime_run(isingmc_batch *b, uint32_t ngroups, const uint32_t *group_start, const uint32_t *group_vars, const uint8_t *group_flip,
                     int64_t *sum_all, int64_t *sum_occ, uint32_t *counts) {
    const uint32_t R = b->dev.R, N = b->dev.N, Nb = b->dev.Nb, nv = ngroups ? group_start[ngroups] : 0u;
    const ItimePlan plan = itime_plan(b->lds_total_words, N, b->dev.nwords, Nb, ngroups, nv, counts != nullptr);
    if (!plan.W) {
        char buf[200];
        snprintf(buf, sizeof buf, "itime_groups: %u groups on %u variables exceed LDS (their sums and bit arrays live there): at most %u groups on this model",
                 ngroups, N, itime_max_groups(b->lds_total_words, N, b->dev.nwords));
        b->err = buf;
        return ISINGMC_ENOTIMPL;
    }
    HIP_TRY(b, hipSetDevice(b->device));
    { const int rcm = ensure_materialized(b); if (rcm) return rcm; }
    // device scratch: sums [2][R][G] (8-byte aligned, first) | counts [R][Nb] | words: start [G + 1], vars [nv], vstart [N + 1], vgroups [nv], flip bytes [G], flip bits
    const size_t o_occ = (size_t)R * ngroups * 8, o_counts = 2 * o_occ, o_meta = o_counts + (counts ? (size_t)R * Nb * 4 : 0);
    const size_t w_vars = (size_t)ngroups + 1, w_vstart = w_vars + nv, w_vgroups = w_vstart + N + 1, w_flip = w_vgroups + nv, w_fbits = w_flip + (ngroups + 3) / 4,
                 meta_words = ngroups ? w_fbits + 2 * (((size_t)ngroups + 63) / 64) : 0;
    const size_t bytes = o_meta + 4 * meta_words;
    if (b->itime_buf.reserve(bytes, b->stream) != hipSuccess) { (void)hipGetLastError(); b->err = "itime fold: allocation of the device scratch failed"; return ISINGMC_ENODEVICE; }
    char *buf = b->itime_buf.as<char>();
    ItimeArgs A{};
    A.W = plan.W; A.hist_lds = plan.hist_lds; A.csr_lds = plan.csr_lds; A.nv = nv;
    std::vector<uint32_t> meta(meta_words); // (lives until the stream has been drained below)
    if (ngroups) {
        std::copy(group_start, group_start + ngroups + 1, meta.begin());
        std::copy(group_vars, group_vars + nv, meta.begin() + w_vars);
        // variable -> groups: a counting sort of the (group, variable) pairs by variable, groups ascending within a variable
        uint32_t *vstart = meta.data() + w_vstart, *vgroups = meta.data() + w_vgroups;
        for (uint32_t k = 0; k < nv; ++k) vstart[group_vars[k] + 1]++;
        for (uint32_t v = 0; v < N; ++v) vstart[v + 1] += vstart[v];
        std::vector<uint32_t> fill(vstart, vstart + N);
        for (uint32_t g = 0; g < ngroups; ++g)
            for (uint32_t k = group_start[g]; k < group_start[g + 1]; ++k) vgroups[fill[group_vars[k]]++] = g;
        if (group_flip)
            for (uint32_t g = 0; g < ngroups; ++g) {
                ((uint8_t *)(meta.data() + w_flip))[g] = group_flip[g] & 1u;
                meta[w_fbits + (g >> 5)] |= (uint32_t)(group_flip[g] & 1u) << (g & 31u);
            }
        HIP_TRY(b, hipMemcpyAsync(buf + o_meta, meta.data(), 4 * meta_words, hipMemcpyHostToDevice, b->stream));
        const uint32_t *dm = (const uint32_t *)(buf + o_meta);
        A.G = ObsGroups{ngroups, dm, dm + w_vars, group_flip ? (const uint8_t *)(dm + w_flip) : nullptr};
        A.vstart = dm + w_vstart; A.vgroups = dm + w_vgroups;
        A.flip_bits = group_flip ? dm + w_fbits : nullptr;
        A.sum_all = sum_all ? (int64_t *)buf : nullptr;
        A.sum_occ = sum_occ ? (int64_t *)(buf + o_occ) : nullptr;
    }
    if (counts) {
        A.counts = (uint32_t *)(buf + o_counts);
        if (!plan.hist_lds) HIP_TRY(b, hipMemsetAsync(A.counts, 0, (size_t)R * Nb * 4, b->stream));
    }
    const hipError_t e = launch_itime(b->stream, b->dev, A);
    if (e != hipSuccess) { b->err = std::string("itime fold launch: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    if (sum_all) HIP_TRY(b, hipMemcpyAsync(sum_all, buf, o_occ, hipMemcpyDeviceToHost, b->stream));
    if (sum_occ) HIP_TRY(b, hipMemcpyAsync(sum_occ, buf + o_occ, o_occ, hipMemcpyDeviceToHost, b->stream));
    if (counts) HIP_TRY(b, hipMemcpyAsync(counts, A.counts, (size_t)R * Nb * 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    return ISINGMC_OK;
}

extern "C" {

int isingmc_get_accumulators(isingmc_batch *b, uint64_t *out) { return b ? copy_down(b, out, b->dev.acc, 8 * (size_t)b->acc_rows) : ISINGMC_EINVAL; }
int isingmc_set_accumulators(isingmc_batch *b, const uint64_t *in) { return b ? copy_up(b, b->dev.acc, in, 8 * (size_t)b->acc_rows, true) : ISINGMC_EINVAL; }
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
    if (const int rc = pt_rows_are_slots(b, nrows, rows, &b->acc_follow_slots)) return rc;
    if (nrows != b->acc_rows) {
        if (const int rc = dalloc(b, &b->dev.acc, (size_t)nrows * 8, true, &b->acc)) return rc; // (the stream is idle: the previous table goes here)
        b->acc_rows = nrows;
    }
    HIP_TRY(b, hipMemcpy(b->d_acc_row, rows, sizeof(uint32_t) * b->dev.R, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}
int isingmc_set_cutoffs(isingmc_batch *b, const uint32_t *cutoffs) {
    if (!b || !cutoffs) return ISINGMC_EINVAL;
    std::vector<uint32_t> cur(b->dev.R);
    if (const int rc = copy_down(b, cur.data(), b->dev.cutoff, b->dev.R)) return rc;
    for (uint32_t r = 0; r < b->dev.R; ++r) {
        if (cutoffs[r] > b->dev.cap) { b->err = "cutoff exceeds capacity"; return ISINGMC_ECAPACITY; }
        if (cutoffs[r] > cur[r]) cur[r] = cutoffs[r]; // fast_ops.rs:1258-1262: only grows
    }
    return copy_up(b, b->dev.cutoff, cur.data(), b->dev.R);
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
    const uint32_t r0 = r == UINT32_MAX ? 0 : r, cnt = r == UINT32_MAX ? b->dev.R : 1;
    std::vector<uint32_t> w((size_t)cnt * b->dev.nwords);
    if (const int rc = copy_down(b, w.data(), b->dev.state + (size_t)r0 * b->dev.nwords, w.size())) return rc;
    unpack_bits(w.data(), cnt, b->dev.N, b->dev.nwords, out);
    return ISINGMC_OK;
}
int isingmc_set_state(isingmc_batch *b, uint32_t r, const uint8_t *in) {
    if (!b || !in || (r != UINT32_MAX && r >= b->dev.R)) { if (b) b->err = "bad replica index"; return ISINGMC_EINVAL; }
    const uint32_t r0 = r == UINT32_MAX ? 0 : r, cnt = r == UINT32_MAX ? b->dev.R : 1;
    std::vector<uint32_t> w((size_t)cnt * b->dev.nwords);
    pack_bits(in, cnt, b->dev.N, b->dev.nwords, w.data());
    return copy_up(b, b->dev.state + (size_t)r0 * b->dev.nwords, w.data(), w.size());
}

int isingmc_get_n(isingmc_batch *b, uint32_t *out) { return b ? copy_down(b, out, b->dev.n, b->dev.R) : ISINGMC_EINVAL; }
int isingmc_get_cutoff(isingmc_batch *b, uint32_t *out) { return b ? copy_down(b, out, b->dev.cutoff, b->dev.R) : ISINGMC_EINVAL; }
int isingmc_get_epoch(isingmc_batch *b, uint64_t *out) { return b ? copy_down(b, out, b->dev.epoch, b->dev.R) : ISINGMC_EINVAL; }
int isingmc_set_epoch(isingmc_batch *b, const uint64_t *epochs) { return b ? copy_up(b, b->dev.epoch, epochs, b->dev.R) : ISINGMC_EINVAL; }
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
    DevBuf d1, d2, d3; // (per call: freed on every way out)
    HIP_TRY(b, d1.alloc(sizeof(long long) * R));
    if (d2.alloc(sizeof(unsigned long long) * R) != hipSuccess || d3.alloc(sizeof(unsigned long long) * R) != hipSuccess) {
        b->err = "itime_magnetization: allocation failed"; return ISINGMC_ENODEVICE;
    }
    hipLaunchKernelGGL(itime_magnetization_kernel, dim3(R), dim3(256), 0, b->stream, b->dev, d1.as<long long>(), d2.as<unsigned long long>(), d3.as<unsigned long long>());
    hipError_t e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(sum_m, d1.as<void>(), sizeof(long long) * R, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(sum_m2, d2.as<void>(), sizeof(unsigned long long) * R, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(sum_abs_m, d3.as<void>(), sizeof(unsigned long long) * R, hipMemcpyDeviceToHost);
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

int isingmc_itime_groups(isingmc_batch *b, uint32_t ngroups, const uint32_t *group_start, const uint32_t *group_vars, const uint8_t *group_flip,
                         int64_t *sum_all, int64_t *sum_occ) {
    if (!b) return ISINGMC_EINVAL;
    if (!ngroups || !group_start || !group_vars) { b->err = "itime_groups: no observable groups"; return ISINGMC_EINVAL; }
    if (!sum_all && !sum_occ) { b->err = "itime_groups: no output buffer"; return ISINGMC_EINVAL; }
    if (const int rc = check_groups(b, "itime_groups", ngroups, group_start, group_vars, b->dev.N)) return rc;
    return itime_run(b, ngroups, group_start, group_vars, group_flip, sum_all, sum_occ, nullptr);
}
int isingmc_bond_counts(isingmc_batch *b, uint32_t *out) {
    if (!b) return ISINGMC_EINVAL;
    if (!out) { b->err = "bond_counts: no output buffer"; return ISINGMC_EINVAL; }
    return itime_run(b, 0, nullptr, nullptr, nullptr, nullptr, nullptr, out);
}

int isingmc_debug_counts(isingmc_batch *b, uint32_t *out) {
    if (!b || !out) return ISINGMC_EINVAL;
    HIP_TRY(b, hipSetDevice(b->device));
    { const int rcm = ensure_materialized(b); if (rcm) return rcm; }
    DevBuf d; // (per call)
    HIP_TRY(b, d.alloc(12 * (size_t)b->dev.R));
    hipLaunchKernelGGL(debug_counts_kernel, dim3(b->dev.R), dim3(256), 0, b->stream, b->dev, d.as<uint32_t>());
    hipError_t e = hipMemcpyAsync(out, d.as<void>(), 12 * (size_t)b->dev.R, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
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
