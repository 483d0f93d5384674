// sse_cluster_pass.hip.h — the general cluster update: segment scan, apply pass, the pass itself; the touched-variable scan and the
// free-spin pass behind it (sse::sweep_kernel, sse_sweep.hip.h; sse_cluster.hip.h shares free_spin_pass).
#pragma once
#include "sse_unionfind.hip.h"

namespace sse {

// Segment scan shared by cluster build and apply.  BARRIER-FREE: wave w owns a contiguous range of chunks of
// the op-string and scans it alone, in p order, with its own copy of the "latest cut per variable" table.
// Segment ids (min-root union-find => canonical label = smallest id of a cluster):
//   [0,N)                 P(0,v): the part of worldline v that contains p=0
//   [N, N+C)              N+k   : the segment opened by the k-th cut in p order (C = number of transverse ops);
//                                 dense ids come from the per-chunk transverse counts kept by the diagonal pass
//   [N+C, N+C+(W-1)N)     P(w,v): "whatever segment v is in when wave w's range begins" — artificial ids, larger
//                                 than every real id so they are never roots; joined to the real segments after
//                                 the scan (cluster_pass).
template <int W, int K, bool CL, bool APPLY, bool G, bool TG, bool PM = false>
__device__ __forceinline__ void cluster_scan(const DevBatch &B, const Lds<W> &L, uint32_t r, uint32_t M, const UFA<G> &uf,
                                             uint32_t C) {
    constexpr int NT = W * 64;
    const Tab<TG> T = make_tab<TG, W>(B, L, r);
    constexpr uint32_t TS = 64 * K; // slots per wave-tile
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6); // scalar: keeps per-wave control flow uniform
    const uint32_t N = B.N;
    uint32_t *ops = B.ops + (size_t)r * B.stride;
    uint32_t *segs_row = B.segs + (size_t)r * B.stride;
    const uint32_t h_mycur = (uint32_t)wave * N; // element offset of this wave's tables inside o_cur / o_cl
    if constexpr (TG) { for (uint32_t i = tid; i < (uint32_t)W * N; i += NT) T.rec_st(i, 0u); }
    else {
        for (uint32_t i = tid; i < ((uint32_t)W * N + 1) / 2; i += NT) T.st32(T.cur, i, 0u);
        for (uint32_t i = tid; i < ((uint32_t)W * N + 3) / 4; i += NT) T.st32(T.cl, i, 0u);
    }
    __syncthreads();
    // this wave's chunk range and the dense id of its first cut
    const uint32_t used = (M + B.CH - 1) / B.CH;
    const uint32_t q = (used + W - 1) / W;
    const uint32_t c0 = min((uint32_t)wave * q, used), c1 = min(c0 + q, used);
    uint32_t cutbase = 0;
    for (uint32_t c = lane; c < c0; c += 64) cutbase += LDSW(L.o_chtr, c);
    for (int off = 32; off > 0; off >>= 1) cutbase += __shfl_xor(cutbase, off);
    cutbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)cutbase);
    const uint32_t pbeg = c0 * B.CH, pend = min(c1 * B.CH, M);
    const uint32_t my_placeholder_base = wave == 0 ? 0u : N + C + (uint32_t)(wave - 1) * N;
    const uint32_t idbase = N + cutbase - 1u; // id of the cut with local rank+1 == x is idbase + x
    if (lane == 0) LDSW(L.o_chg, wave) = idbase; // read back by cluster_pass when it joins the ranges
    uint32_t nlocal = 0;                      // cuts seen so far in this wave's range
    // branch-free prefetch (see diagonal_pass): ranges are whole tiles except at the end of the string, where the
    // padded row holds zeros; past the range end the last tile is simply read again
    uint32_t wnext[K];
#pragma unroll
    for (int j = 0; j < K; ++j) wnext[j] = row_ld(ops, pbeg + j * 64 + lane);
    for (uint32_t p0 = pbeg; p0 < pend; p0 += TS) {
#ifdef SSE_GEN_ROTATE
        sse_set_prio(p0 / TS / SSE_GEN_ROTATE + blockIdx.x);
#endif
        uint32_t word[K], pos[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { word[j] = (p0 + j * 64 + lane < pend) ? wnext[j] : 0u; pos[j] = p0 + j * 64 + lane; }
        {
            const uint32_t pn0 = p0 + TS < pend ? p0 + TS : p0;
#pragma unroll
            for (int j = 0; j < K; ++j) wnext[j] = row_ld(ops, pn0 + j * 64 + lane);
        }
        uint32_t ua[K], uc[K]; // the tile's unions, issued together after the K sub-rounds (unions commute)
        bool utwo[K];
        uint4 pre_rec[K]; // general bond table: request the tile's K records together (see diagonal_pass)
        if constexpr (!CL) {
#pragma unroll
            for (int j = 0; j < K; ++j) pre_rec[j] = bond_rec<PM, W>(B, L, word[j] ? sse_op_bond(word[j]) : 0u);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            // straight-line, predicated code: every LDS read uses a safe index and is issued unconditionally
            const uint32_t wd = word[j];
            const bool nonempty = wd != 0u;
            Bd d;
            if constexpr (CL) d = decode_bond<CL, W>(B, L, nonempty ? sse_op_bond(wd) : 0u);
            else { const uint4 q = pre_rec[j]; d.a = q.x & SSE_VAR_MASK; d.c = q.y; d.kp = q.x >> SSE_INFO_SHIFT; d.w = 0.0; }
            const uint32_t va = d.a, kind = bd_kind(d);
            const bool two = nonempty & (d.c != SSE_NO_VAR);
            const uint32_t vc = two ? d.c : va;
            const bool iscut = nonempty & (kind == SSE_BOND_TRANSVERSE);
            const uint64_t cutmask = sse_ballot(nonempty) & sse_ballot(kind == SSE_BOND_TRANSVERSE); // = ballot(iscut), from the compare masks
            const uint32_t first = idbase + nlocal + 1u;
            const uint32_t kown = popc64(cutmask & lanemask_lt(lane)); // cuts of this sub-round at earlier lanes
            const uint32_t id_own = first + kown;
            // Ordered resolution inside the sub-round: a leg on variable x belongs to the segment of the latest
            // cut on x at an EARLIER slot.  The cut lanes publish 1 + (their rank inside the sub-round) in o_cl;
            // one round of LDS reads then gives every lane the latest cut before the sub-round (o_cur) and the
            // cut inside it (o_cl), which precedes the lane iff its rank is below the lane's own count of
            // earlier cuts.  Two cuts of one sub-round on the same variable are rare: a serial loop over the cut
            // lanes (ballot + v_readlane) resolves those.
            if (cutmask) {
                if (iscut) { if constexpr (TG) T.rec_mark_st(h_mycur + va, kown + 1u); else T.st8(T.cl, h_mycur + va, kown + 1u); }
                SSE_WAVE_FENCE();
            }
            uint32_t xa, xc, ma, mc;
            if constexpr (TG) {
                const uint32_t ra = T.rec_ld(h_mycur + va), rc = T.rec_ld(h_mycur + vc);
                xa = ra & 0xFFFFu; xc = rc & 0xFFFFu; ma = (ra >> 16) & 0xFFu; mc = (rc >> 16) & 0xFFu;
                if constexpr (!APPLY) { // touched flags: stored once per (wave, variable), not once per leg (every store dirties a sector)
                    if (nonempty & !(ra >> 24)) T.rec_touch_st(h_mycur + va);
                    if (nonempty & !(rc >> 24)) T.rec_touch_st(h_mycur + vc);
                }
            } else {
                xa = T.ld16(T.cur, h_mycur + va); xc = T.ld16(T.cur, h_mycur + vc);
                ma = T.ld8(T.cl, h_mycur + va); mc = T.ld8(T.cl, h_mycur + vc);
            }
            uint32_t seg_a = xa ? idbase + xa : my_placeholder_base + va;
            uint32_t seg_c = xc ? idbase + xc : my_placeholder_base + vc;
            if (cutmask) {
                const uint32_t myrank1 = id_own - idbase; // rank+1 of this lane's cut inside the wave's range
                const uint64_t dup = cutmask & sse_ballot(ma != kown + 1u);
                if (!dup) {
                    seg_a = ((ma - 1u) < kown) ? first + (ma - 1u) : seg_a; // ma == 0: no cut on the variable
                    seg_c = ((mc - 1u) < kown) ? first + (mc - 1u) : seg_c;
                    SSE_WAVE_FENCE();
                    if (iscut) { if constexpr (TG) T.rec_st(h_mycur + va, myrank1 | (1u << 24)); /* rank, marker 0, touched */ else { T.st16(T.cur, h_mycur + va, myrank1); T.st8(T.cl, h_mycur + va, 0u); } }
                } else {
                    bool lastcut = iscut; // no later cut lane of this sub-round is on the same variable
                    uint64_t m = cutmask;
                    uint32_t idL = first;
                    while (m) {
                        const int Ls = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const uint32_t vL = __builtin_amdgcn_readlane(va, Ls);
                        const bool later = lane > Ls, same_a = va == vL;
                        seg_a = (later & same_a) ? idL : seg_a;
                        seg_c = (later & (vc == vL)) ? idL : seg_c;
                        lastcut = lastcut & !((lane < Ls) & same_a);
                        idL++;
                    }
                    SSE_WAVE_FENCE();
                    if (iscut) { if constexpr (TG) T.rec_mark_st(h_mycur + va, 0u); else T.st8(T.cl, h_mycur + va, 0u); }
                    if (iscut & lastcut) { if constexpr (TG) T.rec_rank_st(h_mycur + va, myrank1); else T.st16(T.cur, h_mycur + va, myrank1); } // the last cut wins
                }
            }
            nlocal += popc64(cutmask);
            if (!APPLY) {
                if (iscut) uf.set(id_own, id_own);
                if constexpr (!TG) { if (nonempty & !SSE_DBG(B, 8u)) { T.st8(T.touch8, va, 1u); T.st8(T.touch8, vc, 1u); } } // (MODE 2: with the record lookups; diagnostic builds: bit 3 = time the scan without them)
                ua[j] = seg_a; uc[j] = seg_c;
                utwo[j] = two & !SSE_DBG(B, 1u); // diagnostic builds: bit 0 = time the scan without unions
                if (B.has_long) if (nonempty & (kind == SSE_BOND_LONGITUDINAL)) uf.frozen_or(seg_a >> 5, 1u << (seg_a & 31));
                if constexpr (!G) { // ids fit 16 bits on this path: remember them for the apply pass
                    const uint32_t hi = iscut ? id_own : (two ? seg_c : seg_a);
                    row_st(segs_row, pos[j], seg_a | (hi << 16));
                } else if (B.segs2) { // 32-bit ids: two words per slot, so that the apply pass need not repeat the ordered scan
                    const uint32_t hi = iscut ? id_own : (two ? seg_c : seg_a);
                    row_st(segs_row, pos[j], seg_a);
                    row_st(B.segs2 + (size_t)r * B.stride, pos[j], hi);
                }
            } else {
                const uint32_t fa = uf.get(seg_a), fc = uf.get(seg_c), fo = uf.get(iscut ? id_own : seg_a);
                const uint32_t f2 = two ? (fc << 1) : 0u;
                const uint32_t in = sse_op_in(wd) ^ (fa | f2), out = sse_op_out(wd) ^ (fo | f2);
                const uint32_t neww = (wd & ~0xFu) | in | (out << SSE_OP_OUT_SHIFT);
                if (nonempty & (neww != wd)) ops[p0 + j * 64 + lane] = neww;
            }
        }
        if constexpr (!APPLY) {
            {
                // During the scan every wave only touches ids of its own range (its cuts and its placeholders), so
                // its trees are private until the ranges are joined: no atomics are needed, lanes of the wave that
                // hook the same root in one store instruction are sorted out by reading the parent back.  The K
                // unions of the tile go together, three overlapped rounds of table accesses for all of them: parents,
                // grandparents (root test + halving), read-back of the links.  All reads of a batch precede all its
                // stores, so every lane decides on the same snapshot; a link that another lane overwrote (same
                // root hooked twice) or a chain deeper than two falls back to the serial routine.  The same code serves
                // the parents in LDS and the 32-bit parents in HBM (one wave's accesses are ordered, as for the tables).
                uint32_t pa[K], pc[K], ga[K], gc[K], hi[K], lo[K];
                bool link[K], slow[K];
#pragma unroll
                for (int j = 0; j < K; ++j) { pa[j] = uf.get(utwo[j] ? ua[j] : 0u); pc[j] = uf.get(utwo[j] ? uc[j] : 0u); }
#pragma unroll
                for (int j = 0; j < K; ++j) { ga[j] = uf.get(pa[j]); gc[j] = uf.get(pc[j]); }
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const bool differ = utwo[j] & (pa[j] != pc[j]); // same parent: one set already
                    const bool roots = (ga[j] == pa[j]) & (gc[j] == pc[j]);
                    link[j] = differ & roots;
                    slow[j] = differ & !roots;
                    lo[j] = pa[j] < pc[j] ? pa[j] : pc[j];
                    hi[j] = pa[j] < pc[j] ? pc[j] : pa[j];
                    // halving: an endpoint whose parent is not a root moves up (it is not a root itself then)
                    if (utwo[j] & (ga[j] != pa[j])) uf.set(ua[j], ga[j]);
                    if (utwo[j] & (gc[j] != pc[j])) uf.set(uc[j], gc[j]);
                    if (link[j]) uf.set(hi[j], lo[j]);
                }
                SSE_WAVE_FENCE();
                uint32_t chk[K];
#pragma unroll
                for (int j = 0; j < K; ++j) chk[j] = uf.get(link[j] ? hi[j] : 0u);
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const bool redo = slow[j] | (link[j] & (chk[j] != lo[j]));
                    if (sse_any(redo)) { if (redo) uf_union_wave(uf, pa[j], pc[j]); }
                }
            }
        }
    }
    __syncthreads();
}

// Apply pass of the LDS union-find path (cluster.rs:139-167): every slot's segment ids were stored by the build
// scan, flip bits sit in the (flattened) parent table, so the slots can be rewritten in any order: plain strided
// streaming, no ordered scan.  Input bits flip with the incoming segment, output bits with the outgoing one.
template <int W, int K, bool CL, bool G = false, bool PM = false, bool LF = false>
__device__ __forceinline__ void cluster_apply_cached(const DevBatch &B, const Lds<W> &L, uint32_t r, uint32_t M, const UFA<G> &uf) {
    static_assert(!LF || G, "flip bits in LDS belong to the HBM union-find path");
    auto flip_of = [&](uint32_t id) -> uint32_t { // the flip of id: a bit in LDS (LF) or the (flattened, coin-overwritten) parent entry
        if constexpr (LF) return (LDSW(L.o_parent, id >> 5) >> (id & 31u)) & 1u; else return uf.get(id);
    };
    constexpr int NT = W * 64;
    const int tid = threadIdx.x;
    uint32_t *ops = B.ops + (size_t)r * B.stride;
    const uint32_t *segs = B.segs + (size_t)r * B.stride;
    const uint32_t *segs2 = G ? B.segs2 + (size_t)r * B.stride : segs; // 32-bit ids: the second id of a slot has its own row
    // software-pipelined stream over whole tiles (branch-free loads and stores, see diagonal_pass): slots >= M are
    // empty and are written back unchanged
    constexpr uint32_t TS = (uint32_t)(K * NT);
    uint32_t wn[K], sn[K], tn[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { wn[j] = row_ld(ops, (uint32_t)(j * NT + tid)); sn[j] = row_ld(segs, (uint32_t)(j * NT + tid)); tn[j] = G ? row_ld(segs2, (uint32_t)(j * NT + tid)) : 0u; }
    for (uint32_t p0 = 0; p0 < M; p0 += TS) {
#ifdef SSE_GEN_ROTATE
        sse_set_prio(p0 / TS / SSE_GEN_ROTATE + blockIdx.x);
#endif
        uint32_t wd[K], sg[K], sh[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { wd[j] = wn[j]; sg[j] = sn[j]; sh[j] = tn[j]; }
        {
            const uint32_t pn0 = p0 + TS < M ? p0 + TS : p0;
#pragma unroll
            for (int j = 0; j < K; ++j) { wn[j] = row_ld(ops, pn0 + (uint32_t)(j * NT + tid)); sn[j] = row_ld(segs, pn0 + (uint32_t)(j * NT + tid)); if constexpr (G) tn[j] = row_ld(segs2, pn0 + (uint32_t)(j * NT + tid)); }
        }
        uint32_t second[K]; // general bond table: the second variable of the tile's K bonds, requested together
        if constexpr (!CL && !PM) {
#pragma unroll
            for (int j = 0; j < K; ++j) second[j] = reinterpret_cast<const uint32_t *>(B.bonds + (wd[j] ? sse_op_bond(wd[j]) : 0u))[1];
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint32_t w = wd[j];
            const bool nonempty = w != 0u;
            // segment ids of empty slots are stale: read a safe index
            const uint32_t fa = flip_of(nonempty ? (G ? sg[j] : (sg[j] & 0xFFFFu)) : 0u), fb = flip_of(nonempty ? (G ? sh[j] : (sg[j] >> 16)) : 0u);
            bool two;
            if constexpr (CL || PM) two = nonempty & (sse_op_bond(w) < B.E);
            else two = nonempty & (second[j] != SSE_NO_VAR);
            // two-site: both legs of variable a carry fa, both legs of variable c carry fb;
            // single-site: the input leg carries fa (incoming segment), the output leg fb (outgoing segment)
            const uint32_t in = sse_op_in(w) ^ (two ? (fa | (fb << 1)) : fa);
            const uint32_t out = sse_op_out(w) ^ (two ? (fa | (fb << 1)) : fb);
            const uint32_t neww = (w & ~0xFu) | in | (out << SSE_OP_OUT_SHIFT);
            row_st(ops, p0 + (uint32_t)(j * NT + tid), nonempty ? neww : 0u);
        }
    }
    __syncthreads();
}

// Cluster update.  Reference: ClusterUpdater::flip_each_cluster_rng (qmc_traits/cluster.rs:36-172) with the
// longitudinal weight function of qmc_ising.rs:759-775.  Returns the number of clusters.
template <int W, int K, bool CL, bool UF_GLOBAL, bool TG, bool PM = false>
__device__ __forceinline__ uint32_t cluster_pass(const DevBatch &B, const Lds<W> &L, uint32_t r, const Rng &rng, double prob,
                                                 uint32_t M, int n, int ntrans, uint32_t &gr, uint32_t &err) {
    static_assert(UF_GLOBAL || !TG, "tables in HBM imply the HBM union-find");
    constexpr int NT = W * 64;
    const Tab<TG> T = make_tab<TG, W>(B, L, r);
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t N = B.N, nwords = B.nwords;
    UFA<UF_GLOBAL> uf;
    {
        const size_t ids = (size_t)W * N + B.cap;
        uf.gparent = B.uf_scratch + (size_t)r * (ids + 2 * ((ids + 31) / 32));
        uf.gfrozen = uf.gparent + ids;
        uf.gfroot = uf.gfrozen + (ids + 31) / 32;
        uf.o_parent = L.o_parent; uf.o_frozen = L.o_frozen; uf.o_froot = L.o_froot;
    }
    for (uint32_t i = tid; i < nwords; i += NT) LDSW(L.o_touch, i) = 0u;
    for (uint32_t i = tid; i < (N + 3) / 4; i += NT) T.st32(T.touch8, i, 0u);
    if (tid == 0) { LDSW(L.o_misc, MISC_NCLUST) = 0u; LDSW(L.o_misc, MISC_ANYFROZEN) = 0u; }
    if (n == 0) { __syncthreads(); return 0u; } // cluster.rs:46-48
    SSE_STAMP_INIT;
    { // the scan stores 16-bit cut ranks per wave range: every range must hold fewer than 65535 cuts
        const uint32_t used = (M + B.CH - 1) / B.CH, q = (used + W - 1) / W;
        uint32_t bad = 0;
        for (uint32_t w2 = 0; w2 < (uint32_t)W; ++w2) {
            uint32_t cuts = 0;
            for (uint32_t c = min(w2 * q, used); c < min(w2 * q + q, used); ++c) cuts += LDSW(L.o_chtr, c);
            bad |= (cuts >= 65535u);
        }
        if (bad) { err = SSE_ERR_SCAN_RANGE; return 0u; }
    }
    const uint32_t C = (uint32_t)ntrans;            // one id per cut (transverse op)
    const uint32_t S = N + C + (uint32_t)(W - 1) * N; // + artificial range-boundary placeholders
    for (uint32_t i = tid; i < N; i += NT) uf.set(i, i);
    for (uint32_t i = tid; i < (uint32_t)(W - 1) * N; i += NT) uf.set(N + C + i, N + C + i);
    if (B.has_long) for (uint32_t i = tid; i < (S + 31) / 32; i += NT) uf.bits_clear(i);
    __syncthreads();
    // ---- build: label legs with segment ids, union through non-boundary ops ----
    SSE_STAMP(0);
    cluster_scan<W, K, CL, false, UF_GLOBAL, TG, PM>(B, L, r, M, uf, C);
    // touched bytes -> bits (read by the coins, the p=0 state update and the free-spin pass, all behind later barriers)
    for (uint32_t i = tid; i < nwords; i += NT) {
        uint32_t bits = 0;
        if constexpr (TG) { // the touched byte of every wave's record of the variable
            for (uint32_t k = 0; k < 32 && i * 32 + k < N; ++k) {
                uint32_t t = 0;
                for (uint32_t w2 = 0; w2 < (uint32_t)W; ++w2) t |= T.rec_ld(w2 * N + i * 32 + k) >> 24;
                bits |= (t & 1u) << k;
            }
        } else
        for (uint32_t k = 0; k < 8 && (i * 8 + k) < (N + 3) / 4; ++k) {
            const uint32_t w = T.ld32(T.touch8, i * 8 + k);
            bits |= ((w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u)) << (4 * k);
        }
        LDSW(L.o_touch, i) = bits;
    }
    SSE_STAMP(1);
    // join the ranges: the segment v is in when wave w's range ends continues into P(w+1,v); the last
    // range wraps around into P(0,v) (cluster.rs:223-242: worldlines are cyclic in imaginary time)
    for (uint32_t i = tid; i < (uint32_t)W * N; i += NT) {
        const uint32_t w2 = i / N, v = i - w2 * N;
        const uint32_t x = TG ? (T.rec_ld(i) & 0xFFFFu) : T.ld16(T.cur, i);
        const uint32_t last = x ? LDSW(L.o_chg, w2) + x : 0u;
        const uint32_t seg_end = last ? last : (w2 == 0 ? v : N + C + (w2 - 1) * N + v);
        const uint32_t nxt = (w2 + 1 == (uint32_t)W) ? v : N + C + w2 * N + v;
        if (seg_end != nxt) uf_union(uf, seg_end, nxt);
    }
    __syncthreads();
    SSE_STAMP(2);
    // ---- flatten: parent[i] := exact root (no union runs any more), frozen marks move to roots ----
    for (uint32_t i = tid; i < S; i += NT) {
        const uint32_t root = uf_find_ro(uf, i); // no halving stores here: only exact roots may be written
        uf.set(i, root);
        if (B.has_long && ((uf.frozen_get(i >> 5) >> (i & 31)) & 1u)) { uf.froot_or(root >> 5, 1u << (root & 31)); LDSW(L.o_misc, MISC_ANYFROZEN) = 1u; }
    }
    __syncthreads();
    SSE_STAMP(3);
    // ---- coins: one Philox draw per ROOT (= per cluster), then parent[i] := flip bit of its root, in place ----
    // LDS path: the roots are compacted into a list (wave ballot + one LDS counter) so that the draws run on dense
    // lanes; the list lives in the cut-marker tables and the flip bits in the cut-rank tables, both free after the
    // join.  Too many roots or ids for those tables (or no cut at all, or the HBM union-find): every id draws the
    // coin of its root itself — same results, more Philox calls.
    uint32_t myclusters = 0;
    const bool nocuts = (C == 0u);
    const uint32_t anyfrozen = LDSW(L.o_misc, MISC_ANYFROZEN);
    bool dense_done = false;
    // HBM union-find: the flip bit of every id also goes into LDS when the launch has room for S bits behind its fixed regions
    // (the region where the LDS union-find keeps its parents, unused on this path); the apply pass then needs no HBM lookups
    const bool lds_flips = UF_GLOBAL && B.segs2 != nullptr && S <= B.lds_flipcap; // (uniform)
    if (lds_flips) {
        for (uint32_t i = tid; i < (S + 31u) / 32u; i += NT) LDSW(L.o_parent, i) = 0u;
        __syncthreads();
    }
    if constexpr (!UF_GLOBAL) {
        const uint32_t list_cap = ((uint32_t)W * N + 3u) / 4u * 2u;  // u16 entries in the o_cl words
        const uint32_t bits_cap = ((uint32_t)W * N + 1u) / 2u * 32u; // bits in the o_cur words
        if (!nocuts && S <= bits_cap) {
            for (uint32_t i = tid; i < (S + 31u) / 32u; i += NT) LDSW(L.o_cur, i) = 0u;
            if (tid == 0) LDSW(L.o_misc, MISC_LOOP_A) = 0u;
            __syncthreads();
            for (uint32_t i0 = 0; i0 < S; i0 += NT) { // whole waves iterate together (ballot below)
                const uint32_t i = i0 + tid;
                const bool inr = i < S;
                const uint32_t root = inr ? uf.get(i) : 0xFFFFFFFFu;
                const bool isroot = inr & (root == i);
                if (isroot & (i < N + C)) {
                    const bool touched = (i >= N) || ((LDSW(L.o_touch, i >> 5) >> (i & 31)) & 1u);
                    if (touched) myclusters++;
                }
                const uint64_t m = sse_ballot(isroot);
                if (m) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&LDSW(L.o_misc, MISC_LOOP_A), (uint32_t)popc64(m));
                    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                    const uint32_t pos = base + popc64(m & lanemask_lt(lane));
                    if (isroot && pos < list_cap) LDSH(L.o_cl, pos) = (uint16_t)i;
                }
            }
            __syncthreads();
            const uint32_t nroots = LDSW(L.o_misc, MISC_LOOP_A);
            if (nroots <= list_cap) { // uniform: every thread read the same counter
                for (uint32_t k = tid; k < nroots; k += NT) {
                    const uint32_t root = LDSH(L.o_cl, k);
                    const uint4 o = rng.draw(SSE_TAG_CLUSTER, root);
                    const uint32_t isfrozen = B.has_long ? (uf.froot_get(root >> 5) >> (root & 31)) & 1u : 0u;
                    if (!isfrozen && u01(o.x) < prob) atomicOr(&LDSW(L.o_cur, root >> 5), 1u << (root & 31));
                }
                __syncthreads();
                for (uint32_t i = tid; i < S; i += NT) {
                    const uint32_t root = uf.get(i);
                    uf.set(i, (LDSW(L.o_cur, root >> 5) >> (root & 31)) & 1u);
                }
                dense_done = true;
            } else myclusters = 0; // counted again below
        }
    }
    if (!dense_done)
    for (uint32_t i = tid; i < S; i += NT) {
        const uint32_t root = uf.get(i);
        const uint32_t vi = i < N ? i : (i - N - C) % N; // variable of a placeholder id (nocuts: every id is one)
        const bool touched = (i >= N && !nocuts) || ((LDSW(L.o_touch, vi >> 5) >> (vi & 31)) & 1u);
        uint32_t f;
        if (nocuts) {
            // no cluster boundary anywhere: the whole graph is one cluster (cluster.rs:98-107), label 0
            const uint4 o = rng.draw(SSE_TAG_CLUSTER, 0u);
            f = (touched && !anyfrozen && u01(o.x) < prob) ? 1u : 0u;
        } else {
            if (root == i && touched && i < N + C) myclusters++;
            const uint4 o = rng.draw(SSE_TAG_CLUSTER, root);
            const uint32_t isfrozen = B.has_long ? (uf.froot_get(root >> 5) >> (root & 31)) & 1u : 0u;
            f = (!isfrozen && u01(o.x) < prob) ? 1u : 0u;
        }
        uf.set(i, f);
        if (lds_flips && f) atomicOr(&LDSW(L.o_parent, i >> 5), 1u << (i & 31u));
    }
    {
        uint32_t c = myclusters;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
        if (lane == 0 && c) atomicAdd(&LDSW(L.o_misc, MISC_NCLUST), c);
    }
    __syncthreads();
    SSE_STAMP(4);
    // ---- apply (cluster.rs:139-167) ----
    if constexpr (UF_GLOBAL) {
        if (lds_flips) cluster_apply_cached<W, K, CL, true, PM, true>(B, L, r, M, uf);
        else if (B.segs2) cluster_apply_cached<W, K, CL, true, PM>(B, L, r, M, uf); // both ids of every slot were stored by the build scan
        else cluster_scan<W, K, CL, true, UF_GLOBAL, TG, PM>(B, L, r, M, uf, C);  // (a replica that outgrew the LDS union-find before the host planned for it)
    } else cluster_apply_cached<W, K, CL, false, PM>(B, L, r, M, uf);
    SSE_STAMP(5);
    // p=0 state follows the placeholder segment of each touched variable
    for (uint32_t i = tid; i < nwords; i += NT) {
        uint32_t x = 0;
        const uint32_t t = LDSW(L.o_touch, i);
        for (uint32_t j = 0; j < 32 && i * 32 + j < N; ++j) x |= (uf.get(i * 32 + j) & 1u) << j;
        LDSW(L.o_state, i) ^= (x & t);
    }
    __syncthreads();
    return nocuts ? 1u : LDSW(L.o_misc, MISC_NCLUST);
}

// touched-variable scan for launches that flip free spins without a preceding cluster pass
template <int W, bool CL, bool PM = false>
__device__ __forceinline__ void touch_scan(const DevBatch &B, const Lds<W> &L, uint32_t r, uint32_t M) {
    constexpr int NT = W * 64;
    const int tid = threadIdx.x;
    const uint32_t *ops = B.ops + (size_t)r * B.stride;
    for (uint32_t i = tid; i < B.nwords; i += NT) LDSW(L.o_touch, i) = 0u;
    __syncthreads();
    for (uint32_t p0 = 0; p0 < M; p0 += 4 * NT) {
        uint32_t wd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const uint32_t p = p0 + j * NT + tid; wd[j] = p < M ? ops[p] : 0u; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!wd[j]) continue;
            const Bd d = decode_bond<CL, W, PM>(B, L, sse_op_bond(wd[j]));
            atomicOr(&LDSW(L.o_touch, d.a >> 5), 1u << (d.a & 31));
            if (d.c != SSE_NO_VAR) atomicOr(&LDSW(L.o_touch, d.c >> 5), 1u << (d.c & 31));
        }
    }
    __syncthreads();
}

// qmc_ising.rs:780-784 / qmc_runner.rs:241-255
template <int W>
__device__ __forceinline__ void free_spin_pass(const DevBatch &B, const Lds<W> &L, const Rng &rng) {
    constexpr int NT = W * 64;
    const int tid = threadIdx.x;
    for (uint32_t i = tid; i < B.nwords; i += NT) {
        const uint32_t t = LDSW(L.o_touch, i);
        uint32_t s = LDSW(L.o_state, i);
        for (uint32_t j = 0; j < 32 && i * 32 + j < B.N; ++j)
            if (!((t >> j) & 1u)) {
                const uint4 o = rng.draw(SSE_TAG_FREE, i * 32 + j);
                s = (s & ~(1u << j)) | ((o.x >> 31) << j);
            }
        LDSW(L.o_state, i) = s;
    }
    __syncthreads();
}

} // namespace sse
