// sse_diag.hip.h — the general diagonal pass (sse::sweep_kernel, sse_sweep.hip.h; the trimmed one of the headline geometry is sse_fast.hip.h).
#pragma once
#include "sse_core.hip.h"

namespace sse {

// Diagonal pass.  Reference: DiagonalUpdater::make_diagonal_update_with_rng_and_state_ref
// (qmc_traits/diagonal.rs:114-135) with metropolis_single_diagonal_update (:142-191), or the heat-bath
// rule (qmc_traits/heatbath.rs:149-209) when HB.
//
// The slot rule depends on the live operator count n, which makes the sweep sequential in p.  One tile of
// W*64*K slots is decided by a fixed-point iteration instead: every candidate slot evaluates its rule with
// n = (count at the tile start) + (net accepted candidates at earlier slots of the tile), starting from "none
// accepted", until no decision changes.  The fixed point is unique and equal to the sequential result (the
// decision of slot p only depends on decisions at slots < p), and it is reached in 2 rounds almost always
// because n moves by a few units inside a tile while the rule compares against M - n ~ 1e4..1e5.
//
// Per slot and round the work is: one int->f64 convert, one f64 multiply, two f64 compares (written straight to
// wave masks), the mask algebra on the scalar unit, and four mbcnt for the prefix counts.  All compares are the
// IEEE f64 expressions of oracle/sse_oracle.c (built with -ffp-contract=off on both sides).
template <int W, int K, bool CL, bool HB, bool TG, bool PM = false>
__device__ __forceinline__ void diagonal_pass(const DevBatch &B, const Lds<W> &L, uint32_t r, const Rng &rng, double beta, uint32_t M,
                              int &n_io, int &ntrans_io, uint32_t &gr) {
    constexpr int NT = W * 64;
    const Tab<TG> T = make_tab<TG, W>(B, L, r);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6); // scalar: keeps per-wave control flow uniform
    uint32_t *ops = B.ops + (size_t)r * B.stride;
    const double beta_nb = beta * (double)B.Nb;
    const double hb_bw = beta * B.wtot;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    // CL mode (uniform |J|): the three bond weights and beta*Nb times them, as vector-register constants
    double wJv = 0, wGv = 0, wHv = 0, nJv = 0, nGv = 0, nHv = 0;
    if constexpr (CL) {
        wJv = vgpr_copy(B.wJ); wGv = vgpr_copy(B.gamma); wHv = vgpr_copy(B.wh);
        nJv = vgpr_copy(beta_nb * B.wJ); nGv = vgpr_copy(beta_nb * B.gamma); nHv = vgpr_copy(beta_nb * B.wh);
    }
    // a few scalars every sub-round needs, pinned into vector registers: the pass is short of scalar registers (they
    // were being spilled to vector lanes and read back with v_readlane once per use) and has vector registers to spare
    const uint32_t pE = vgpr_copy_u32(B.E), pN = vgpr_copy_u32(B.N), pNb = vgpr_copy_u32(B.Nb), pM = vgpr_copy_u32(M);
    // Per-wave spin tables T_w[v] (u8, in the o_cur area the cluster scan uses later): bit 0 = spin of v at the
    // wave's current position; bits 1..7 = lane+1 of an off-diagonal op on v inside the sub-round being resolved.
    const uint32_t N = B.N, h_my = (uint32_t)wave * N;
    for (uint32_t i = tid; i < (uint32_t)W * N; i += NT) {
        const uint32_t v = i % N;
        T.st8(T.cur, i, (LDSW(L.o_state, v >> 5) >> (v & 31)) & 1u);
    }
    __syncthreads();

    const uint32_t ntiles = (M + NT * K - 1) / (NT * K);
    int n_start = n_io, ntrans = 0;

    // off-diagonal ops ("events") of a tile's words: which of the op's variables flip.  Ising bonds: only single-site ops
    // can be off-diagonal (bit 0 of in^out); generic two-variable interactions (never in CL mode) may flip either.
    auto event_of = [&](uint32_t wd, uint32_t &va, uint32_t &vc, bool &fc) -> bool {
        const uint32_t xb = sse_op_in(wd) ^ sse_op_out(wd);
        const bool fa = (xb & 1u) != 0u;
        fc = CL ? false : ((xb & 2u) != 0u);
        if constexpr (CL) { // only one-variable ops flip a spin here: their variable follows from the bond number alone
            const uint32_t s1 = sse_op_bond(wd) - B.E;
            va = fa ? (s1 < B.N ? s1 : s1 - B.N) : 0u;
            vc = va;
        } else {
            const Bd d = decode_bond<CL, W, PM>(B, L, (fa | fc) ? sse_op_bond(wd) : 0u);
            va = d.a; vc = d.c != SSE_NO_VAR ? d.c : d.a;
        }
        return fa;
    };
    // flip the spin of the event variables in the tables of waves [wlo, whi) (wave-uniform bounds)
    auto propagate = [&](const uint32_t (&var)[K], const bool (&ev)[K], int wlo, int whi) {
        if ((N & 3u) == 0u) { // tables start on word boundaries: word index and bit inside a table do not depend on the wave
            uint32_t widx[K], bit[K];
#pragma unroll
            for (int j = 0; j < K; ++j) { widx[j] = var[j] >> 2; bit[j] = 1u << ((var[j] & 3u) * 8u); }
            for (int w2 = wlo; w2 < whi; ++w2) {
                const uint32_t tbl = (uint32_t)w2 * (N >> 2); // word index of wave w2's table inside the region
#pragma unroll
                for (int j = 0; j < K; ++j)
                    if (ev[j]) T.xor32(T.cur, tbl + widx[j], bit[j]);
            }
        } else {
            for (int w2 = wlo; w2 < whi; ++w2) {
                const uint32_t base = (uint32_t)w2 * N;
#pragma unroll
                for (int j = 0; j < K; ++j)
                    if (ev[j]) T.xor32(T.cur, (base + var[j]) >> 2, 1u << (((base + var[j]) & 3u) * 8u));
            }
        }
    };

    // Loads and stores of whole tiles are unconditional and branch-free: rows are padded to a whole number of
    // tiles (DevBatch::stride) and slots >= M hold 0, so a partial last tile reads zeros and writes them back.
    // (Predicated loads put every access into its own basic block, and the compiler then waits for ALL
    // outstanding memory operations before the first use — i.e. for the prefetch it has just issued.)
    uint32_t wnext[K];
    // prologue: tile 0 words; their events go to the tables of later waves
#pragma unroll
    for (int j = 0; j < K; ++j) wnext[j] = row_ld(ops, slot_of<W, K>(0, wave, j, lane));
    {
        uint32_t var[K], var2[K]; bool ev[K], ev2[K];
#pragma unroll
        for (int j = 0; j < K; ++j) ev[j] = event_of(wnext[j], var[j], var2[j], ev2[j]);
        propagate(var, ev, wave + 1, W);
        if constexpr (!CL) propagate(var2, ev2, wave + 1, W);
    }
    __syncthreads();

    SSE_STAMP_INIT;
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
#ifdef SSE_GEN_ROTATE
        sse_set_prio(tile / SSE_GEN_ROTATE + blockIdx.x);
#endif
        SSE_STAMP(11);
        uint32_t word[K];
#pragma unroll
        for (int j = 0; j < K; ++j) word[j] = wnext[j];
        {   // prefetch the next tile (after the last one: the same tile again, the values are not used)
            const uint32_t tn = tile + 1 < ntiles ? tile + 1 : tile;
#pragma unroll
            for (int j = 0; j < K; ++j) wnext[j] = row_ld(ops, slot_of<W, K>(tn, wave, j, lane));
        }

        // per slot, kept across the rounds:
        //   fa, fb : f64 operands of the rule (see the rounds below); fa = +inf when the slot is not a candidate
        //   cb     : M (insert candidate) or M + 1 (removal candidate), so that the rule's den is cb - n
        //   cw     : the op word to store when the candidate is accepted (new diagonal op, or 0 for a removal);
        //   keep   : the word to store otherwise (what the slot holds now)
        double fa[K], fb[K];
        uint32_t cb[K], cw[K], keep[K], evA[K], evC[K];
        bool isevj[K], isevc[K];
        uint64_t insm[K]; // insert candidates
        uint32_t trbits = 0; // bit j: the op at stake in sub-round j is a transverse-field op
        uint4 rnd = make_uint4(0, 0, 0, 0);
        // random numbers and bond of slot j (shared by the two loops below)
        auto draw_bond = [&](int j, uint32_t p, uint32_t wd, bool occ, bool is_empty, uint32_t &r0, uint32_t &r1) -> uint32_t {
            uint32_t r2 = 0;
            if (HB) {
                rnd = rng.draw(SSE_TAG_HEATBATH, p);
                r0 = rnd.x; r1 = rnd.y; r2 = rnd.z;
            } else {
                // slots p and p^64 share one Philox call (include/sse_format.h)
                if (K == 1 || (j & 1) == 0) rnd = rng.draw(SSE_TAG_DIAG, p & ~64u);
                const bool hi = (K == 1) ? ((p & 64u) != 0u) : ((j & 1) != 0);
                r0 = hi ? rnd.z : rnd.x; r1 = hi ? rnd.w : rnd.y;
            }
            uint32_t b;
            if (HB) {
                b = 0;
                if (occ) b = sse_op_bond(wd);
                else if (is_empty) {
                    const double c = u01(r2) * B.wtot;
                    uint32_t lo = 0, hi2 = B.Nb;
                    while (lo < hi2) { const uint32_t mid = lo + ((hi2 - lo) >> 1); if (B.cumw[mid] < c) lo = mid + 1; else hi2 = mid; }
                    b = lo < B.Nb ? lo : B.Nb - 1;
                }
            } else {
                b = occ ? sse_op_bond(wd) : __umulhi(r0, pNb);
            }
            return b;
        };
        // General bond table (non-uniform couplings, per-replica couplings, generic interactions): the 16-byte records live
        // in HBM/L2, so all K of a tile are requested before the first one is used (a load inside the sub-round loop would
        // expose its full latency K times per tile).
        uint32_t pre_b[K], pre_r0[K], pre_r1[K];
        uint4 pre_rec[K];
        if constexpr (!CL) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t p = slot_of<W, K>(tile, wave, j, lane);
                const uint32_t wd = word[j];
                pre_b[j] = draw_bond(j, p, wd, wd != 0u, (p < pM) & (wd == 0u), pre_r0[j], pre_r1[j]);
                pre_rec[j] = bond_rec<PM, W>(B, L, pre_b[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint32_t p = slot_of<W, K>(tile, wave, j, lane);
            const uint32_t wd = word[j];
            const bool occ = wd != 0u;
            const uint32_t inb = sse_op_in(wd) & 1u, inc = (sse_op_in(wd) >> 1) & 1u;
            const uint32_t xbits = sse_op_in(wd) ^ sse_op_out(wd);
            const bool flipa = (xbits & 1u) != 0u;                        // the op flips its first variable
            const bool flipc = CL ? false : ((xbits & 2u) != 0u);          // ... its second (generic interactions only)
            const bool isev = flipa | flipc;
            const bool is_empty = (p < pM) & !occ;
            const bool is_diag = occ & !isev;
            uint32_t r0, r1, b;
            if constexpr (CL) b = draw_bond(j, p, wd, occ, is_empty, r0, r1);
            else { b = pre_b[j]; r0 = pre_r0[j]; r1 = pre_r1[j]; }
            // bond -> variables, kind, preferred alignment, weight w and beta*Nb*w
            uint32_t va, vc, pref;
            bool two, tr;
            double wbond, nbond;
            if constexpr (CL) {
                two = b < pE;
                const uint32_t e = LDSW(L.o_edges, two ? b : 0u);
                const uint32_t s1 = b - pE;  // wraps far above N for two-site bonds
                tr = s1 < pN;
                va = two ? (e & SSE_CE_VAR_MASK) : (tr ? s1 : s1 - pN);
                vc = two ? ((e >> 15) & SSE_CE_VAR_MASK) : va;
                pref = two ? ((e >> 30) & 1u) : B.hpos;
                wbond = two ? wJv : (tr ? wGv : wHv);
                nbond = two ? nJv : (tr ? nGv : nHv);
            } else {
                Bd d;
                { const uint4 q = pre_rec[j]; d.a = q.x & SSE_VAR_MASK; d.c = q.y; d.kp = q.x >> SSE_INFO_SHIFT; d.w = __hiloint2double((int)q.w, (int)q.z); }
                two = d.c != SSE_NO_VAR;
                tr = bd_kind(d) == SSE_BOND_TRANSVERSE;
                va = d.a; vc = two ? d.c : va;
                pref = (d.kp >> 2) & 1u;
                wbond = d.w;
                nbond = beta_nb * d.w;
            }
            const bool generic = !CL && B.mats != nullptr; // wave-uniform
            evA[j] = va; isevj[j] = flipa; evC[j] = vc; isevc[j] = flipc;
            trbits |= tr ? (1u << j) : 0u;
            // Spins at this slot = table value, corrected for the off-diagonal ops at EARLIER lanes of this
            // sub-round.  The op word itself carries the spin before (in) and after (out), so the event lanes
            // publish (lane+1, in) in the table, everybody reads, then they store the spin after their op.  Two
            // events on one variable inside a sub-round are rare; a serial loop over the event lanes handles them.
            const uint64_t ev0 = SSE_DBG(B, 16u) ? 0ull : sse_ballot(isev);
            if (ev0) {
                if (flipa) T.st8(T.cur, h_my + va, (((uint32_t)lane + 1u) << 1) | inb);
                if (flipc) T.st8(T.cur, h_my + vc, (((uint32_t)lane + 1u) << 1) | inc);
                SSE_WAVE_FENCE();
            }
            const uint32_t ea = T.ld8(T.cur, h_my + va), ec = T.ld8(T.cur, h_my + vc);
            uint32_t sa = ea & 1u, sc = ec & 1u;
            if (ev0) {
                const uint32_t La = ea >> 1, Lc = ec >> 1;
                const uint64_t dup = sse_ballot((flipa & (La != (uint32_t)lane + 1u)) | (flipc & (Lc != (uint32_t)lane + 1u)));
                if (!dup) {
                    sa ^= (uint32_t)((La - 1u) < (uint32_t)lane); // La == 0: no event on the variable
                    sc ^= (uint32_t)((Lc - 1u) < (uint32_t)lane);
                    SSE_WAVE_FENCE();
                    if (flipa) T.st8(T.cur, h_my + va, inb ^ 1u);
                    if (flipc) T.st8(T.cur, h_my + vc, inc ^ 1u);
                } else {
                    bool seen_a = false, seen_c = false;
                    uint64_t m = ev0;
                    while (m) {
                        const int Ls = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const bool later = lane > Ls;
                        // up to two flipped variables per event lane (different variables of one op: order irrelevant)
                        for (int which = 0; which < (CL ? 1 : 2); ++which) {
                            const uint32_t fL = __builtin_amdgcn_readlane(which ? (uint32_t)flipc : (uint32_t)flipa, Ls);
                            if (!fL) continue; // wave-uniform
                            const uint32_t vL = __builtin_amdgcn_readlane(which ? vc : va, Ls);
                            const uint32_t inL = __builtin_amdgcn_readlane(which ? inc : inb, Ls);
                            if (va == vL) { sa = later ? (inL ^ 1u) : (seen_a ? sa : inL); seen_a = true; }
                            if (vc == vL) { sc = later ? (inL ^ 1u) : (seen_c ? sc : inL); seen_c = true; }
                            if (lane == Ls) T.st8(T.cur, h_my + vL, inL ^ 1u); // in order: the last event wins
                        }
                    }
                    SSE_WAVE_FENCE();
                }
            }
            const uint32_t sub = sa | (two ? (sc << 1) : 0u);
            // Would a diagonal op on this bond have non-zero weight here (qmc_ising.rs:863-888)?  Two-site: the spins'
            // alignment equals the bond's preference; longitudinal: the spin equals the field's; transverse: always.
            // An op already in the string has its bond's weight (it was inserted with non-zero weight and the string
            // is consistent).
            const uint32_t agree = two ? ((sa ^ sc) ^ 1u) : sa;
            bool ok = tr | (agree == pref);
            double w_gen = 0.0;
            if constexpr (!CL) if (generic) {
                // Interaction::at (qmc_runner.rs:573-612): the weight of the op at stake — the diagonal op that would be
                // inserted (state sub) or the diagonal op in the slot (its own bits)
                const uint32_t st = is_empty ? sub : sse_op_in(wd);
                w_gen = B.mats[(size_t)b * 16u + (st | (st << 2))];
                nbond = beta_nb * w_gen;
                ok = true;
            }
            const double uacc = u01(HB ? r0 : r1);
            bool ins;
            if (HB) {
                // insert: u*(den + bW) < bW after the bond was chosen and kept with u1*maxw < w (heatbath.rs:163-193)
                const double w_ins = generic ? w_gen : (ok ? wbond : 0.0);
                ins = is_empty & (u01(r1) * wbond < w_ins);
                fa[j] = (ins | is_diag) ? uacc : inf;
                fb[j] = 0.0;
            } else {
                ins = is_empty & ok & (nbond > 0.0);
                // insert: u*den < num          (fa = u, fb = num)
                // remove: u*num < den          (fa = u*num)
                fa[j] = ins ? uacc : (is_diag ? uacc * nbond : inf);
                fb[j] = nbond;
            }
            insm[j] = sse_ballot(ins);
            cb[j] = pM + (ins ? 0u : 1u);
            cw[j] = ins ? sse_op_make(b, sub, sub) : 0u;
            keep[j] = wd;
        }

        SSE_STAMP(8);
        // ---- fixed point on n ----
        int npref[K];
#pragma unroll
        for (int j = 0; j < K; ++j) npref[j] = n_start;
        uint64_t acc[K], accp[K];
#pragma unroll
        for (int j = 0; j < K; ++j) accp[j] = 0ull;
        int tot_all = 0;
        bool first = true;
        for (;;) {
            int wtot = 0;
            bool changed = first;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double t = (double)(int)(cb[j] - (uint32_t)npref[j]); // den of the rule
                uint64_t lt_ins, lt_rem;
                if (HB) {
                    const double lhs = fa[j] * (t + hb_bw);
                    lt_ins = sse_ballot(lhs < hb_bw);
                    lt_rem = sse_ballot(lhs < t);
                } else {
                    lt_ins = sse_ballot(fa[j] * t < fb[j]);
                    lt_rem = sse_ballot(fa[j] < t);
                }
                acc[j] = (lt_ins & insm[j]) | (lt_rem & ~insm[j]);
                changed |= acc[j] != accp[j];
                wtot += popc64(acc[j] & insm[j]) - popc64(acc[j] & ~insm[j]);
            }
            const int buf = gr & 1;
            if (lane == 0) { LDSI(L.o_tot, buf * W + wave) = wtot; LDSW(L.o_chg, buf * W + wave) = changed ? 1u : 0u; }
            __syncthreads();
            if (first && !SSE_DBG(B, 8u)) {
                // events of this tile -> tables of earlier waves (all readers of this tile are done);
                // events of the next tile -> tables of later waves (visible after the next barrier)
                propagate(evA, isevj, 0, wave);
                if constexpr (!CL) propagate(evC, isevc, 0, wave);
                if (tile + 1 < ntiles) {
                    uint32_t var[K], var2[K]; bool ev[K], ev2[K];
#pragma unroll
                    for (int j = 0; j < K; ++j) ev[j] = event_of(wnext[j], var[j], var2[j], ev2[j]);
                    propagate(var, ev, wave + 1, W);
                    if constexpr (!CL) propagate(var2, ev2, wave + 1, W);
                }
            }
            // every lane reads the same words: move them to scalar registers so that the loop stays wave-uniform
            // (the compiler cannot see that an LDS value is the same in all lanes)
            int base = 0; tot_all = 0; uint32_t anychg = 0;
#pragma unroll
            for (int w2 = 0; w2 < W; ++w2) {
                const int t = __builtin_amdgcn_readfirstlane(LDSI(L.o_tot, buf * W + w2));
                if (w2 < wave) base += t;
                tot_all += t;
                anychg |= (uint32_t)__builtin_amdgcn_readfirstlane((int)LDSW(L.o_chg, buf * W + w2));
            }
            gr++;
#ifdef SSE_PHASE_TIMING
            if (threadIdx.x == 0) B.dbg[(size_t)r * 16 + 13] += 1; // rounds
#endif
            if (SSE_DBG(B, 4u)) break;
            if (!first && !anychg) break;
            first = false;
            int run = n_start + base;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint64_t im = acc[j] & insm[j], rm = acc[j] & ~insm[j];
                npref[j] = run + popc64(im & lanemask_lt(lane)) - popc64(rm & lanemask_lt(lane));
                run += popc64(im) - popc64(rm);
                accp[j] = acc[j];
            }
        }
        SSE_STAMP(9);
#ifdef SSE_PHASE_TIMING
        if (threadIdx.x == 0) B.dbg[(size_t)r * 16 + 12] += 1; // tiles
#endif
        // ---- commit ----
        int dn = 0, dtr = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            row_st(ops, slot_of<W, K>(tile, wave, j, lane), ((acc[j] >> lane) & 1ull) ? cw[j] : keep[j]);
            const uint64_t im = acc[j] & insm[j], rm = acc[j] & ~insm[j];
            const uint64_t trm = sse_ballot((trbits >> j) & 1u);
            dn += popc64(im) - popc64(rm);
            dtr += popc64(im & trm) - popc64(rm & trm);
        }
        ntrans += dtr;
        if (lane == 0 && (dtr | dn)) { // a wave's 64*K slots of a tile lie inside one chunk (CH is a multiple of 256 >= 64*K)
            const uint32_t ch = slot_of<W, K>(tile, wave, 0, 0) / B.CH;
            if (dn) atomicAdd(&LDSW(L.o_chn, ch), (uint32_t)dn);
            if (dtr) atomicAdd(&LDSW(L.o_chtr, ch), (uint32_t)dtr);
        }
        n_start += tot_all;
    }
    // per-wave transverse deltas -> block total
    __syncthreads();
    if (lane == 0) LDSI(L.o_tot, wave) = ntrans;
    __syncthreads();
    int dt = 0;
#pragma unroll
    for (int w2 = 0; w2 < W; ++w2) dt += LDSI(L.o_tot, w2);
    __syncthreads();
    ntrans_io += dt;
    n_io = n_start;
}

} // namespace sse
