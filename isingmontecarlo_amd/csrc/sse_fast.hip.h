// sse_fast.hip.h — the diagonal sweep of the headline geometry, written for instruction count.
//
// Same algorithm, same Philox counters and bit-identical results as sse::diagonal_pass<4, K, CL = true, HB = false> (which stays the
// general implementation and the one the parity tests drive in every other geometry); reference: DiagonalUpdater::
// make_diagonal_update_with_rng_and_state_ref (qmc_traits/diagonal.rs:114-135) with metropolis_single_diagonal_update (:142-191).
// The general pass is VALU-bound at ~270 vector instructions per 64-slot row; this one spends ~110:
//   * ONE packed LDS table entry per bond (two-site, transverse and longitudinal alike) gives both variables, the truth table
//     "does a diagonal op on this bond have weight in spin state (sa, sc)", the state-bit mask of its op word and the weight
//     class — no selects on the bond kind anywhere;
//   * the W = 4 per-wave copies of the propagated spins are the four BYTES of one 32-bit entry per variable, so an
//     off-diagonal op reaches the copies of all later (or all earlier) waves with one ds_xor_b32 instead of a loop of W - 1
//     predicated atomics;
//   * the acceptance rule is exact integer arithmetic (sse_accept.h): per round of the fixed point one 32 x 32 + 64 multiply-add
//     with a sign test (insert) and one integer compare (remove); every lane evaluates both, and a lane that is no candidate
//     carries a constant that never passes, so the two ballots are the accepted masks themselves.  The integer rule equals the
//     oracle's f64 expressions for cutoffs up to 2^21; batches with a larger capacity run the f64 rounds (F64 = true), whose
//     expressions are exactly those of the general pass and of the oracle;
//   * no scalar-register spills: the kernel holds nothing but the diagonal pass (and the short directed loop behind it).
// Requirements (checked by the host, create.hip): uniform |J| (LDS edge tables), N <= 4096 variables, 4 waves per
// replica, Metropolis rule, two launches per timestep.
#pragma once
#include "sse_accept.h"
#include "sse_loop.hip.h"

namespace sse {

#define SSE_FAST_MAX_VARS 4096u
#define LDS8(a) (reinterpret_cast<uint8_t *>(lds_raw)[(a)]) // byte at LDS byte address a
// packed bond entry: a [0,12) | c [12,24) (= a for one-variable bonds) | ok4 [24,28): bit (sa | sc << 1) set iff a diagonal op
// has non-zero weight in that state | submask [28,30): state bits an op word of this bond carries (3 or 1) | class [30,32)
#define SSE_FAST_CLASS_J 0u
#define SSE_FAST_CLASS_G 1u
#define SSE_FAST_CLASS_H 2u

// bitfield insert: (a & mask) | (b & ~mask)
// (as an instruction: written in C the optimiser turns it back into compare + select, the very thing it is here to avoid)
__device__ __forceinline__ uint32_t bfi32(uint32_t mask, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(mask), "v"(a), "v"(b));
    return r;
}

struct FastLds {
    uint32_t o_nb;   // [4] 16 bytes per class, num = beta*Nb*weight: u64 2^63 - ceil(num * 2^32) (sse_accept.h; F64 rounds: f64 num * 2^32)
                     // and f64 num * 2^-32 (the 2^-32 of the uniform folded in)
    uint32_t o_xch;  // [2][4] per-wave (operator-count change << 1) | changed of a round, double buffered by round parity: the
                     // two 16-byte aligned groups inside the 16 words of the general pass' o_tot / o_chg (no LDS of its own)
    uint32_t o_tab;  // [Nb] packed bond entries
    uint32_t o_spin; // [N] u32: byte w = wave w's copy of the propagated spin (bit 0) + in-row event marker (bits 1..7)
    uint32_t o_dummy; // [64] one word per lane: target of the stores / atomics of lanes that have nothing to store
    uint32_t end;
};
// The tables start where the general layout keeps the compact edge table: the directed loop behind the diagonal pass is the
// only user of that table in this kernel and stages it when the tables below are dead.
template <int W>
__host__ __device__ __forceinline__ FastLds fast_carve(const Lds<W> &L, const DevBatch &B) {
    FastLds F;
    static_assert(4 * W >= 3 + 8, "o_xch: eight words behind an alignment gap of up to three, inside o_tot + o_chg");
    uint32_t base = (L.o_edges + 3u) & ~3u; // 16-byte aligned: the class constants are read as one b128
    F.o_nb = base; base += 16;
    F.o_xch = (L.o_tot + 3u) & ~3u; // 16-byte aligned: a round reads its four words as one b128 (o_tot, o_chg: [2][W] each, adjacent)
    F.o_tab = base; base += B.Nb;
    F.o_spin = base; base += B.N;
    F.o_dummy = base; base += 64;
    F.end = base;
    return F;
}

__device__ __forceinline__ uint32_t fast_entry(const DevBatch &B, uint32_t b, uint32_t ce) {
    if (b < B.E) {
        const uint32_t a = ce & SSE_CE_VAR_MASK, c = (ce >> 15) & SSE_CE_VAR_MASK, pref = (ce >> 30) & 1u;
        return a | (c << 12) | ((pref ? 0x9u : 0x6u) << 24) | (3u << 28) | (SSE_FAST_CLASS_J << 30);
    }
    const uint32_t s1 = b - B.E;
    if (s1 < B.N) return s1 | (s1 << 12) | (0xFu << 24) | (1u << 28) | (SSE_FAST_CLASS_G << 30);
    const uint32_t v = s1 - B.N; // longitudinal: sc == sa, so only states 00 and 11 occur
    return v | (v << 12) | ((B.hpos ? 0x8u : 0x1u) << 24) | (1u << 28) | (SSE_FAST_CLASS_H << 30);
}

template <int K, bool F64>
__device__ __forceinline__ void diagonal_fast(const DevBatch &B, const Lds<4> &L, const FastLds &F, uint32_t r, const Rng &rng, double beta,
                                              uint32_t M, int &n_io, int &ntrans_io, uint32_t &gr, uint32_t fbmask) {
    constexpr int W = 4, NT = W * 64;
    constexpr uint32_t TS = (uint32_t)(NT * K);
    static_assert(K == 2 || K == 4, "rows p and p + 64 share one Philox call");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t *ops = B.ops + (size_t)r * B.stride;
    // pending cluster flips of this replica (fbmask = 0xFF) are applied to every word as it is loaded: one byte per slot, the xor
    // mask of its four state bits (0 for empty slots and beyond the cutoff); fbmask = 0: the string in HBM is current
    // (the byte load is unconditional — a branch would put it into a basic block of its own and cost the prefetch its counted
    // waits; without pending flips it reads bytes of the string itself and the mask drops them)
    const uint8_t *flipb = (fbmask ? B.flipb : reinterpret_cast<const uint8_t *>(B.ops)) + (size_t)r * B.stride;
    auto ld_word = [&](uint32_t idx) -> uint32_t {
        return row_ld(ops, idx) ^ ((uint32_t)*reinterpret_cast<const uint8_t *>(reinterpret_cast<const char *>(flipb) + (size_t)idx) & fbmask);
    };
    const uint32_t N = B.N, Nb = B.Nb, E = B.E;
    for (uint32_t i = tid; i < N; i += NT) LDSW(F.o_spin, i) = ((LDSW(L.o_state, i >> 5) >> (i & 31)) & 1u) * 0x01010101u;
    __syncthreads();

    const uint32_t ntiles = (M + TS - 1) / TS;
    int n_start = n_io, ntrans = 0;
    // bytes of the waves after / before this one in a spin entry (wave-uniform)
    const uint32_t m_later = (uint32_t)((0x0101010100ull << (8 * wave)) & 0xFFFFFFFFull);
    const uint32_t m_earlier = 0x01010101u & ((1u << (8 * wave)) - 1u);
    const uint32_t spin_my = 4u * F.o_spin + (uint32_t)wave; // byte address of this wave's copy of variable 0
    const uint32_t markhi = (127u - (uint32_t)lane) << 1; // marker of an off-diagonal op of this lane (bits 1..7 of its variable's byte)

    // Predicated LDS stores and atomics are written branch-free: lanes that have nothing to do are pointed at a per-lane dummy
    // word instead (an address select costs two integer instructions; an exec-masked store costs a compare, a mask in two
    // scalar registers and an exec save / restore).
    const uint32_t dummy_b = 4u * (F.o_dummy + (uint32_t)lane); // byte address of this lane's dummy word
    // all-ones iff the op word is off-diagonal (CL: only transverse-field ops can be: bit 0 of in ^ out)
    auto evmask32 = [](uint32_t wd) -> uint32_t { return 0u - ((wd ^ (wd >> 2)) & 1u); };
    // Each op word is decoded ONCE, when it is prefetched: byte address of the spin entry that an off-diagonal op flips, or of
    // the lane's dummy word.  The register travels with the word into the next tile and serves both propagations and phase 2
    // (an address different from the dummy is also the only "is off-diagonal" test they need).
    const uint32_t spin_b = 4u * (F.o_spin - 1u - E); // (entry of the variable of transverse bond b: o_spin + b - E, b = (word >> 4) - 1)
    auto decode = [&](uint32_t wd) -> uint32_t { return bfi32(evmask32(wd), spin_b + 4u * (wd >> 4), dummy_b); };
    // flip the spin of the off-diagonal ops among K decoded words in the copies selected by `mask`
    auto propagate = [&](const uint32_t (&vb)[K], uint32_t mask) {
        if (mask == 0u) return; // wave-uniform
#pragma unroll
        for (int j = 0; j < K; ++j) atomicXor(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(lds_raw) + vb[j]), mask);
    };

    uint32_t wnext[K], vnext[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { wnext[j] = ld_word((uint32_t)(wave * 64 * K + j * 64 + lane)); vnext[j] = decode(wnext[j]); }
    propagate(vnext, m_later);
    __syncthreads();
    const uint32_t lane2 = 2u * (uint32_t)lane;
    const uint32_t vzero = vgpr_copy_u32(0u);
    const uint32_t vnever_hi = vgpr_copy_u32((uint32_t)(SSE_ACCEPT_NEVER_INSERT >> 32)), vnever_thr = vgpr_copy_u32((uint32_t)SSE_ACCEPT_NEVER_REMOVE);
    uint32_t ch = (uint32_t)(wave * 64 * K) / B.CH, chpos = (uint32_t)(wave * 64 * K) % B.CH; // chunk of this wave's share of the tile, and its offset in it

    for (uint32_t tile = 0; tile < ntiles; ++tile) {
        // The issue arbiter serves the oldest wave first: of the four workgroups of a CU the first dispatched runs almost as if alone
        // (measured: the four end at 372 / 438 / 511 / 600 us on every CU) and the last one finishes the launch alone on its SIMDs,
        // bound by latency.  Rotating the waves' priorities lets the four progress side by side: they end within 60 us of each other
        // and the launch is 11 % shorter.
#if SSE_ROTATE_PRIO // (0: off — the arbiter's own order, for tools/wg_timeline.py)
        if ((tile & (SSE_ROTATE_PRIO - 1u)) == 0u) sse_set_prio((tile / SSE_ROTATE_PRIO) + blockIdx.x); // (the wave's slot on its SIMD, HW_ID.WAVE_ID, as the phase: no better)
#endif
        uint32_t word[K], vcur[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { word[j] = wnext[j]; vcur[j] = vnext[j]; }
        const uint32_t pbase = tile * TS + (uint32_t)(wave * 64 * K + lane);
        {
            const uint32_t pn = (tile + 1 < ntiles ? pbase + TS : pbase);
#pragma unroll
            for (int j = 0; j < K; ++j) wnext[j] = ld_word(pn + (uint32_t)(j * 64));
        }
        const bool partial = tile * TS + TS > M; // wave-uniform: only the last tile can hold slots >= M

        uint32_t neww[K], ent[K], bnd[K], rr1[K];
        uint64_t acci[K], accr[K]; // accepted inserts / removals of the round before
        // operands of the rule: integer rounds (sse_accept.h) ...
        uint32_t chi[K]; // (high word of the insert constant; candidates of one class share the low word: clo)
        uint32_t clo[K];
        int32_t thr[K];
        // ... or f64 rounds, with the candidate masks that they have to apply
        double un[K], nb[K];
        uint64_t insm[K], remm[K];
        // Lane predicates that have to survive the rounds are wave masks (accepted inserts, accepted removals);
        // everything else is recomputed from the op word with integer arithmetic when needed — the pass is short of scalar
        // registers, and a spilled mask costs a v_readlane per half and use.
        // ---- phase 1, all rows at once (nothing here depends on the spin tables): random numbers, bond, packed table entry
        {
            // one Philox block per pair of rows (bit 6 of the slot index is clear on even rows); the two blocks of a K = 4 tile
            // share one chain of round keys
            uint4 rnds[K / 2];
            if constexpr (K == 4) rng.draw2(SSE_TAG_DIAG, pbase, pbase + 128u, rnds[0], rnds[1]);
            else rnds[0] = rng.draw(SSE_TAG_DIAG, pbase);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t wd = word[j];
                const uint4 rnd = rnds[j / 2];
                const uint32_t r0 = (j & 1) ? rnd.z : rnd.x;
                rr1[j] = (j & 1) ? rnd.w : rnd.y;
                const uint64_t occm = sse_ballot(wd != 0u);
                bnd[j] = sel64(occm, (wd >> 4) - 1u, __umulhi(r0, Nb));
                ent[j] = LDSW(F.o_tab, bnd[j]);
            }
        }
        // ---- phase 2, row after row: the propagated spins of the two variables.  In-row ordering of the off-diagonal ops: they
        // publish (127 - lane, spin before) in their variable's byte, everybody reads, they store the spin after.  A reader's
        // spin is flipped iff the publishing lane is below its own: 127 - L' < lane, i.e. bit 8 of (byte + 2 * lane) — plain
        // integer arithmetic, no compare.  (Rows without such an op run the same code: clean bytes have L' = 0, never a flip.)
        uint32_t sub0[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint32_t e = ent[j], inb = word[j] & 1u;
            const uint32_t va = e & 0xFFFu, vc = (e >> 12) & 0xFFFu;
            const uint32_t adr_a = spin_my + 4u * va, adr_c = spin_my + 4u * vc;
            const uint32_t mark = markhi | inb;
            const uint32_t adr_w = vcur[j] + (uint32_t)wave; // where this lane stores: its variable's byte (= adr_a), or its dummy
            const uint64_t evm = sse_ballot(vcur[j] != dummy_b); // the off-diagonal ops of the row
            LDS8(adr_w) = (uint8_t)mark;
            SSE_WAVE_FENCE();
            const uint32_t ea = LDS8(adr_a), ec = LDS8(adr_c);
            uint32_t sa, sc;
            const uint64_t dup = sse_ballot(ea != mark) & evm; // an off-diagonal op whose marker was overwritten
            if (!dup) {
                sa = (ea ^ ((ea + lane2) >> 8)) & 1u;
                sc = (ec ^ ((ec + lane2) >> 8)) & 1u;
                SSE_WAVE_FENCE();
                LDS8(adr_w) = (uint8_t)(inb ^ 1u);
            } else { // two off-diagonal ops of this row on one variable (rare): resolve in lane order
                sa = ea & 1u; sc = ec & 1u;
                bool seen_a = false, seen_c = false;
                uint64_t m = evm;
                while (m) {
                    const int Ls = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const bool later = lane > Ls;
                    const uint32_t vL = __builtin_amdgcn_readlane(va, Ls), inL = __builtin_amdgcn_readlane(inb, Ls);
                    if (va == vL) { sa = later ? (inL ^ 1u) : (seen_a ? sa : inL); seen_a = true; }
                    if (vc == vL) { sc = later ? (inL ^ 1u) : (seen_c ? sc : inL); seen_c = true; }
                    if (lane == Ls) LDS8(adr_a) = (uint8_t)(inL ^ 1u); // in order: the last one wins
                }
                SSE_WAVE_FENCE();
            }
            sub0[j] = sa | (sc << 1);
        }
        // ---- phase 3, all rows: candidates and the operands of the rule
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint32_t e = ent[j], wd = word[j];
            const uint32_t okbit = (e >> (24u + sub0[j])) & 1u; // a diagonal op on this bond has weight in this spin state
            const uint32_t sub = sub0[j] & (e >> 28) & 3u;
            const uint4 cls = *reinterpret_cast<const uint4 *>(&lds_raw[F.o_nb + 4u * (e >> 30)]);
            const double num_lo = __hiloint2double((int)cls.w, (int)cls.z); // num * 2^-32
            uint64_t im = sse_ballot(okbit > wd); // insert candidates: empty slot (word 0) and okbit 1
            if (partial) im &= sse_ballot(pbase + (uint32_t)(j * 64) < M);
            // removal candidates: occupied and diagonal.  A diagonal op's decoded address is the lane's dummy word, an off-diagonal
            // op's a spin entry, and the spin entries lie below the dummy words (fast_carve): written as a compare of its own, which
            // is one v_cmp here; the ballot of phase 2 (!= dummy_b) asked again comes back as v_cndmask 0/1 + v_cmp_ne
            const uint64_t rm = sse_ballot(wd != 0u) & sse_ballot(vcur[j] >= dummy_b);
            if constexpr (F64) {
                // insert:  (u 2^-32) * den < num   <=>  u * den < num * 2^32  (u is converted again in every round: one
                // instruction against two registers per row held across the rounds)
                // remove:  (u 2^-32) * num < den   with  u * (num 2^-32) == (u 2^-32) * num  bit for bit
                un[j] = (double)rr1[j] * num_lo;
                nb[j] = __hiloint2double((int)cls.y, (int)cls.x);
                insm[j] = im; remm[j] = rm;
            } else {
                // the candidate masks end here: who is no candidate gets the operand that never passes (2^63 in the high word
                // of the insert constant: whatever the low word, rr1 * den + it stays below 2^64 and keeps the sign bit)
                clo[j] = cls.x;
                chi[j] = sel64(im, cls.y, vnever_hi);
                thr[j] = (int32_t)sel64(rm, (uint32_t)sse_accept_remove_threshold(rr1[j], num_lo), vnever_thr);
            }
            // what an accepted candidate leaves in the slot: ((bnd + 1) << 4) | sub | (sub << 2), as a shift-add and a 24-bit multiply-add
            // (sub <= 3: 5 * sub stays below 16, so the sum is the or)
            neww[j] = sel64(im, __umul24(sub, 5u) + ((bnd[j] << 4) + 16u), vzero);
            acci[j] = 0ull; accr[j] = 0ull;
        }

        // ---- fixed point on the live operator count (see diagonal_pass) ----
        // q = M - (live operators in front of the lane's slot): the denominator of an insert; a removal's is q + 1 (no select
        // between the two: an insert candidate is an empty slot, a removal candidate an occupied one)
        uint32_t q[K];
#pragma unroll
        for (int j = 0; j < K; ++j) q[j] = M - (uint32_t)n_start;
        int tot_all = 0, base = 0, wtot = 0;
        bool first = true;
        for (;;) {
            wtot = 0;
            uint64_t diff = 0ull; // lanes whose acceptance changed in this round
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int t = (int)q[j];
                uint64_t ai, ar;
                if constexpr (F64) {
                    ai = sse_ballot((double)rr1[j] * (double)t < nb[j]) & insm[j];
                    ar = sse_ballot(un[j] < (double)(t + 1)) & remm[j];
                } else {
                    ai = sse_ballot(sse_accept_insert(rr1[j], (uint32_t)t, ((uint64_t)chi[j] << 32) | clo[j]));
                    ar = sse_ballot(sse_accept_remove(t + 1, thr[j]));
                }
                diff |= (ai ^ acci[j]) | (ar ^ accr[j]);
                acci[j] = ai; accr[j] = ar;
                wtot += popc64(ai) - popc64(ar);
            }
            // one word per wave and round: every wave reads the four of them back at once
            const bool changed = first | (diff != 0ull);
            const uint32_t xch = F.o_xch + 4u * (gr & 1u);
            if (lane == 0) LDSW(xch, wave) = ((uint32_t)wtot << 1) | (changed ? 1u : 0u);
            __syncthreads();
            if (first) {
                // this tile's off-diagonal ops -> copies of the earlier waves (every reader of this tile is done); the next
                // tile's -> copies of the later waves (visible behind the next barrier, before anybody decodes that tile)
                propagate(vcur, m_earlier);
#pragma unroll
                for (int j = 0; j < K; ++j) vnext[j] = decode(wnext[j]);
                if (tile + 1 < ntiles) propagate(vnext, m_later);
            }
            const uint4 xw = *reinterpret_cast<const uint4 *>(&lds_raw[xch]);
            const int x4[W] = {__builtin_amdgcn_readfirstlane((int)xw.x), __builtin_amdgcn_readfirstlane((int)xw.y),
                               __builtin_amdgcn_readfirstlane((int)xw.z), __builtin_amdgcn_readfirstlane((int)xw.w)};
            base = 0; tot_all = 0;
#pragma unroll
            for (int w2 = 0; w2 < W; ++w2) {
                const int t = x4[w2] >> 1;
                if (w2 < wave) base += t;
                tot_all += t;
            }
            const uint32_t anychg = (uint32_t)(x4[0] | x4[1] | x4[2] | x4[3]) & 1u;
            gr++;
            if (!first && !anychg) break;
            first = false;
            // q of the next round: M - run - (accepted inserts below the lane) + (accepted removals below it).  The scalar enters
            // through the subtraction that seeds the second count (an instruction reads one scalar register: a count seeded
            // with the scalar itself would need a copy into a vector register first)
            uint32_t mrun = M - (uint32_t)(n_start + base);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint64_t im = acci[j], rm = accr[j];
                const uint32_t ci = __builtin_amdgcn_mbcnt_hi((uint32_t)(im >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)im, 0u));
                q[j] = __builtin_amdgcn_mbcnt_hi((uint32_t)(rm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rm, mrun - ci));
                mrun -= (uint32_t)(popc64(im) - popc64(rm));
            }
        }
        // ---- commit ----
        const int dn = wtot; // of the last round: the masks it left are the accepted ones
        int dtr = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint32_t fw = sel64(acci[j] | accr[j], neww[j], word[j]);
            row_st(ops, pbase + (uint32_t)(j * 64), fw);
            const uint64_t trm = sse_ballot((ent[j] >> 30) == SSE_FAST_CLASS_G); // the bond at stake is a transverse-field bond
            dtr += popc64(acci[j] & trm) - popc64(accr[j] & trm);
        }
        ntrans += dtr;
        if (lane == 0 && (dtr | dn)) { // the 64*K slots of a wave's share of a tile lie inside one chunk
            if (dn) atomicAdd(&LDSW(L.o_chn, ch), (uint32_t)dn);
            if (dtr) atomicAdd(&LDSW(L.o_chtr, ch), (uint32_t)dtr);
        }
        n_start += tot_all;
        // chunk of this wave's share of the next tile (TS is a few chunks at the most: CH is a multiple of 256)
        chpos += TS;
        while (chpos >= B.CH) { chpos -= B.CH; ch++; }
    }
    __syncthreads(); // (also: every wave has read the last round's exchange words, which share their LDS with o_tot)
    if (lane == 0) LDSI(L.o_tot, wave) = ntrans;
    __syncthreads();
    int dt = 0;
#pragma unroll
    for (int w2 = 0; w2 < W; ++w2) dt += LDSI(L.o_tot, w2);
    __syncthreads();
    ntrans_io += dt;
    n_io = n_start;
}

// One launch = the diagonal sweep (and, if asked for, the directed loop behind it) of every replica: the first of the two
// launches of a timestep (driver.hip run()), for the geometry above.  PHASE only tags the symbol (see sweep_kernel).
// F64: the rounds of the acceptance rule in f64 (batches whose capacity exceeds SSE_ACCEPT_MAX_DEN, launch_sweep_fast).
template <int K, int PHASE, bool F64>
__global__ __launch_bounds__(256, 4) void sweep_fast_kernel(DevBatch B, SweepArgs A) {
    constexpr int W = 4, NT = W * 64;
    Lds<W> L;
    L.carve(B.N, B.nwords, B.lds_ufcap, B.E, B.has_long);
    const FastLds F = fast_carve<W>(L, B);
    const int tid = threadIdx.x;
    const uint32_t r = blockIdx.x;
#ifdef SSE_WG_TIMELINE // diagnostic builds: when and where every workgroup ran (absolute 100-MHz ticks, HW_ID)
    if (tid == 0 && (B.dbg_flags & 32u)) { B.dbg[(size_t)r * 16 + 0] = __builtin_amdgcn_s_memrealtime(); B.dbg[(size_t)r * 16 + 2] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)); B.dbg[(size_t)r * 16 + 3] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)); }
#endif
    const double beta = A.beta ? A.beta[r] : 0.0;
    for (uint32_t i = tid; i < B.nwords; i += NT) LDSW(L.o_state, i) = B.state[(size_t)r * B.nwords + i];
    for (uint32_t i = tid; i < B.Nb; i += NT) LDSW(F.o_tab, i) = fast_entry(B, i, i < B.E ? B.edges_compact[i] : 0u);
    for (uint32_t i = tid; i < 2 * SSE_MAX_CHUNKS; i += NT) LDSW(L.o_chn, i) = B.chunks[(size_t)r * 2 * SSE_MAX_CHUNKS + i];
    if (tid < 4) {
        const double beta_nb = beta * (double)B.Nb;
        const double w = tid == 0 ? B.wJ : (tid == 1 ? B.gamma : (tid == 2 ? B.wh : 0.0));
        const double num = beta_nb * w; // the general pass' nbond, then scaled by exact powers of two
        if constexpr (F64) *reinterpret_cast<double *>(&lds_raw[F.o_nb + 4u * (uint32_t)tid]) = num * 4294967296.0;
        else *reinterpret_cast<uint64_t *>(&lds_raw[F.o_nb + 4u * (uint32_t)tid]) = sse_accept_insert_const(num);
        *reinterpret_cast<double *>(&lds_raw[F.o_nb + 4u * (uint32_t)tid + 2u]) = num * (1.0 / 4294967296.0);
    }
    __syncthreads();
    int n = (int)B.n[r], ntrans = (int)B.ntrans[r];
    uint32_t M = B.cutoff[r], err = B.err[r], gr = 0, last_out = 0;
    uint64_t epoch = B.epoch[r];
    uint64_t a4 = 0, a5 = 0;
    // pending cluster flips of this replica: applied by the first diagonal pass of the launch (the host passes defer_flips only
    // to launches that start with one)
    const uint32_t fbmask = (A.defer_flips && B.flipb && (A.domask & SSE_DO_DIAG) && !err && B.pend[r]) ? 0xFFu : 0u;
    for (uint64_t step = 0; step < A.nsteps; ++step) {
        if (err) break;
        if (A.domask & SSE_DO_DIAG) {
            const Rng rng = make_rng(B, r, epoch);
            diagonal_fast<K, F64>(B, L, F, r, rng, beta, M, n, ntrans, gr, step == 0 ? fbmask : 0u);
            epoch++;
            a5 += M;
            if (A.domask & SSE_DO_GROW) { // qmc_ising.rs:786, qmc_runner.rs:197
                const uint32_t want = (uint32_t)n + (uint32_t)n / 2u;
                if (want > M) { if (want > B.cap) { err = SSE_ERR_CAPACITY; break; } M = want; }
            }
        }
        if (A.domask & SSE_DO_LOOP) {
            // the directed loop decodes through the compact edge table, which shares its LDS with the (now dead) diagonal tables
            __syncthreads();
            for (uint32_t i = tid; i < B.E; i += NT) LDSW(L.o_edges, i) = B.edges_compact[i];
            __syncthreads();
            const Rng rng = make_rng(B, r, epoch);
            last_out = loop_pass<W, true>(B, L, r, rng, M, n, gr, err);
            epoch++;
            a4 += last_out;
            if (err) break;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < B.nwords; i += NT) B.state[(size_t)r * B.nwords + i] = LDSW(L.o_state, i);
    for (uint32_t i = tid; i < 2 * SSE_MAX_CHUNKS; i += NT) B.chunks[(size_t)r * 2 * SSE_MAX_CHUNKS + i] = LDSW(L.o_chn, i);
    if (tid == 0) {
        B.n[r] = (uint32_t)n; B.ntrans[r] = (uint32_t)ntrans; B.cutoff[r] = M; B.err[r] = err; B.epoch[r] = epoch;
        if (fbmask && A.nsteps) B.pend[r] = 0u; // the diagonal pass rewrote the whole string with the flips applied
        if (A.out_u32) A.out_u32[r] = last_out;
        uint64_t *acc = B.acc + (size_t)B.acc_row[r] * 8;
        acc[4] += a4; acc[5] += a5;
#ifdef SSE_WG_TIMELINE
        if (B.dbg_flags & 32u) B.dbg[(size_t)r * 16 + 1] = __builtin_amdgcn_s_memrealtime();
#endif
    }
}

} // namespace sse
