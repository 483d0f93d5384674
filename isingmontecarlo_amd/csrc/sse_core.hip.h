// sse_core.hip.h — what every gfx950 kernel of the SSE sweep is built from (workgroup-per-replica design): Philox, the LDS carve,
// the per-variable tables, the bond decode and the wave helpers.
//
// One workgroup of W wave64s owns one replica for a whole launch.  The op-string (one u32 per slot,
// include/sse_format.h) streams from HBM in tiles of W*64*K consecutive slots: wave w owns the contiguous
// range [w*64K, (w+1)*64K) of the tile and walks it in K sub-rounds of 64 slots (lane l, sub-round j holds
// slot w*64K + j*64 + l), so K coalesced 256-B loads per wave are in flight per tile.
// Everything the reference keeps in per-node linked lists (src/sse/fast_ops.rs:181-190: prev/next p,
// per-variable prev/next) is recomputed on chip by ORDERED SCANS:
//   * inside a sub-round: wave64 ballot + a serial loop over the (few) writer lanes with v_readlane;
//   * between sub-rounds of a wave: the wave updates its own copy of the per-variable table in LDS;
//   * across the W waves of a tile: W copies of the table; a writer in wave w updates the copies of waves
//     > w before the tile's readers run (one barrier) and the copies of waves < w after they are done
//     (XOR for spin bits, MAX for monotonically increasing segment ids), so copy[w] always equals
//     "the table as of the first slot of wave w in the current tile".
// The live operator count n (the reference reads s.get_n() per slot, qmc_traits/diagonal.rs:126) makes
// the diagonal rule a sequential recurrence n_{p+1} = n_p + d_p(n_p); a tile solves it exactly by
// fixed-point iteration with ballot/popcount prefix sums (unique fixed point = the sequential result).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sse_format.h"
#include "sse_batch.h"

namespace sse {

#ifdef SSE_PHASE_TIMING
#define SSE_STAMP(slot) do { if (threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); B.dbg[(size_t)r * 16 + (slot)] += t_ - dbg_t0; dbg_t0 = t_; } } while (0)
#define SSE_STAMP_INIT unsigned long long dbg_t0 = __builtin_amdgcn_s_memrealtime()
#else
#define SSE_STAMP(slot) do { } while (0)
#define SSE_STAMP_INIT do { } while (0)
#endif

// scalar add that the optimiser may not hoist or merge: the ten round keys are wave-uniform and loop-invariant,
// and hoisted out of the sweep loops they would occupy 20 scalar registers for the whole kernel (they were being
// spilled to vector lanes and read back with v_readlane on every use); one s_add per key and call is cheaper
__device__ __forceinline__ uint32_t philox_bump(uint32_t k, uint32_t w) {
    uint32_t r;
    // (readfirstlane: free when the key already sits in a scalar register; under scalar-register pressure the allocator may hold
    // the uniform key in a vector register, which the "s" constraint alone does not move back)
    const uint32_t ks = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
    asm volatile("s_add_u32 %0, %1, %2" : "=s"(r) : "s"(ks), "s"(w) : "scc");
    return r;
}
__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        // one v_mad_u64_u32 per 32x32->64 product (hi and lo halves together) instead of v_mul_hi + v_mul_lo
        const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0, p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        // three-input xor in one instruction (gfx950 v_bitop3_b32, truth table 0x96)
        uint32_t n0 = __builtin_amdgcn_bitop3_b32(hi1, c1, k0, 0x96), n2 = __builtin_amdgcn_bitop3_b32(hi0, c3, k1, 0x96);
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        if (i < 9) { k0 = philox_bump(k0, 0x9E3779B9u); k1 = philox_bump(k1, 0xBB67AE85u); }
    }
    return make_uint4(c0, c1, c2, c3);
}
// Two blocks that differ in their first counter word only, round by round: one chain of round keys serves both (a call of its
// own would derive them again: 18 s_add, most of them with an s_nop behind for the scalar-write -> vector-read hazard), and the
// other block's vector instructions stand between a key's add and its first reader.  Same outputs as two philox4x32_10 calls.
__device__ __forceinline__ void philox4x32_10_x2(uint32_t c0a, uint32_t c0b, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                 uint4 &oa, uint4 &ob) {
    uint32_t a0 = c0a, a1 = c1, a2 = c2, a3 = c3, b0 = c0b, b1 = c1, b2 = c2, b3 = c3;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t pa0 = (uint64_t)0xD2511F53u * (uint64_t)a0, pa1 = (uint64_t)0xCD9E8D57u * (uint64_t)a2;
        const uint64_t pb0 = (uint64_t)0xD2511F53u * (uint64_t)b0, pb1 = (uint64_t)0xCD9E8D57u * (uint64_t)b2;
        const uint32_t na0 = __builtin_amdgcn_bitop3_b32((uint32_t)(pa1 >> 32), a1, k0, 0x96), na2 = __builtin_amdgcn_bitop3_b32((uint32_t)(pa0 >> 32), a3, k1, 0x96);
        const uint32_t nb0 = __builtin_amdgcn_bitop3_b32((uint32_t)(pb1 >> 32), b1, k0, 0x96), nb2 = __builtin_amdgcn_bitop3_b32((uint32_t)(pb0 >> 32), b3, k1, 0x96);
        a0 = na0; a1 = (uint32_t)pa1; a2 = na2; a3 = (uint32_t)pa0;
        b0 = nb0; b1 = (uint32_t)pb1; b2 = nb2; b3 = (uint32_t)pb0;
        if (i < 9) { k0 = philox_bump(k0, 0x9E3779B9u); k1 = philox_bump(k1, 0xBB67AE85u); }
    }
    oa = make_uint4(a0, a1, a2, a3); ob = make_uint4(b0, b1, b2, b3);
}

struct Rng {
    uint32_t k0, k1, replica, epoch_lo, epoch_hi24;
#ifdef SSE_PHASE_TIMING
    uint32_t dbgx;
#endif
    __device__ __forceinline__ uint4 draw(uint32_t tag, uint32_t index) const {
#ifdef SSE_PHASE_TIMING // diagnostic builds: dbg bit 1 = cheap hash instead of Philox (timing attribution only)
        if (dbgx & 2u) {
            const uint32_t h = (index * 0x9E3779B9u) ^ (epoch_lo * 0x85EBCA6Bu) ^ (replica * 0xC2B2AE35u) ^ tag;
            return make_uint4(h * 0x27D4EB2Fu, h ^ (h >> 15), h * 0x165667B1u, h ^ (h << 13));
        }
#endif
        return philox4x32_10(index, epoch_lo, replica, (tag << 24) | epoch_hi24, k0, k1);
    }
    // draw(tag, ia) and draw(tag, ib) with one derivation of the round keys
    __device__ __forceinline__ void draw2(uint32_t tag, uint32_t ia, uint32_t ib, uint4 &oa, uint4 &ob) const {
#ifdef SSE_PHASE_TIMING
        if (dbgx & 2u) { oa = draw(tag, ia); ob = draw(tag, ib); return; }
#endif
        philox4x32_10_x2(ia, ib, epoch_lo, replica, (tag << 24) | epoch_hi24, k0, k1, oa, ob);
    }
};
__device__ __forceinline__ Rng make_rng(const DevBatch &B, uint32_t r, uint64_t epoch) {
    Rng g;
    g.k0 = B.seed_lo; g.k1 = B.seed_hi; g.replica = B.rid ? B.rid[r] : B.replica_offset + r;
    g.epoch_lo = (uint32_t)epoch; g.epoch_hi24 = (uint32_t)(epoch >> 32) & 0xFFFFFFu;
#ifdef SSE_PHASE_TIMING
    g.dbgx = B.dbg_flags;
#endif
    return g;
}
__device__ __forceinline__ double u01(uint32_t x) { return (double)x * (1.0 / 4294967296.0); }

// decoded bond: variables, kind|pref<<2, weight when satisfied
struct Bd {
    uint32_t a, c, kp;
    double w;
};
__device__ __forceinline__ uint32_t bd_kind(const Bd &b) { return b.kp & SSE_BOND_KIND_MASK; }

// matrix element of the shifted bond operator (reference: src/sse/qmc_ising.rs:863-888); straight-line code
__device__ __forceinline__ double bond_weight(const Bd &b, uint32_t in, uint32_t out) {
    const uint32_t kind = b.kp & SSE_BOND_KIND_MASK, pref = (b.kp >> 2) & 1u;
    const uint32_t aligned = ((in ^ (in >> 1)) & 1u) ^ 1u;
    const uint32_t sat = (kind == SSE_BOND_TWO_SITE) ? (uint32_t)(aligned == pref) : (uint32_t)((in & 1u) == pref);
    const bool ok = (kind == SSE_BOND_TRANSVERSE) | ((in == out) & (sat != 0u));
    return ok ? b.w : 0.0;
}

// matrix element of bond b for any model: Interaction::at (qmc_runner.rs:573-612) when the batch carries weight
// matrices, the closed Ising form otherwise
__device__ __forceinline__ double op_weight(const DevBatch &B, uint32_t b, const Bd &d, uint32_t in, uint32_t out) {
    if (B.mats) return B.mats[(size_t)b * 16u + (in | (out << 2))];
    return bond_weight(d, in, out);
}

// ---------------------------------------------------------------------------------------------
// LDS carve (dynamic shared memory).  All sizes in u32 words.
// Every LDS access below indexes this one array directly so that the compiler always emits ds_*
// instructions (pointers held in structs decay to the generic address space and become flat_* ops,
// which are slower and make s_waitcnt on LDS data also wait for the in-flight HBM prefetches).
extern __shared__ __align__(16) uint32_t lds_raw[];
#define LDSW(off, i) lds_raw[(off) + (i)]
#define LDSI(off, i) (reinterpret_cast<int &>(lds_raw[(off) + (i)]))
#define LDSH(off, i) (reinterpret_cast<uint16_t *>(lds_raw)[2u * (off) + (i)]) // 16-bit element i of the array at word offset off
#define LDSB(off, i) (reinterpret_cast<uint8_t *>(lds_raw)[4u * (off) + (i)])  // 8-bit element i of the array at word offset off
// Tables that OTHER lanes of the same wave write between two reads of one lane need a wavefront-scope fence
// between the writes and the re-reads (the C++ memory model would otherwise let the compiler reuse the first
// value).  It emits no instruction: LDS operations of one wave execute in order.
// Diagnostic builds (-DSSE_PHASE_TIMING) can switch parts of a pass off at run time to attribute time; results are
// then wrong by construction.  Normal builds compile the switches away.
#ifdef SSE_PHASE_TIMING
#define SSE_DBG(B, bit) (((B).dbg_flags & (bit)) != 0u)
#else
#define SSE_DBG(B, bit) false
#endif
#define SSE_WAVE_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")

template <int W>
struct Lds {           // word offsets into lds_raw
    uint32_t o_state;  // [nwords]      p=0 spin state
    uint32_t o_touch;  // [nwords]      variables touched by any op
    uint32_t o_touch8; // [N] u8        the same as bytes while the cluster scan runs (plain byte stores instead of atomics)
    uint32_t o_tot;    // [2][W]        per-wave totals (double buffered by round parity)
    uint32_t o_chg;    // [2][W]
    uint32_t o_misc;   // [16]
    uint32_t o_chn;    // [SSE_MAX_CHUNKS] occupied slots per chunk
    uint32_t o_chtr;   // [SSE_MAX_CHUNKS] transverse ops per chunk
    uint32_t o_edges;  // [E]           compact edge table (CL mode only)
    uint32_t o_signs;  // [pm_words]    this replica's coupling signs (+-J decode only)
    uint32_t o_cur;    // [W][N] u16    per wave: rank+1 (within the wave's range) of the latest cut on each variable
    uint32_t o_cl;     // [W][N] u8     per wave: 1 + rank inside the current sub-round of a cut on the variable (0 = none)
    uint32_t o_frozen; // [ufwords]     bit per id: segment holds a longitudinal op
    uint32_t o_froot;  // [ufwords]     bit per id: root is frozen
    uint32_t o_parent; // [ufcap] u16 (the LDS union-find is only used when every id fits 16 bits)
    uint32_t end;      // first word behind the parent table: the dynamic LDS of a launch of this layout
    uint32_t end_diag; // first word behind what a diagonal-pass launch uses (the regions up to o_cur, o_cur as [W][N] u8 spin bytes)
    // diag_only: the launch runs the diagonal pass (+ directed loop) alone and its per-wave spin BYTES are the only per-variable
    // table (large models whose cluster tables live in HBM can still keep these in LDS)
    __host__ __device__ __forceinline__ void carve(uint32_t N, uint32_t nwords, uint32_t ufcap, uint32_t ledges, uint32_t has_long, bool tg = false,
                                                   uint32_t pm_words = 0, bool diag_only = false) {
        uint32_t base = 0;
        o_state = base; base += nwords;
        o_touch = base; base += nwords;
        if (tg) N = 0; // MODE 2: the per-variable tables live in HBM (Tab<true>), only the bit arrays stay in LDS
        o_touch8 = base; base += diag_only ? 0u : (N + 3) / 4;
        o_tot = base; base += 2 * W;
        o_chg = base; base += 2 * W;
        o_misc = base; base += 16;
        o_chn = base; base += SSE_MAX_CHUNKS;
        o_chtr = base; base += SSE_MAX_CHUNKS;
        o_edges = base; base += ledges;
        o_signs = base; base += pm_words;
        o_cur = base; base += diag_only ? (W * N + 3) / 4 : (W * N + 1) / 2;
        end_diag = o_cur + (W * N + 3) / 4;
        o_cl = base; base += diag_only ? 0u : (W * N + 3) / 4;
        o_frozen = base; base += has_long ? (ufcap + 31) / 32 : 0u;
        o_froot = base; base += has_long ? (ufcap + 31) / 32 : 0u;
        o_parent = base;
        end = base + (ufcap + 1) / 2;
    }
};
// Per-variable tables of the ordered scans (spin bytes of the diagonal pass, cut ranks / cut markers / touched bytes of the
// cluster scan).  TG = false: LDS (ds_* instructions, `reg` = word offset into lds_raw).  TG = true: a per-replica scratch in
// HBM, in practice served by L2 / Infinity Cache (`reg` = byte offset into g) — for models whose tables exceed the 160 KB of
// LDS (N >~ 10^4 variables, BASELINE configs[4] at 32^3).  A wave's own table is only touched by that wave between two
// barriers, and global accesses of one wave are ordered at wavefront scope without waits, so the code is the same in both
// modes; other waves' tables are only changed by atomics separated from their owners' accesses by a workgroup barrier.
template <bool TG>
struct Tab {
    uint8_t *g;
    uint32_t cur, cl, touch8;
    __device__ __forceinline__ uint32_t ld8(uint32_t reg, uint32_t i) const { if constexpr (TG) return g[reg + i]; else return LDSB(reg, i); }
    __device__ __forceinline__ void st8(uint32_t reg, uint32_t i, uint32_t v) const { if constexpr (TG) g[reg + i] = (uint8_t)v; else LDSB(reg, i) = (uint8_t)v; }
    __device__ __forceinline__ uint32_t ld16(uint32_t reg, uint32_t i) const { if constexpr (TG) return reinterpret_cast<const uint16_t *>(g + reg)[i]; else return LDSH(reg, i); }
    __device__ __forceinline__ void st16(uint32_t reg, uint32_t i, uint32_t v) const { if constexpr (TG) reinterpret_cast<uint16_t *>(g + reg)[i] = (uint16_t)v; else LDSH(reg, i) = (uint16_t)v; }
    __device__ __forceinline__ uint32_t ld32(uint32_t reg, uint32_t i) const { if constexpr (TG) return reinterpret_cast<const uint32_t *>(g + reg)[i]; else return LDSW(reg, i); }
    __device__ __forceinline__ void st32(uint32_t reg, uint32_t i, uint32_t v) const { if constexpr (TG) reinterpret_cast<uint32_t *>(g + reg)[i] = v; else LDSW(reg, i) = v; }
    // MODE 2 keeps the scan tables of a (wave, variable) pair in ONE 4-byte record {u16 rank, u8 marker, u8 touched}: a leg's
    // lookups and a cut's stores then hit one 64-B sector of HBM instead of three (that path is bound by random-sector traffic)
    __device__ __forceinline__ uint32_t rec_ld(uint32_t i) const { return reinterpret_cast<const uint32_t *>(g)[i]; }
    __device__ __forceinline__ void rec_st(uint32_t i, uint32_t v) const { reinterpret_cast<uint32_t *>(g)[i] = v; }
    __device__ __forceinline__ void rec_rank_st(uint32_t i, uint32_t v) const { reinterpret_cast<uint16_t *>(g)[2u * i] = (uint16_t)v; }
    __device__ __forceinline__ void rec_mark_st(uint32_t i, uint32_t v) const { g[4u * i + 2u] = (uint8_t)v; }
    __device__ __forceinline__ void rec_touch_st(uint32_t i) const { g[4u * i + 3u] = (uint8_t)1u; }
    __device__ __forceinline__ void xor32(uint32_t reg, uint32_t i, uint32_t bits) const {
        if constexpr (TG) __hip_atomic_fetch_xor(reinterpret_cast<uint32_t *>(g + reg) + i, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else atomicXor(&LDSW(reg, i), bits);
    }
};
template <bool TG, int W>
__device__ __forceinline__ Tab<TG> make_tab(const DevBatch &B, const Lds<W> &L, uint32_t r) {
    Tab<TG> T;
    if constexpr (TG) {
        T.g = B.tbl + (size_t)r * B.tbl_stride;
        T.cur = 0u; T.cl = (uint32_t)W * B.N * 2u; T.touch8 = (uint32_t)W * B.N * 4u; // byte offsets (N is a multiple of 4 in this mode); the cluster scan uses the records (rec_*) at offset 0
    } else {
        T.g = nullptr;
        T.cur = L.o_cur; T.cl = L.o_cl; T.touch8 = L.o_touch8;
    }
    return T;
}

enum { MISC_NCLUST = 0, MISC_ANYFROZEN = 1, MISC_LOOP_A = 2, MISC_LOOP_B = 3, MISC_LOOP_C = 4, MISC_LOOP_D = 5 };

// The 16-byte bond record of bond b: loaded from this replica's table (general decode) or, for the +-J decode, put together from
// the shared compact edge table, the replica's sign bits in LDS and the uniform weights — everything downstream is the same code.
template <bool PM, int W>
__device__ __forceinline__ uint4 bond_rec(const DevBatch &B, const Lds<W> &L, uint32_t b) {
    if constexpr (PM) {
        const bool two = b < B.E;
        const uint32_t eb = two ? b : 0u;
        const uint32_t e = B.edges_compact[eb];
        const uint32_t sgn = (LDSW(L.o_signs, eb >> 5) >> (eb & 31u)) & 1u;
        const uint32_t s1 = b - B.E;
        const bool tr = s1 < B.N;
        const uint32_t a = two ? (e & SSE_CE_VAR_MASK) : (tr ? s1 : s1 - B.N);
        const uint32_t kp = two ? (SSE_BOND_TWO_SITE | (sgn << 2)) : (tr ? SSE_BOND_TRANSVERSE : (SSE_BOND_LONGITUDINAL | (B.hpos << 2)));
        const double w = two ? B.wJ : (tr ? B.gamma : B.wh);
        return make_uint4(a | (kp << SSE_INFO_SHIFT), two ? ((e >> 15) & SSE_CE_VAR_MASK) : SSE_NO_VAR, (uint32_t)__double2loint(w), (uint32_t)__double2hiint(w));
    } else {
        return *reinterpret_cast<const uint4 *>(B.bonds + b);
    }
}

template <bool CL, int W, bool PM = false>
__device__ __forceinline__ Bd decode_bond(const DevBatch &B, const Lds<W> &L, uint32_t b) {
    Bd d;
    if constexpr (CL) {
        // straight-line: one LDS read with a safe index, then selects
        const bool two = b < B.E;
        const uint32_t e = LDSW(L.o_edges, two ? b : 0u);
        const uint32_t s1 = b - B.E;
        const bool tr = s1 < B.N;
        d.a = two ? (e & SSE_CE_VAR_MASK) : (tr ? s1 : s1 - B.N);
        d.c = two ? ((e >> 15) & SSE_CE_VAR_MASK) : SSE_NO_VAR;
        d.kp = two ? (SSE_BOND_TWO_SITE | (((e >> 30) & 1u) << 2))
                   : (tr ? SSE_BOND_TRANSVERSE : (SSE_BOND_LONGITUDINAL | (B.hpos << 2)));
        // CL mode is only selected for uniform |J|: the three weights are scalars.  Select on their halves held in
        // scalar registers; written as a select of the doubles the compiler turns it into a per-lane LOAD from the
        // kernel-argument segment, whose s_waitcnt then also waits for the op-word prefetch (vmcnt is in order).
        const int jlo = __builtin_amdgcn_readfirstlane(__double2loint(B.wJ)), jhi = __builtin_amdgcn_readfirstlane(__double2hiint(B.wJ));
        const int glo = __builtin_amdgcn_readfirstlane(__double2loint(B.gamma)), ghi = __builtin_amdgcn_readfirstlane(__double2hiint(B.gamma));
        const int hlo = __builtin_amdgcn_readfirstlane(__double2loint(B.wh)), hhi = __builtin_amdgcn_readfirstlane(__double2hiint(B.wh));
        d.w = __hiloint2double(two ? jhi : (tr ? ghi : hhi), two ? jlo : (tr ? glo : hlo));
    } else {
        const uint4 q = bond_rec<PM, W>(B, L, b);
        d.a = q.x & SSE_VAR_MASK; d.c = q.y; d.kp = q.x >> SSE_INFO_SHIFT;
        d.w = __hiloint2double((int)q.w, (int)q.z);
    }
    return d;
}

// wave priority for the issue arbiter (s_setprio takes an immediate): x mod 4, wave-uniform
#ifndef SSE_ROTATE_PRIO
#define SSE_ROTATE_PRIO 2u // tiles of the trimmed diagonal kernel between two priority changes (power of two)
#endif
#ifndef SSE_GEN_ROTATE
#define SSE_GEN_ROTATE 2u  // the same for the tile loops of the general kernels
#endif
__device__ __forceinline__ void sse_set_prio(uint32_t x) {
    switch (x & 3u) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// wave64 ballot straight from the i1 condition (HIP's __ballot(int) goes through a 0/1 integer: v_cndmask + v_cmp_ne)
__device__ __forceinline__ uint64_t sse_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool sse_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
__device__ __forceinline__ uint64_t lanemask_lt(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ int popc64(uint64_t x) { return __popcll(x); }

// v_cndmask on a wave mask held in scalar registers: mask bit of the lane set ? a : b
__device__ __forceinline__ uint32_t sel64(uint64_t mask, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(mask));
    return r;
}

// flip bit 0 of 8-bit element e of the table at word offset off (other waves' tables: 32-bit atomic on the word)
__device__ __forceinline__ void spin_table_flip(uint32_t off, uint32_t e) { atomicXor(&LDSW(off, e >> 2), 1u << ((e & 3u) * 8u)); }

// A wave-uniform double pinned into vector registers: selects between such values then cost two v_cndmask each,
// instead of copying scalar halves into vector registers at every use.
__device__ __forceinline__ double vgpr_copy(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x), vlo, vhi;
    asm volatile("v_mov_b32 %0, %1" : "=v"(vlo) : "s"(lo));
    asm volatile("v_mov_b32 %0, %1" : "=v"(vhi) : "s"(hi));
    return __hiloint2double(vhi, vlo);
}

// Row accesses as (uniform base pointer) + (32-bit byte offset): the offset is computed in 32 bits (rows are far below
// 2^30 words), which lets the compiler use the scalar-base + vector-offset addressing mode instead of 64-bit vector
// address arithmetic per access.
__device__ __forceinline__ uint32_t row_ld(const uint32_t *row, uint32_t idx) {
    return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(row) + (size_t)(idx * 4u));
}
__device__ __forceinline__ void row_st(uint32_t *row, uint32_t idx, uint32_t v) {
    *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(row) + (size_t)(idx * 4u)) = v;
}

__device__ __forceinline__ uint32_t vgpr_copy_u32(uint32_t x) {
    uint32_t v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

// slot index of (tile, wave, sub-round j, lane)
template <int W, int K>
__device__ __forceinline__ uint32_t slot_of(uint32_t tile, int wave, int j, int lane) {
    return tile * (uint32_t)(W * 64 * K) + (uint32_t)(wave * 64 * K + j * 64 + lane);
}

} // namespace sse
