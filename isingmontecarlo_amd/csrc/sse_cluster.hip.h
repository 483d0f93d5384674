// sse_cluster.hip.h — the cluster update of the headline geometry as its own kernel, written for LDS traffic and
// instruction count (round 3).
//
// Same algorithm, same ids, same Philox counters and bit-identical results as sse::cluster_pass<16, K, CL = true, UF_GLOBAL = false>
// (sse_cluster_pass.hip.h, which stays the general implementation: every other geometry, HBM union-find, HBM tables, generic
// interactions).  Reference: ClusterUpdater::flip_each_cluster_rng (qmc_traits/cluster.rs:36-172) + expand_whole_cluster
// (:193-271), the longitudinal weight function of qmc_ising.rs:759-775, then the free-spin step and the sampling of
// qmc_ising.rs:780-786 / qmc_stepper.rs:149-161.
//
// Why a second implementation.  Measured on MI355X (profiles/r02_*), the general off-diagonal kernel spends 179 vector + 112
// scalar + 35 LDS instructions per 64-slot row in its build scan, holds four cluster_pass variants in one symbol (128 VGPRs,
// 640 scalar spills, 72 B scratch) and keeps 8 B of cached ids per slot in HBM.  This kernel holds ONE path:
//   * one packed 32-bit LDS entry per bond, index = op word >> 4 (entry 0 = empty slot): both variables, "two-site", "cut"
//     (transverse-field op: the sign bit, so the cut mask is one signed compare), "longitudinal".  Empty slots and one-variable
//     bonds name the same variable twice / a dummy variable N, so that nothing below is predicated on the kind of the slot;
//   * per wave ONE packed 32-bit entry per variable: current segment id (16) | in-row cut marker (8) | touched (1).  A leg's
//     lookup is one 32-bit read (id + marker + flag): two LDS round trips per row instead of the four sub-dword reads + two
//     touched-byte stores of the general scan (the scan is bound by LDS bank conflicts of random full-wave accesses once the
//     instruction count is down).  Without a longitudinal field the flag needs no store of its own (see the build scan);
//   * the table holds the segment ID itself (placeholder ids are written at initialisation), not a rank to be converted;
//   * every slot keeps ONE 16-bit id in HBM (B.segs, two rows per dword): a two-site op's legs are in one cluster once its
//     union is done, a cut's own id is its dense number, recomputed by the apply pass from the row's cut mask.  HBM traffic of the
//     update: 4 + 2 (build) + 4 + 2 + 4 (apply) = 16 B per slot against 20 B before and 12 B algorithmic;
//   * the apply pass runs over the same wave -> range partition as the build: a wave only re-reads ids it stored itself.
// Replicas whose ids do not fit the LDS union-find of this launch (or that hold no op / no cut) are left untouched and flagged
// in B.aux; the host follows up with the general kernel restricted to flagged replicas (driver.hip run()).
#pragma once
#include "sse_cluster_pass.hip.h" // the union-find and free_spin_pass

namespace sse {

#define SSE_CLW 16                  // waves per replica
#define SSE_CL_MAX_VARS 4095u       // variable fields of a bond entry are 13 bits, N itself names the dummy variable
// packed bond entry: a [0,13) | c [13,26) (= a for one-variable bonds, both = N for the empty slot) | two-site (bit 28) |
// longitudinal (bit 29) | cut (bit 31)
#define SSE_CLE_TWO (1u << 28)
#define SSE_CLE_LONG (1u << 29)
#define SSE_CLE_CUT (1u << 31)
#define SSE_CL_TOUCHED (1u << 24)

// LDS accesses of the hot loops by ABSOLUTE LDS byte address held in a 32-bit register (bases below include the address of
// lds_raw): written as pointer arithmetic on lds_raw every access costs an extra v_add of the symbol's (link-time) address
typedef __attribute__((address_space(3))) uint32_t sse_lds_u32;
typedef __attribute__((address_space(3))) uint16_t sse_lds_u16;
typedef __attribute__((address_space(3))) uint8_t sse_lds_u8;
#define LDS32B(a) (*(sse_lds_u32 *)(uintptr_t)(a))
#define LDS16B(a) (*(sse_lds_u16 *)(uintptr_t)(a))
#define LDS8B(a) (*(sse_lds_u8 *)(uintptr_t)(a))
__device__ __forceinline__ void lds_cas32(uint32_t addr, uint32_t expect, uint32_t val) { // ds_cmpst_b32, result unused
    (void)__hip_atomic_compare_exchange_strong((sse_lds_u32 *)(uintptr_t)addr, &expect, val, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// A 16-bit LDS load used as a 32-bit value: ds_read_u16 clears the upper half of its register.  The empty asm hides the origin of
// the value, so the compiler neither compares in 16 bits nor re-masks a second, zero-extended copy of it.
__device__ __forceinline__ uint32_t lds_ld16(uint32_t addr) {
    uint32_t v = LDS16B(addr);
    asm("" : "+v"(v));
    return v;
}
// low half of a word as a value of its own (an instruction of its own: written as a mask, the compiler folds it into the shift of
// the address that follows and spends an instruction more)
__device__ __forceinline__ uint32_t cl_low16(uint32_t x) {
    uint32_t r;
    asm("v_and_b32 %0, 0xffff, %1" : "=v"(r) : "v"(x));
    return r;
}
// The two places of the scan that need the clean 16-bit id of a leg word.  Without a longitudinal field (HL = false) a leg word may
// carry the touched flag above its id (see the build scan); each takes the low half inside the one instruction it costs anyway:
// two ids of the apply pass in one dword (v_perm_b32 in place of v_lshl_or_b32; sel = SSE_CL_PACK_SEL, which the caller keeps in a
// vector register: as a scalar it cost the kernel two more scalar spills) ...
#define SSE_CL_PACK_SEL 0x05040100u // bytes 1:0 of the second operand below bytes 1:0 of the first
template <bool HL>
__device__ __forceinline__ uint32_t cl_pack_ids(uint32_t lo, uint32_t hi, uint32_t sel) {
    if constexpr (HL) return lo | (hi << 16);
    else return __builtin_amdgcn_perm(hi, lo, sel);
}
// ... and the LDS address of the id's parent-table entry (v_mad_u32_u16 in place of v_lshl_add_u32)
template <bool HL>
__device__ __forceinline__ uint32_t cl_par_addr(uint32_t par_b, uint32_t leg) {
    if constexpr (HL) return par_b + 2u * leg;
    else {
        uint32_t r;
        asm("v_mad_u32_u16 %0, %1, 2, %2" : "=v"(r) : "v"(leg), "s"(par_b));
        return r;
    }
}
// word of o_misc that the lanes of a predicated LDS store with nothing to store are pointed at (sse_fast.hip.h, "Predicated LDS
// stores and atomics are written branch-free"): this kernel uses words 0-2 of the 16, nothing ever reads this one
#define SSE_CL_MISC_DUMMY 12u
// Parked unions of the build scan (see there): every wave owns SSE_CL_QCAP queue words and, behind them, the word that counts
// them and the count of the full queues it has served
#define SSE_CL_QCAP 64u
#define SSE_CL_QWAVE (SSE_CL_QCAP + 2u)
#define SSE_CL_QUEUE_WORDS ((uint32_t)SSE_CLW * SSE_CL_QWAVE)

struct ClLds { // word offsets into lds_raw
    uint32_t o_tab;    // [Nb + 1]   packed bond entries, at word 0 (the index is the op word >> 4)
    uint32_t o_state;  // [nwords]
    uint32_t o_touch;  // [nwords]   bit v: some op acts on variable v
    uint32_t o_misc;   // [16]
    uint32_t o_chn;    // [SSE_MAX_CHUNKS]
    uint32_t o_chtr;   // [SSE_MAX_CHUNKS]
    uint32_t o_queue;  // [16][SSE_CL_QWAVE] per wave: parked unions of the build scan (two u16 ids per word), their count, full queues served
    uint32_t o_ent;    // [16][N + 1] per (wave, variable): id | marker << 16 | touched << 24; after the joins: root list + flip bits
    uint32_t o_frozen, o_froot; // [ufwords] (h != 0)
    uint32_t o_parent; // [ufcap] u16
    uint32_t end;      // first word behind the parent table: the launch's dynamic LDS
    __host__ __device__ __forceinline__ void carve(uint32_t N, uint32_t nwords, uint32_t Nb, uint32_t ufcap, bool has_long) {
        uint32_t base = 0;
        o_tab = base; base += Nb + 1u;
        o_state = base; base += nwords;
        o_touch = base; base += nwords;
        o_misc = base; base += 16u;
        o_chn = base; base += SSE_MAX_CHUNKS;
        o_chtr = base; base += SSE_MAX_CHUNKS;
        o_queue = base; base += SSE_CL_QUEUE_WORDS;
        o_ent = base; base += (uint32_t)SSE_CLW * (N + 1u);
        o_frozen = base; base += has_long ? (ufcap + 31u) / 32u : 0u;
        o_froot = base; base += has_long ? (ufcap + 31u) / 32u : 0u;
        o_parent = base;
        end = base + (ufcap + 1u) / 2u;
    }
};
// Is a replica with N variables and S ids (16 N + C: initial segments and placeholders, cuts) this kernel's case?  The 16-bit
// parent table must hold S + 1 entries (id S is the null id of empty slots) below the 16-bit limit, and after the joins the S flip
// bits reuse the per-wave tables o_ent (16 (N + 1) words): with few variables and many cuts they would run into the tables behind.
// The one test of the kernel (replicas outside it are flagged for the general kernel), of plan_lean() and of the host audit.
static inline __host__ __device__ bool cl_ids_fit(uint32_t N, uint32_t S, uint32_t ufcap) {
    return S < ufcap && S < 65535u && ((size_t)S + 31) / 32 <= (size_t)SSE_CLW * (N + 1);
}
// u16 entries of the root list behind the flip bits in the dead per-wave tables (0 when the bits fill them)
static inline __host__ __device__ uint32_t cl_list_cap(uint32_t N, uint32_t S) {
    const size_t tab = (size_t)SSE_CLW * (N + 1), bits = ((size_t)S + 31) / 32;
    return bits < tab ? (uint32_t)(2 * (tab - bits)) : 0u;
}

// lane `l` (a constant) of v := the wave-uniform x; the other lanes keep their value
// This clang has no builtin for it, so the LLVM intrinsic is declared by name.  Not inline assembly: the compiler must see the
// instruction, because on gfx950 a VALU read of a scalar register needs two wait states behind the VALU write of it, and the
// v_cmp of a ballot can stand right in front of the v_writelane that reads its mask (the compiler then inserts the s_nop or
// schedules around it).  The lane select is a constant once the row loop is unrolled: an immediate of the instruction.
extern "C" __device__ int sse_cl_llvm_writelane(int, int, int) __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ uint32_t cl_writelane(uint32_t v, uint32_t x, int l) { return (uint32_t)sse_cl_llvm_writelane((int)x, l, (int)v); }

// union on trees that only the calling wave touches (see uf_union_wave); returns the surviving root.  Both walks to the roots
// advance together (two independent LDS reads per step instead of two walks one after the other), and the two start nodes are
// re-pointed at their roots (they are not roots themselves when they differ from them)
__device__ __forceinline__ uint32_t cl_union_wave(const UFA<false> &uf, uint32_t a, uint32_t b) {
    for (;;) {
        uint32_t xa = a, xb = b, pa = uf.get(a), pb = uf.get(b);
        while ((pa != xa) | (pb != xb)) { xa = pa; xb = pb; pa = uf.get(xa); pb = uf.get(xb); } // (a root is its own parent: it stays put)
        if (a != xa) uf.set(a, xa);
        if (b != xb) uf.set(b, xb);
        if (xa == xb) return xa;
        const uint32_t lo = min(xa, xb), hi = max(xa, xb);
        uf.set(hi, lo);
        SSE_WAVE_FENCE();
        if (uf.get(hi) == lo) return lo;
        a = xa; b = xb;
    }
}

// Behind the scan (see "join the ranges" and "flatten" in the kernel)
#ifndef SSE_CL_JOIN_ROTATE
#define SSE_CL_JOIN_ROTATE 1 // wave wv joins the range boundaries in the order (k + wv) & 15 (0: every wave in the order 0 .. 15)
#endif
#ifndef SSE_CL_FLATTEN_BATCH
#define SSE_CL_FLATTEN_BATCH 4 // ids a thread of the flatten pass walks to their roots together
#endif
// link the trees of two DIFFERENT roots as the caller's finds left them, on trees that other waves link at the same time: the
// compare-and-swap loop of uf_union, entered behind its first pair of finds.  att / lost count the attempts and the lost ones
// (diagnostic builds read them, elsewhere they are dead)
__device__ __forceinline__ void cl_link_roots(const UFA<false> &uf, uint32_t a, uint32_t b, uint32_t &att, uint32_t &lost) {
    for (;;) {
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        att++;
        if (uf.cas(b, b, a) == b) return;
        lost++;
        a = uf_find(uf, a);
        b = uf_find(uf, b);
        if (a == b) return;
    }
}

// One launch = the cluster update (+ free spins + sampling) of every replica: the second launch of a split timestep.
// PHASE only tags the symbol (see sweep_kernel).
#ifndef SSE_CL_FIND_LEVELS
#define SSE_CL_FIND_LEVELS 4 // hops of the straight-line find in front of a union
#endif
template <int K, bool HAS_LONG, int PHASE>
__global__ __launch_bounds__(SSE_CLW * 64, 4) void cluster_kernel(DevBatch B, SweepArgs A) {
    constexpr int W = SSE_CLW, NT = W * 64;
    constexpr uint32_t TS = 64u * K;
    static_assert(K == 2 || K == 4, "ids are stored two rows per dword");
    ClLds L;
    L.carve(B.N, B.nwords, B.Nb, B.lds_ufcap, HAS_LONG);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t r = blockIdx.x;
    const uint32_t N = B.N, nwords = B.nwords;
    const int n = (int)B.n[r];
    const uint32_t C = B.ntrans[r], M = B.cutoff[r], err = B.err[r];
    if (err) return;                                  // sticky error: the general kernel would not touch the replica either
    const uint32_t S = N + C + (uint32_t)(W - 1) * N; // ids: initial segments, cuts, range-boundary placeholders
    if (n == 0 || C == 0u || !cl_ids_fit(N, S, B.lds_ufcap)) { // not this kernel's case: the general one follows up (id S itself is the
                                                               // null id of empty slots: a table entry of its own, its flip bit stays 0)
        if (tid == 0) B.aux[r] = 1u;
        return;
    }
    UFA<false> uf;
    uf.gparent = nullptr; uf.gfrozen = nullptr; uf.gfroot = nullptr;
    uf.o_parent = L.o_parent; uf.o_frozen = L.o_frozen; uf.o_froot = L.o_froot;
    uint64_t epoch = B.epoch[r];
    uint32_t *ops = B.ops + (size_t)r * B.stride;
    uint32_t *ids = B.segs + (size_t)r * B.stride;    // 16-bit ids, rows 2k and 2k+1 share dword (p >> 1 rounded to the pair) + lane
    // deferred flips (A.defer_flips): the row masks live behind the ids (second half of the scratch row: 16 B per 64 slots)
    const bool DEFER = A.defer_flips != 0u && B.flipb != nullptr;
    uint4 *msk = reinterpret_cast<uint4 *>(ids + B.stride / 2u);

    SSE_STAMP_INIT;
    // ---- initialisation ----
    for (uint32_t i = tid; i < nwords; i += NT) { LDSW(L.o_state, i) = B.state[(size_t)r * nwords + i]; LDSW(L.o_touch, i) = 0u; }
    // bond entries, one loop per kind of bond (bonds [0, E): two-site, [E, E + N): transverse field, then the longitudinal ones): entry 1 + b of bond b, entry 0 = the empty slot
    if (tid == 0) LDSW(L.o_tab, 0u) = N | (N << 13);
    for (uint32_t i = tid; i < B.E; i += NT) {
        const uint32_t ce = B.edges_compact[i];
        LDSW(L.o_tab, 1u + i) = (ce & SSE_CE_VAR_MASK) | (((ce >> 15) & SSE_CE_VAR_MASK) << 13) | SSE_CLE_TWO;
    }
    for (uint32_t v = tid; v < N; v += NT) {
        const uint32_t vv = v | (v << 13);
        LDSW(L.o_tab, 1u + B.E + v) = vv | SSE_CLE_CUT;
        if (1u + B.E + N + v <= B.Nb) LDSW(L.o_tab, 1u + B.E + N + v) = vv | SSE_CLE_LONG;
    }
    for (uint32_t i = tid; i < 2 * SSE_MAX_CHUNKS; i += NT) LDSW(L.o_chn, i) = B.chunks[(size_t)r * 2 * SSE_MAX_CHUNKS + i];
    if (tid == 0) { LDSW(L.o_misc, MISC_NCLUST) = 0u; LDSW(L.o_misc, MISC_ANYFROZEN) = 0u; LDSW(L.o_misc, MISC_LOOP_A) = 0u; }
    // per-wave tables: the segment a variable is in when the wave's range begins = the placeholder id of (wave, variable)
    // (wave w fills table w: the variable is the running index, the placeholder base is a scalar)
    {
        const uint32_t tb = L.o_ent + (uint32_t)wave * (N + 1u), id0 = wave == 0 ? 0u : N + C + (uint32_t)(wave - 1) * N;
        for (uint32_t v = (uint32_t)lane; v < N; v += 64u) LDSW(tb, v) = id0 + v;
        if (lane == 0) LDSW(tb, N) = S; // (the dummy variable of empty slots carries the null id S)
        if (lane < 2) LDSW(L.o_queue, (uint32_t)wave * SSE_CL_QWAVE + SSE_CL_QCAP + (uint32_t)lane) = 0u; // no union parked, no queue served
    }
    for (uint32_t i = tid; i < S / 2u + 1u; i += NT) LDSW(L.o_parent, i) = (2u * i) | ((2u * i + 1u) << 16); // parent[i] = i for i <= S
    if constexpr (HAS_LONG) for (uint32_t i = tid; i < (S + 31u) / 32u; i += NT) uf.bits_clear(i);
    __syncthreads();

    // ---- this wave's range of chunks, the id of its first cut ----
    const uint32_t used = (M + B.CH - 1u) / B.CH;
    const uint32_t q = (used + W - 1u) / W;
    const uint32_t c0 = min((uint32_t)wave * q, used), c1 = min(c0 + q, used);
    uint32_t cutbase = 0;
    for (uint32_t c = lane; c < c0; c += 64) cutbase += LDSW(L.o_chtr, c);
    for (int off = 32; off > 0; off >>= 1) cutbase += __shfl_xor(cutbase, off);
    cutbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)cutbase);
    const uint32_t pbeg = c0 * B.CH, pend = min(c1 * B.CH, M); // whole tiles except at the end of the string, where the row holds zeros
    const uint32_t lds0 = (uint32_t)(uintptr_t)(sse_lds_u32 *)lds_raw; // LDS address of the dynamic region
    const uint32_t ent_b = lds0 + 4u * (L.o_ent + (uint32_t)wave * (N + 1u)); // LDS address of this wave's table
    const uint32_t par_b = lds0 + 4u * L.o_parent;
    // Predicated LDS stores of the scan and of the union block are written branch-free (see SSE_CL_MISC_DUMMY): an address select
    // on the mask the code has anyway, instead of an exec save / restore around every store
    const uint32_t dummy_b = vgpr_copy_u32(lds0 + 4u * (L.o_misc + SSE_CL_MISC_DUMMY));
    const uint32_t que_b = lds0 + 4u * (L.o_queue + (uint32_t)wave * SSE_CL_QWAVE), qcnt_b = que_b + 4u * SSE_CL_QCAP; // this wave's queue, its count (the count of full queues served: the word behind)

    SSE_STAMP(0);
    // ---- build: label every leg, union through the two-site ops (cluster.rs:193-271) ----
    // The id a table entry holds is a REPRESENTATIVE of the segment's cluster as this wave knows it, not necessarily the
    // segment's own id: after a union both legs' entries are rewritten with the surviving root (compare-and-store against the
    // value the lane saw, so that a later cut's fresh id is never overwritten).  A two-site op whose legs already carry the same
    // representative — most of them, clusters being long-lived — then costs no union-find access at all, and the others start
    // their finds one hop from a root.  Any member of the cluster serves the apply pass and the range joins equally well.
    //
    // The touched flag without a longitudinal field (HAS_LONG = false) costs no store of its own.  An entry of a wave's table holds
    // its initial id (the placeholder id0 + v, or v itself in wave 0: unique to the variable, flag clear), a cut's id (written by
    // the cut lane as a whole word, flag set) or a root (written by the union block's compare-and-store, flag set).  At h == 0 every
    // op is a cut or a two-site op.  A cut flags its variable.  A two-site op whose legs differ runs the union block, which
    // rewrites BOTH legs' entries with the flag, the leg whose own id survives as the root included; where its compare-and-store
    // fails, a cut or a union of another lane wrote the entry first, with the flag.  A two-site op whose legs carry the same id on
    // different variables can only have met values that a cut or a union wrote: an untouched initial id is referenced by its own
    // entry alone.  Hence: variable v is touched in this wave's range <=> its entry carries SSE_CL_TOUCHED behind the scan (the test
    // of the join phase).  The leg words ua / uc keep the flag bit of the entry they were read from (LEGF), so that they are the
    // compare-and-store's expected word as they stand, and the id of a cut carries it through cutnext; where a clean id is needed
    // (the id stored for the apply pass, the parent-table address) the instruction that takes it reads the low half only.  With a
    // longitudinal field an op can act on a variable without cutting or linking: both legs store the flag byte, as before.
    constexpr uint32_t LEGF = HAS_LONG ? 0u : SSE_CL_TOUCHED, LEGM = 0xFFFFu | LEGF; // flag bit kept in a leg word; what a leg word keeps of its entry
    {
        uint32_t cutnext = (N + cutbase) | LEGF; // id of the next cut of this range (ids stay below 2^16: the flag rides along in the additions)
        const uint32_t packsel = vgpr_copy_u32(SSE_CL_PACK_SEL);
        uint32_t wnext[K], idpend[K / 2];
        // deferred flips: the cut mask and the two-site mask of every row are wave-uniform; dword c of row j's uint4 is collected in
        // lane 4 j + c of one register (v_writelane) and lanes 0 .. 4 K - 1 store the tile's masks with one dword store each
        uint32_t mpend = 0u;
        uint32_t *mskw = reinterpret_cast<uint32_t *>(msk);
#pragma unroll
        for (int j = 0; j < K; ++j) wnext[j] = row_ld(ops, pbeg + (uint32_t)(j * 64 + lane));
#pragma unroll
        for (int j = 0; j < K / 2; ++j) idpend[j] = 0u;
        uint32_t pprev = pbeg;
        // Parked unions.  A lane of the union blocks below whose find does not end inside the straight-line hops, or whose link
        // lost against another lane's, does not walk on there (a latency chain of LDS reads at whole-wave issue cost for one or
        // two lanes, in a fifth of the rows): it appends the pair of ancestors it reached to this wave's queue, and the pairs are
        // served together, one lane each, when the queue is full (looked at once per tile) and behind the scan.  Sound because
        // the partition a set of unions leaves does not depend on their order, and nothing in front of the barrier behind the
        // scan asks for more than a representative: the ids stored per slot and the table entries name members of the right
        // clusters once every parked union is done, which is when the apply pass and the joins read them.
        auto drain = [&](uint32_t cnt) {
            if ((uint32_t)lane < cnt) {
                const uint32_t pr = LDS32B(que_b + 4u * (uint32_t)lane);
                (void)cl_union_wave(uf, pr & 0xFFFFu, pr >> 16);
            }
            LDS32B(qcnt_b) = 0u;
        };
        for (uint32_t p0 = pbeg; p0 < pend; p0 += TS) {
            uint32_t e[K];
            const uint32_t qfill = LDS32B(qcnt_b); // (read here, used in front of the union blocks)
            {
                uint32_t word[K];
#pragma unroll
                for (int j = 0; j < K; ++j) word[j] = wnext[j];
                // the ids of the previous tile are stored here, in front of the prefetch: a wave's memory operations complete in
                // order, so waiting for the prefetched words at the top of the next tile then waits for stores that have had a
                // whole tile to complete, not for stores issued a moment ago (first tile: a dummy store that the next one overwrites)
#pragma unroll
                for (int j = 0; j < K; j += 2) if (!SSE_DBG(B, 1u)) row_st(ids, (pprev >> 1) + (uint32_t)(j * 32 + lane), idpend[j / 2]);
                if (DEFER) { if (lane < 4 * K) row_st(mskw, (pprev >> 6) * 4u + (uint32_t)lane, mpend); }
                pprev = p0;
                const uint32_t pn0 = p0 + TS < pend ? p0 + TS : p0;
#pragma unroll
                for (int j = 0; j < K; ++j) wnext[j] = row_ld(ops, pn0 + (uint32_t)(j * 64 + lane));
#pragma unroll
                for (int j = 0; j < K; ++j) e[j] = LDS32B(lds0 + 4u * (word[j] >> 4)); // entry (word >> 4) of the table at LDS word 0
            }
            uint32_t ua[K], uc[K], adra[K], adrc[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t aa = ent_b + 4u * (e[j] & 0x1FFFu), ac = ent_b + 4u * ((e[j] >> 13) & 0x1FFFu);
                adra[j] = aa; adrc[j] = ac;
                const bool iscut = (int32_t)e[j] < 0;
                const uint64_t cutm = sse_ballot(iscut);
                const uint32_t kown = __builtin_amdgcn_mbcnt_hi((uint32_t)(cutm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cutm, 0u));
                // In-row ordering: the cut lanes publish 1 + their rank inside the row in the marker byte of their variable's entry,
                // every lane reads once; a cut on the leg's variable precedes the lane iff its rank is below the lane's own count.
                const uint32_t acut = iscut ? aa : dummy_b; // the entry a cut lane writes: marker now, its new segment below
                LDS8B(acut + 2u) = (uint8_t)(kown + 1u);
                SSE_WAVE_FENCE();
                const uint32_t ea = LDS32B(aa), ec = LDS32B(ac);
                if constexpr (HAS_LONG) { LDS8B(aa + 3u) = (uint8_t)1; LDS8B(ac + 3u) = (uint8_t)1; } // touched flag (byte 3): plain stores with an immediate offset, nothing waits for them
                const uint32_t qa = (ea >> 16) & 0xFFu, qc = (ec >> 16) & 0xFFu;
                uint32_t seg_a = ea & LEGM, seg_c = ec & LEGM;
                const uint64_t dup = cutm & sse_ballot(qa != kown + 1u);
                if (!dup) {
                    seg_a = ((qa - 1u) < kown) ? cutnext + (qa - 1u) : seg_a; // qa == 0: no cut on the variable in this row
                    seg_c = ((qc - 1u) < kown) ? cutnext + (qc - 1u) : seg_c;
                    SSE_WAVE_FENCE();
                    LDS32B(acut) = (cutnext + kown) | (SSE_CL_TOUCHED & ~LEGF); // the segment the cut opens, touched; clears the marker
                } else { // two cuts of this row on one variable (rare): lane order decides
                    const uint32_t va = e[j] & 0x1FFFu, vc = (e[j] >> 13) & 0x1FFFu;
                    bool lastcut = iscut;
                    uint64_t m = cutm;
                    uint32_t idL = cutnext;
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
                    LDS8B(acut + 2u) = (uint8_t)0;
                    if (iscut & lastcut) { // the last cut wins
                        LDS16B(aa) = (uint16_t)(cutnext + kown);
                        if constexpr (!HAS_LONG) LDS8B(aa + 3u) = (uint8_t)1; // (the 16-bit store leaves the flag byte as it was)
                    }
                    SSE_WAVE_FENCE();
                }
                if constexpr (HAS_LONG)
                    if (e[j] & SSE_CLE_LONG) uf.frozen_or(seg_a >> 5, 1u << (seg_a & 31)); // qmc_ising.rs:759-775
                cutnext += (uint32_t)popc64(cutm);
                // the row's masks for a deferred apply pass, collected whether or not one follows: two v_writelane cost what the test
                // of the flag in front of them did (without a longitudinal field every op that is not a cut is a two-site op: the
                // cut mask alone will do)
                mpend = cl_writelane(mpend, (uint32_t)cutm, 4 * j); mpend = cl_writelane(mpend, (uint32_t)(cutm >> 32), 4 * j + 1);
                if constexpr (HAS_LONG) { // (without one, dwords 2 and 3 of a row stay 0)
                    const uint64_t twom = sse_ballot((e[j] & SSE_CLE_TWO) != 0u);
                    mpend = cl_writelane(mpend, (uint32_t)twom, 4 * j + 2); mpend = cl_writelane(mpend, (uint32_t)(twom >> 32), 4 * j + 3);
                }
                ua[j] = seg_a; uc[j] = seg_c; // (one-variable ops and empty slots: seg_c == seg_a, no union below)
            }
            // one 16-bit id per slot for the apply pass: the input leg's representative (a two-site op's other leg is in the same
            // cluster once its union below is done; a cut's own id is recomputed from the cut masks)
#pragma unroll
            for (int j = 0; j < K; j += 2) idpend[j / 2] = cl_pack_ids<HAS_LONG>(ua[j], ua[j + 1], packsel);
            // Unions: only the lanes whose two legs carry different representatives take part — a handful per tile once the
            // representatives have settled —, row by row, under their own exec mask (the union-find reads of a full wave at random
            // addresses would cost the LDS more than the whole scan).  Parents, grandparents (root test), link + read-back (two lanes
            // hooking one root); the trees a wave touches during the scan are private to it (own cuts, own placeholders): plain
            // stores, no atomics.  Anything deeper is parked (see above).
            if ((uint32_t)__builtin_amdgcn_readfirstlane((int)qfill) == SSE_CL_QCAP) { drain(SSE_CL_QCAP); LDS32B(qcnt_b + 4u) += 1u; }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const bool need = ua[j] != uc[j]; // (h == 0: equal ids carry equal flags, see LEGF)
                if (need && !SSE_DBG(B, 2u)) { // entered on the exec mask alone: a row without such a lane branches over the block
                    // SSE_CL_FIND_LEVELS hops up from each representative, straight-line (a representative is a root or close to one: it was
                    // a root when it was written); nodes found below a root are re-pointed at it on the way (they are not roots, so
                    // no link of this batch can be undone by that)
                    const uint32_t xa = cl_par_addr<HAS_LONG>(par_b, ua[j]), xc = cl_par_addr<HAS_LONG>(par_b, uc[j]); // (each parent address: one instruction)
                    const uint32_t pa = lds_ld16(xa), pc = lds_ld16(xc);
#if SSE_CL_FIND_LEVELS >= 3
                    uint32_t ga = lds_ld16(par_b + 2u * pa), gc = lds_ld16(par_b + 2u * pc);
#else // (two hops, timed in round 17 and slower: the parent is the candidate root, "found" below is ga == pa, nothing is re-pointed)
                    uint32_t ga = pa, gc = pc;
#endif
                    uint32_t ta = lds_ld16(par_b + 2u * ga), tc = lds_ld16(par_b + 2u * gc);
#pragma unroll
                    for (int lv = 3; lv < SSE_CL_FIND_LEVELS; ++lv) { // (further levels: the candidate root moves one hop up)
                        const uint32_t na = lds_ld16(par_b + 2u * ta), nc = lds_ld16(par_b + 2u * tc);
                        ga = ta; gc = tc; ta = na; tc = nc;
                    }
                    const bool found = (ta == ga) & (tc == gc); // ga / gc are roots (also when the chain is shorter: a root is its own parent)
                    const bool differ = ga != gc;
                    const bool link = found & differ;
                    uint32_t lo = min(ga, gc);
                    const uint32_t hi = max(ga, gc);
                    const uint32_t xh = par_b + 2u * hi;
                    LDS16B((found & (pa != ga)) ? xa : dummy_b) = (uint16_t)ga;
                    LDS16B((found & (pc != gc)) ? xc : dummy_b) = (uint16_t)gc;
                    LDS16B(link ? xh : dummy_b) = (uint16_t)lo;
                    SSE_WAVE_FENCE();
                    const uint32_t chk = lds_ld16(xh);
#ifdef SSE_CL_UNION_COUNTERS // (a diagnostic build of its own: the counters cost the union block a quarter of its time)
                    if (wave == 3) { // why rows reach the serial routine
                        const uint64_t nf = sse_ballot(!found), cf = sse_ballot(found & link & (chk != lo)), nd = sse_ballot(true);
                        if (lane == (int)(__ffsll((long long)nd) - 1)) {
                            B.dbg[(size_t)r * 16 + 8] += 1; B.dbg[(size_t)r * 16 + 12] += (uint64_t)popc64(nd);
                            if (nf) B.dbg[(size_t)r * 16 + 9] += 1;
                            if (!nf && cf) B.dbg[(size_t)r * 16 + 10] += 1;
                            B.dbg[(size_t)r * 16 + 13] += (uint64_t)popc64(nf); B.dbg[(size_t)r * 16 + 14] += (uint64_t)popc64(cf);
                        }
                    }
#endif
                    if ((!found | (link & (chk != lo))) && !SSE_DBG(B, 16u)) {
                        // park the union of the highest ancestors the hops reached (found: the two roots) behind the pairs the
                        // queue holds: the count and, of the lanes in here, those below this one.  (Re-pointing the legs' start
                        // nodes at these ancestors as well, and a returning LDS add for the position, were timed and are slower.)
                        const uint64_t bm = sse_ballot(true); // the lanes in here
                        const uint32_t fill = LDS32B(qcnt_b);
                        const uint32_t pos = fill + __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
                        LDS32B(qcnt_b) = min(fill + (uint32_t)popc64(bm), SSE_CL_QCAP);
                        lo = min(ta, tc); // (found: min(ga, gc) as before)
                        if (pos < SSE_CL_QCAP) LDS32B(que_b + 4u * pos) = ta | (tc << 16);
                        else lo = cl_union_wave(uf, ta, tc); // the queue is full until the next tile looks at it: served here, as every such lane used to be
                    }
                    // both legs' entries now name the surviving root (or the common parent found one hop up; parked: the smaller of
                    // the two ancestors, a member of the cluster both legs are in once the queue is served), touched.  Expected is
                    // the word the entry held when the lane looked it up (h == 0: the leg word itself, an untouched initial id
                    // included; h != 0: the id, which the byte store of the scan has flagged): the store fails only where a cut or a
                    // union of another lane rewrote the entry first, and those write the flag too
                    lds_cas32(adra[j], ua[j] | (SSE_CL_TOUCHED & ~LEGF), lo | SSE_CL_TOUCHED);
                    lds_cas32(adrc[j], uc[j] | (SSE_CL_TOUCHED & ~LEGF), lo | SSE_CL_TOUCHED);
                }
            }
        }
        if (pbeg < pend) {
#pragma unroll
            for (int j = 0; j < K; j += 2) row_st(ids, (pprev >> 1) + (uint32_t)(j * 32 + lane), idpend[j / 2]);
            if (DEFER) { if (lane < 4 * K) row_st(mskw, (pprev >> 6) * 4u + (uint32_t)lane, mpend); }
        }
        // what is still parked, in front of the barrier: behind it every id and table entry is read as what it stands for
        const uint32_t qlast = (uint32_t)__builtin_amdgcn_readfirstlane((int)LDS32B(qcnt_b));
        const uint32_t qdrains = (uint32_t)__builtin_amdgcn_readfirstlane((int)LDS32B(qcnt_b + 4u));
        drain(qlast);
        // for the tests (isingmc_debug_phase_ticks, every build): unions this replica's waves parked, drains in front of the last
        if (lane == 0 && (qlast | qdrains)) {
            atomicAdd(&B.dbg[(size_t)r * 16 + 11], (unsigned long long)(qdrains * SSE_CL_QCAP + qlast));
            if (qdrains) atomicAdd(&B.dbg[(size_t)r * 16 + 15], (unsigned long long)qdrains);
        }
    }
    __syncthreads();
    SSE_STAMP(1);

    // ---- join the ranges (the segment a worldline is in when range w ends continues into the placeholder of range w + 1; the
    // last range wraps into [0, N): cluster.rs:223-242), collect the touched bits ----
    // One thread per variable, 16 joins each: two finds and, where the roots differ, the compare-and-swap loop (what uf_union does,
    // with the finds in front so that a diagnostic build can count them).  Wave wv takes the boundaries in the order (k + wv) & 15:
    // at any moment the 16 waves then work on 16 different boundaries instead of meeting at the same pairs of roots, where all but
    // one of the threads that try a link lose it and find again (at the headline size 62 % of the attempts were lost, now 25 %).
    // The partition a set of unions leaves and its smallest-id roots do not depend on the order of the unions.
    {
#ifdef SSE_CL_JOIN_COUNTERS // (a diagnostic build of its own) per replica: joins, joins whose first finds agree, compare-and-swap attempts, lost ones
        uint32_t jc_joins = 0, jc_agree = 0;
#endif
        uint32_t jc_att = 0, jc_lost = 0; // (dead without SSE_CL_JOIN_COUNTERS)
        for (uint32_t v = tid; v < N; v += NT) {
            uint32_t t = 0;
#pragma unroll 4
            for (uint32_t k = 0; k < (uint32_t)W; ++k) {
                const uint32_t w2 = SSE_CL_JOIN_ROTATE ? ((k + (uint32_t)wave) & (uint32_t)(W - 1)) : k;
                const uint32_t x = LDSW(L.o_ent, w2 * (N + 1u) + v);
                t |= x;
                const uint32_t seg_end = x & 0xFFFFu;
                const uint32_t nxt = (w2 + 1u == (uint32_t)W) ? v : N + C + w2 * N + v;
                if (seg_end != nxt) {
                    const uint32_t a = uf_find(uf, seg_end), b = uf_find(uf, nxt);
                    if (a != b) cl_link_roots(uf, a, b, jc_att, jc_lost);
#ifdef SSE_CL_JOIN_COUNTERS
                    jc_joins++; jc_agree += a == b;
#endif
                }
            }
            if (t >> 24) atomicOr(&LDSW(L.o_touch, v >> 5), 1u << (v & 31));
        }
#ifdef SSE_CL_JOIN_COUNTERS
        if (jc_joins) atomicAdd(&B.dbg[(size_t)r * 16 + 8], (unsigned long long)jc_joins);
        if (jc_agree) atomicAdd(&B.dbg[(size_t)r * 16 + 9], (unsigned long long)jc_agree);
        if (jc_att) atomicAdd(&B.dbg[(size_t)r * 16 + 10], (unsigned long long)jc_att);
        if (jc_lost) atomicAdd(&B.dbg[(size_t)r * 16 + 12], (unsigned long long)jc_lost);
#endif
    }
    __syncthreads();
    SSE_STAMP(2);
    // ---- flatten: parent[i] := exact root; frozen marks move to the roots.  The same pass lists the roots: the per-wave tables are
    // dead behind the barrier above, their words now hold the flip bits (S bits) and, behind them, the list of roots (u16); the
    // touched bits are complete as well.  A root's entry is its own id from the joins on and nobody rewrites it, so "my find ends
    // at myself" is final here (only exact roots are ever stored in this pass: uf_find_ro) ----
    const uint32_t o_bits = L.o_ent, o_list = L.o_ent + (S + 31u) / 32u;
    const uint32_t list_cap = cl_list_cap(N, S);
    uint32_t myclusters = 0;
    // A thread walks SSE_CL_FLATTEN_BATCH ids to their roots together: the walks are chains of dependent LDS reads, and with four
    // waves per SIMD nothing else hides their latency
    constexpr int FB = SSE_CL_FLATTEN_BATCH;
    for (uint32_t i0 = 0; i0 < S; i0 += NT * FB) { // whole waves iterate together (ballot below)
        uint32_t fx[FB], fp[FB];
#pragma unroll
        for (int f = 0; f < FB; ++f) {
            const uint32_t i = i0 + (uint32_t)(f * NT + tid);
            fx[f] = i < S ? i : 0u; // (beyond the ids: id 0, a root)
            fp[f] = lds_ld16(par_b + 2u * fx[f]);
        }
        for (;;) { // read-only, as uf_find_ro
            bool more = false;
#pragma unroll
            for (int f = 0; f < FB; ++f) { more |= fp[f] != fx[f]; fx[f] = fp[f]; }
            if (!more) break;
#pragma unroll
            for (int f = 0; f < FB; ++f) fp[f] = lds_ld16(par_b + 2u * fx[f]);
        }
        uint64_t m[FB];
        bool isr[FB];
        uint32_t nroot = 0; // roots of the wave in this batch: one append to the list for all of them
#pragma unroll
        for (int f = 0; f < FB; ++f) {
            const uint32_t i = i0 + (uint32_t)(f * NT + tid);
            bool isroot = false;
            if (i < S) {
                const uint32_t root = fx[f];
                uf.set(i, root);
                if constexpr (HAS_LONG)
                    if ((uf.frozen_get(i >> 5) >> (i & 31)) & 1u) { uf.froot_or(root >> 5, 1u << (root & 31)); LDSW(L.o_misc, MISC_ANYFROZEN) = 1u; }
                isroot = root == i;
                if (isroot & (i < N + C)) {
                    const bool touched = (i >= N) || ((LDSW(L.o_touch, i >> 5) >> (i & 31)) & 1u);
                    if (touched) myclusters++;
                }
            }
            isr[f] = isroot;
            m[f] = sse_ballot(isroot);
            nroot += (uint32_t)popc64(m[f]);
        }
        if (nroot) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&LDSW(L.o_misc, MISC_LOOP_A), nroot);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
            for (int f = 0; f < FB; ++f) {
                const uint32_t pos = base + popc64(m[f] & lanemask_lt(lane));
                if (isr[f] && pos < list_cap) LDSH(o_list, pos) = (uint16_t)(i0 + (uint32_t)(f * NT + tid));
                base += (uint32_t)popc64(m[f]);
            }
        }
    }
    for (uint32_t i = tid; i < (S + 31u) / 32u; i += NT) LDSW(o_bits, i) = 0u;
    __syncthreads();
    SSE_STAMP(3);
    // ---- coins: one Philox draw per root (= per cluster, keyed by the canonical label = smallest id), cluster.rs:111-137 ----
    const Rng rng = make_rng(B, r, epoch);
    const uint32_t nroots = LDSW(L.o_misc, MISC_LOOP_A);
    if (nroots <= list_cap) { // uniform: every thread read the same counter
        for (uint32_t k = tid; k < nroots; k += NT) {
            const uint32_t root = LDSH(o_list, k);
            const uint4 o = rng.draw(SSE_TAG_CLUSTER, root);
            const uint32_t isfrozen = HAS_LONG ? (uf.froot_get(root >> 5) >> (root & 31)) & 1u : 0u;
            if (!isfrozen && u01(o.x) < A.prob) atomicOr(&LDSW(o_bits, root >> 5), 1u << (root & 31));
        }
        __syncthreads();
        for (uint32_t i = tid; i < S; i += NT) {
            const uint32_t root = uf.get(i);
            uf.set(i, (LDSW(o_bits, root >> 5) >> (root & 31)) & 1u);
        }
    } else { // more roots than the list holds: every id draws the coin of its root itself (same results)
        for (uint32_t i = tid; i < S; i += NT) {
            const uint32_t root = uf.get(i);
            const uint4 o = rng.draw(SSE_TAG_CLUSTER, root);
            const uint32_t isfrozen = HAS_LONG ? (uf.froot_get(root >> 5) >> (root & 31)) & 1u : 0u;
            uf.set(i, (!isfrozen && u01(o.x) < A.prob) ? 1u : 0u);
        }
    }
    if (tid == 0) uf.set(S, 0u); // the null id never flips
    {
        uint32_t c = myclusters;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
        if (lane == 0 && c) atomicAdd(&LDSW(L.o_misc, MISC_NCLUST), c);
    }
    __syncthreads();
    SSE_STAMP(4);

    // ---- apply (cluster.rs:139-167): input bits flip with the incoming segment, output bits with the outgoing one ----
    if (DEFER) {
        // Deferred: the op-string is not touched.  Every slot gets the xor mask of its four state bits as one byte (0 for an empty
        // slot); the diagonal pass of the next timestep applies it while it streams the string (sse_fast.hip.h), any other reader
        // goes through materialize_kernel first.  Reads 2 B of ids + 16 B of row masks per row, writes 1 B per slot: a quarter
        // of the traffic of the in-place pass below.
        uint32_t cutnext = N + cutbase;
        uint8_t *fb = B.flipb + (size_t)r * B.stride;
        // The loop body is short, so the loads run D tiles ahead (one tile per memory round trip would leave the pass waiting):
        // per tile two dwords of ids per lane and the 64 bytes of row masks, one dword per lane 0..15 (read back with v_readlane).
        // The tile loop is unrolled D times, so that the D slots of the queue change roles instead of contents, and every access
        // is (tile base, scalar) + (lane offset, the same in every tile) + (row offset, an immediate): one address per tile for
        // the ids, one for the masks and one for the stores.
        constexpr int D = 3;
        const uint32_t *mskw = reinterpret_cast<const uint32_t *>(msk);
        uint32_t qid[D][K / 2], qmk[D], bpend[K];
        const uint32_t lane4 = 4u * (uint32_t)lane, lane15_4 = 4u * (uint32_t)(lane & 15);
        auto issue = [&](int slot, uint32_t pt) { // loads of the tile at pt (clamped to the last tile of the range: values unused beyond it)
            const uint32_t pc = pt < pend ? pt : pbeg;
            const char *idt = reinterpret_cast<const char *>(ids + (pc >> 1));
            const char *mkt = reinterpret_cast<const char *>(mskw + (pc >> 6) * 4u);
#pragma unroll
            for (int j = 0; j < K; j += 2)
                qid[slot][j / 2] = *reinterpret_cast<const uint32_t *>(idt + (size_t)lane4 + (size_t)(j * 128));
            qmk[slot] = *reinterpret_cast<const uint32_t *>(mkt + (size_t)lane15_4);
        };
        auto store = [&](uint32_t pt) { // the flip bytes of the tile at pt
            uint8_t *fbt = fb + pt;
#pragma unroll
            for (int j = 0; j < K; ++j) fbt[(size_t)(uint32_t)lane + (size_t)(j * 64)] = (uint8_t)bpend[j];
        };
        auto tile = [&](int slot) { // flip bytes of the tile whose loads are in `slot`
            const uint32_t mkv = qmk[slot];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint64_t cutm = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mkv, 4 * j) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mkv, 4 * j + 1) << 32);
                // the id a cut opens: cutnext + (cuts below the lane); the scalar is added behind the count instead of seeding it
                const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(cutm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cutm, 0u));
                const uint32_t idw = qid[slot][j / 2];
                const uint32_t idin = (j & 1) ? (idw >> 16) : cl_low16(idw);
                const uint32_t f1 = LDS16B(par_b + 2u * idin), f2 = LDS16B(par_b + 2u * (cutnext + below));
                uint32_t m_other = __umul24(f1, 0xFu); // two-site: all four bits follow the one cluster (a flip is 0 or 1)
                if constexpr (HAS_LONG) { // longitudinal op: both bits of its variable
                    const uint64_t twom = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mkv, 4 * j + 2) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mkv, 4 * j + 3) << 32);
                    m_other &= sel64(twom, vgpr_copy_u32(0xFu), vgpr_copy_u32(0x5u));
                }
                bpend[j] = sel64(cutm, f1 | (f2 << 2), m_other);
                cutnext += (uint32_t)popc64(cutm);
            }
        };
#pragma unroll
        for (int d = 0; d < D; ++d) issue(d, pbeg + (uint32_t)d * TS);
        // a tile's bytes are stored in front of the next tile's prefetch (see the build loop); the first tile has none in front
        if (pbeg < pend) {
            uint32_t p0 = pbeg;
            for (;;) {
                bool done = false;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    if (d > 0 || p0 != pbeg) store(p0 - TS);
                    tile(d);
                    issue(d, p0 + (uint32_t)D * TS);
                    p0 += TS;
                    if (p0 >= pend) { done = true; break; }
                }
                if (done) break;
            }
            store(p0 - TS);
        }
    } else
    {
        uint32_t cutnext = N + cutbase;
        const uint32_t E1 = B.E + 1u;
        uint32_t wnext[K], inext[K / 2], wpend[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { wnext[j] = row_ld(ops, pbeg + (uint32_t)(j * 64 + lane)); wpend[j] = wnext[j]; }
#pragma unroll
        for (int j = 0; j < K; j += 2) inext[j / 2] = row_ld(ids, (pbeg >> 1) + (uint32_t)(j * 32 + lane));
        uint32_t pprev = pbeg;
        for (uint32_t p0 = pbeg; p0 < pend; p0 += TS) {
            uint32_t word[K], id2[K / 2];
#pragma unroll
            for (int j = 0; j < K; ++j) word[j] = wnext[j];
#pragma unroll
            for (int j = 0; j < K / 2; ++j) id2[j] = inext[j];
            {
                // the previous tile's words are stored in front of this tile's prefetch (see the build loop; first tile: its own
                // words, unchanged)
#pragma unroll
                for (int j = 0; j < K; ++j) row_st(ops, pprev + (uint32_t)(j * 64 + lane), wpend[j]);
                pprev = p0;
                const uint32_t pn0 = p0 + TS < pend ? p0 + TS : p0;
#pragma unroll
                for (int j = 0; j < K; ++j) wnext[j] = row_ld(ops, pn0 + (uint32_t)(j * 64 + lane));
#pragma unroll
                for (int j = 0; j < K; j += 2) inext[j / 2] = row_ld(ids, (pn0 >> 1) + (uint32_t)(j * 32 + lane));
            }
            // straight-line: both flip lookups are issued for every lane (lanes that hold no cut read a valid id, at most the first
            // id of the next range; empty slots carry the null id, whose flip is 0, so their word stays 0 without a test)
            uint32_t f1[K], f2[K];
            uint64_t cutm[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                cutm[j] = sse_ballot(((word[j] >> 4) - E1) < N); // bonds [E, E + N): transverse field
                const uint32_t own = __builtin_amdgcn_mbcnt_hi((uint32_t)(cutm[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cutm[j], cutnext));
                const uint32_t idin = (j & 1) ? (id2[j / 2] >> 16) : (id2[j / 2] & 0xFFFFu);
                f1[j] = LDS16B(par_b + 2u * idin);
                f2[j] = LDS16B(par_b + 2u * own); // the segment a cut opens
                cutnext += (uint32_t)popc64(cutm[j]);
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                // two-site: all four bits follow the one cluster; longitudinal: both bits of its variable; cut: input with the incoming,
                // output with the outgoing segment
                const uint32_t allbits = (((word[j] >> 4) - 1u) < B.E) ? 0xFu : 0x5u;
                const uint32_t m_other = (0u - f1[j]) & allbits;
                const uint32_t m_cut = f1[j] | (f2[j] << 2);
                wpend[j] = word[j] ^ sel64(cutm[j], m_cut, m_other);
            }
        }
        if (pbeg < pend) {
#pragma unroll
            for (int j = 0; j < K; ++j) row_st(ops, pprev + (uint32_t)(j * 64 + lane), wpend[j]);
        }
    }
    // p=0 state follows the initial segment of each touched variable
    // (one variable per thread: a wave's ballot is two whole state words, lanes 0 and 1 take one each)
    for (uint32_t v0 = (uint32_t)wave * 64u; v0 < N; v0 += NT) {
        const uint32_t v = v0 + (uint32_t)lane;
        const uint64_t fm = sse_ballot(v < N && (uf.get(v) & 1u) != 0u);
        const uint32_t i = (v0 >> 5) + (uint32_t)lane;
        if (lane < 2 && i < nwords) LDSW(L.o_state, i) ^= (lane ? (uint32_t)(fm >> 32) : (uint32_t)fm) & LDSW(L.o_touch, i);
    }
    __syncthreads();
    SSE_STAMP(5);
    const uint32_t nclusters = LDSW(L.o_misc, MISC_NCLUST);
    epoch++;
    uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, a6 = 0;
    // ---- free spins (qmc_ising.rs:780-784) ----
    if (A.domask & SSE_DO_FREE) {
        const Rng rngf = make_rng(B, r, epoch);
        for (uint32_t v0 = (uint32_t)wave * 64u; v0 < N; v0 += NT) { // (same layout: an untouched variable draws, a touched one keeps its bit)
            const uint32_t v = v0 + (uint32_t)lane;
            const bool isfree = v < N && !((LDSW(L.o_touch, v >> 5) >> (v & 31u)) & 1u);
            uint32_t bit = 0u;
            if (isfree) bit = rngf.draw(SSE_TAG_FREE, v).x >> 31;
            const uint64_t fm = sse_ballot(isfree), bm = sse_ballot(bit != 0u);
            const uint32_t i = (v0 >> 5) + (uint32_t)lane;
            if (fm != 0ull && lane < 2 && i < nwords) {
                const uint32_t f = lane ? (uint32_t)(fm >> 32) : (uint32_t)fm, b = lane ? (uint32_t)(bm >> 32) : (uint32_t)bm;
                LDSW(L.o_state, i) = (LDSW(L.o_state, i) & ~f) | b;
            }
        }
        __syncthreads();
        epoch++;
    }
    // ---- sampling (qmc_stepper.rs:149-161) ----
    if (A.sampling_freq && (A.step0 + 1) % A.sampling_freq == 0) {
        if (tid == 0) LDSW(L.o_misc, MISC_LOOP_A) = 0u;
        __syncthreads();
        uint32_t up = 0;
        for (uint32_t i = tid; i < nwords; i += NT) up += __popc(LDSW(L.o_state, i));
        for (int off = 32; off > 0; off >>= 1) up += __shfl_down(up, off);
        if (lane == 0 && up) atomicAdd(&LDSW(L.o_misc, MISC_LOOP_A), up);
        __syncthreads();
        const long long mag = 2ll * (long long)LDSW(L.o_misc, MISC_LOOP_A) - (long long)N;
        a0 = (uint64_t)n; a1 = 1; a2 = (uint64_t)(mag < 0 ? -mag : mag); a3 = (uint64_t)(mag * mag); a6 = (uint64_t)C;
    }
    for (uint32_t i = tid; i < nwords; i += NT) B.state[(size_t)r * nwords + i] = LDSW(L.o_state, i);
    if (tid == 0) {
        B.epoch[r] = epoch;
        if (DEFER) B.pend[r] = 1u; // (behind the barriers above: every wave's flip bytes are on their way; the kernel boundary orders them)
        if (A.out_u32) A.out_u32[r] = nclusters;
        uint64_t *acc = B.acc + (size_t)B.acc_row[r] * 8;
        acc[0] += a0; acc[1] += a1; acc[2] += a2; acc[3] += a3; acc[4] += (uint64_t)n; acc[6] += a6;
    }
}

} // namespace sse
