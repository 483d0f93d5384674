// sse_unionfind.hip.h — the lock-free union-find of the cluster updates, in LDS or HBM (sse_cluster_pass.hip.h, sse_cluster.hip.h).
#pragma once
#include "sse_core.hip.h"

namespace sse {

// Union-find storage: LDS (fast path) or the per-replica HBM scratch (when N + #cuts exceeds the LDS
// capacity).  The accessor keeps the address space static so that the LDS path compiles to ds_* ops.
template <bool G>
struct UFA {
    uint32_t *gparent, *gfrozen, *gfroot; // HBM arrays (G)
    uint32_t o_parent, o_frozen, o_froot; // lds_raw offsets (!G)
    __device__ __forceinline__ uint32_t get(uint32_t i) const { if constexpr (G) return gparent[i]; else return (uint32_t)LDSH(o_parent, i); }
    __device__ __forceinline__ void set(uint32_t i, uint32_t v) const { if constexpr (G) gparent[i] = v; else LDSH(o_parent, i) = (uint16_t)v; }
    __device__ __forceinline__ uint32_t cas(uint32_t i, uint32_t cmp, uint32_t v) const {
        if constexpr (G) return atomicCAS(&gparent[i], cmp, v);
        else {
            // 16-bit compare-and-swap through a 32-bit CAS on the containing word; a concurrent 16-bit store to
            // the other half only makes the CAS fail and retry with the value it returned
            const uint32_t widx = i >> 1, sh = (i & 1u) * 16u;
            uint32_t old = __hip_atomic_load(&LDSW(o_parent, widx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            for (;;) {
                const uint32_t cur = (old >> sh) & 0xFFFFu;
                if (cur != cmp) return cur;
                const uint32_t neww = (old & ~(0xFFFFu << sh)) | (v << sh);
                const uint32_t prev = atomicCAS(&LDSW(o_parent, widx), old, neww);
                if (prev == old) return cmp;
                old = prev;
            }
        }
    }
    __device__ __forceinline__ void frozen_or(uint32_t w, uint32_t bits) const { if constexpr (G) atomicOr(&gfrozen[w], bits); else atomicOr(&LDSW(o_frozen, w), bits); }
    __device__ __forceinline__ void froot_or(uint32_t w, uint32_t bits) const { if constexpr (G) atomicOr(&gfroot[w], bits); else atomicOr(&LDSW(o_froot, w), bits); }
    __device__ __forceinline__ uint32_t frozen_get(uint32_t w) const { if constexpr (G) return gfrozen[w]; else return LDSW(o_frozen, w); }
    __device__ __forceinline__ uint32_t froot_get(uint32_t w) const { if constexpr (G) return gfroot[w]; else return LDSW(o_froot, w); }
    __device__ __forceinline__ void bits_clear(uint32_t w) const {
        if constexpr (G) { gfrozen[w] = 0u; gfroot[w] = 0u; } else { LDSW(o_frozen, w) = 0u; LDSW(o_froot, w) = 0u; }
    }
};

// Lock-free union-find with smallest-id roots (canonical cluster labels).
template <bool G>
__device__ __forceinline__ uint32_t uf_find(const UFA<G> &uf, uint32_t x) {
    uint32_t p = uf.get(x);
    while (p != x) {
        const uint32_t g = uf.get(p);
        if (g != p) uf.set(x, g); // path halving; benign race (always an ancestor)
        x = p;
        p = g;
    }
    return x;
}
// Read-only find for the flatten phase: there the owner of id i overwrites parent[i] with the exact root, and a
// path-halving store from another thread's walk could land after it and put a non-root ancestor back.
template <bool G>
__device__ __forceinline__ uint32_t uf_find_ro(const UFA<G> &uf, uint32_t x) {
    uint32_t p = uf.get(x);
    while (p != x) { x = p; p = uf.get(x); }
    return x;
}
template <bool G>
__device__ __forceinline__ void uf_union(const UFA<G> &uf, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(uf, a);
        b = uf_find(uf, b);
        if (a == b) return;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        if (uf.cas(b, b, a) == b) return;
    }
}

// Union on trees that only the calling wave touches (cluster scan): plain stores; lanes that hook the same root in
// one instruction are detected by reading the parent back.
template <bool G>
__device__ __forceinline__ void uf_union_wave(const UFA<G> &uf, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(uf, a);
        b = uf_find(uf, b);
        if (a == b) return;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        uf.set(b, a);
        SSE_WAVE_FENCE();
        if (uf.get(b) == a) return;
    }
}

} // namespace sse
