// lds_plan.hip — lds_plan.h over the kernels' own carves: the one host-side translation unit that includes kernel headers, and it
// launches nothing.
#include "lds_plan.h"
#include "sse_core.hip.h" // Lds<W>::carve
#include "sse_fast.hip.h" // fast_carve
#include "sse_rvb.hip.h"  // rvb_carve

#include <algorithm>

namespace sse {

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
size_t general_lds_words(uint32_t W, const DevBatch &D, uint32_t ledges, bool tg, uint32_t pm_words, uint32_t ufcap) {
    return with_lds(W, [&](auto L) { L.carve(D.N, D.nwords, ufcap, ledges, D.has_long, tg, pm_words); return (size_t)L.end; });
}
size_t diag_lds_words(uint32_t W, const DevBatch &D, uint32_t ledges, bool tg, uint32_t pm_words, bool diag_only) {
    return with_lds(W, [&](auto L) { L.carve(D.N, D.nwords, 0u, ledges, 0u, tg, pm_words, diag_only); return (size_t)L.end_diag; });
}
size_t fast_lds_words(const DevBatch &D) {
    Lds<4> L;
    L.carve(D.N, D.nwords, 0u, D.E, 0u);
    return std::max<size_t>(fast_carve<4>(L, D).end, L.o_signs);
}
size_t rvb_lds_words(uint32_t W, const DevBatch &D, uint32_t ledges, bool tg, uint32_t pm_words) {
    return with_lds(W, [&](auto L) { RvbLds R; L.carve(D.N, D.nwords, 0u, ledges, 0u, tg, pm_words); rvb_carve(R, L, D); return (size_t)R.o_cps + D.cap; });
}
size_t rvb_global_lds_words(const DevBatch &D, uint32_t ledges, uint32_t areas) {
    Lds<16> L; RvbLds R;
    L.carve(D.N, D.nwords, 0u, ledges, 0u, true);
    rvb_carve<16, true>(R, L, D);
    return (size_t)R.o_free + (size_t)areas * SSE_RVB_SLOT_WORDS;
}
size_t rvb_tbl_words(const DevBatch &D) { return rvb_tbl_words(D.N, D.E, D.cap); }

LdsPlan plan_lds(const LdsNeeds &n, uint32_t W) {
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

} // namespace sse
