// lds_plan.h — from a model's shape to the dynamic LDS words of every kind of launch (lds_plan.hip, the one host file that includes the
// kernels' carves), and the plan of a general launch's LDS union-find.  Plain C++ over sse_batch.h: create.hip, driver.hip and
// isingmc_hip.hip size their launches through it and see no kernel header.
#pragma once
#include <stddef.h>
#include "sse_batch.h"

namespace sse {

inline bool is_tg(uint32_t mode) { return mode == SSE_MODE_GLOBAL_TABLES || mode == SSE_MODE_PM_GLOBAL_TABLES; }
inline bool is_pm(uint32_t mode) { return mode == SSE_MODE_PM_GLOBAL_TABLES; }
inline uint32_t lds_edges(uint32_t mode, const DevBatch &D) { return mode == SSE_MODE_LDS_EDGES ? D.E : 0u; } // compact edge table words in LDS
// the wave counts per replica that the kernels are built for (sweep_w*.hip), and a count's place among them (-1: not one)
constexpr uint32_t WAVES[5] = {1, 4, 6, 8, 16};
inline int wave_index(uint32_t W) { for (int i = 0; i < 5; ++i) if (WAVES[i] == W) return i; return -1; }

// Dynamic LDS of every kind of launch, read off the carve its kernel lays its LDS out with (the carves are the only statement of
// the layouts; what the host adds on top — constant-op tables, growth areas, headroom — is policy and stays at the call sites).
// general / off-diagonal launch at W waves whose LDS union-find holds ufcap ids (tg: per-variable tables in HBM; pm_words: +-J signs)
size_t general_lds_words(uint32_t W, const DevBatch &D, uint32_t ledges, bool tg, uint32_t pm_words, uint32_t ufcap);
// diagonal-pass launch (diag_only: the +-J decode's diagonal kernel, mode SSE_MODE_PM_LDS_TABLES)
size_t diag_lds_words(uint32_t W, const DevBatch &D, uint32_t ledges, bool tg, uint32_t pm_words, bool diag_only = false);
// trimmed diagonal-pass launch (sse_fast.hip.h): its tables, or the compact edge table that the directed loop behind the pass stages
// in the same place
size_t fast_lds_words(const DevBatch &D);
// RVB sweep inside the general kernel at W waves: its scratch (rvb_carve) and a constant-op table of cap entries (cutoff <= cap)
size_t rvb_lds_words(uint32_t W, const DevBatch &D, uint32_t ledges, bool tg, uint32_t pm_words);
// RVB sweep with its tables in HBM (SSE_PASSES_RVB_G, 16 waves): the LDS scratch of rvb_carve<16, true> and `areas` small growth areas
size_t rvb_global_lds_words(const DevBatch &D, uint32_t ledges, uint32_t areas);
// ... and the words per replica of those tables (DevBatch::rvb_tbl)
size_t rvb_tbl_words(const DevBatch &D);
// bytes of a launch of `words` dynamic LDS words (whole 8-byte units)
inline size_t lds_bytes_of(size_t words) { return (4 * words + 7) & ~(size_t)7; }

// LDS footprint of the next launch.  The union-find of the cluster pass lives in LDS as 16-bit parents when all
// ids fit; its capacity follows the largest transverse-op count seen so far (+ headroom), so that the footprint
// stays small enough for two workgroups per CU whenever the model allows it.  Replicas that outgrow it use the HBM
// union-find for that sweep and the host enlarges the table before the next launch.
struct LdsPlan { uint32_t W, ufcap; size_t words; bool all_ids_fit; };
// What such a plan is made from: the model's shape (D: N, E, cap, nwords, has_long, pm_words), the batch's mode, all of LDS, the
// test limit on the ids and the largest transverse-op count seen so far
struct LdsNeeds { const DevBatch &D; uint32_t mode; size_t total_words; uint32_t uf_ids_limit, max_ntrans; };
// ids that the union-find of a launch at W waves is sized for: W per variable, the transverse ops seen so far, headroom
inline size_t uf_ids_wanted(const LdsNeeds &n, uint32_t W) { return (size_t)W * n.D.N + n.max_ntrans + n.max_ntrans / 16 + 384; }
LdsPlan plan_lds(const LdsNeeds &n, uint32_t W);

} // namespace sse
