// Instantiations of sse::rvb_grow_kernel / sse::rvb_main_kernel (sse_rvb_split.hip.h): the RVB sweep as two launches.
#include "sse_launch.h"
#include "sse_rvb_split.hip.h"
namespace sse {
template <bool CL>
static hipError_t launch_grow_one(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    return launch_lds(rvb_grow_kernel<CL>, dim3(B.R), dim3(1024), c.lds_bytes, c.stream, B, A);
}
template <int W, bool CL>
static hipError_t launch_main_one(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    return launch_lds(rvb_main_kernel<W, CL>, dim3(B.R), dim3(W * 64), c.lds_bytes, c.stream, B, A);
}
uint32_t rvb_grow_table_start(const DevBatch &B, uint32_t ledges) { Lds<16> L; RvbLds R; L.carve(B.N, B.nwords, 0u, ledges, 0u); rvb_carve_grow<16>(R, L, B); return R.o_cps; }
template <int W>
static uint32_t rvb_main_end(const DevBatch &B, uint32_t ledges) {
    Lds<W> L; RvbLds R; RvbMainLds P;
    rvb_carve_main<W>(L, R, P, B, ledges); // (its end: the record region is its last; a field for it changes rvb_main_kernel's registers)
    return P.o_big + rvb_region_words(rvb_bm_words(B.Nb));
}
uint32_t rvb_main_lds_words(uint32_t W, const DevBatch &B, uint32_t ledges) {
    return W == 4 ? rvb_main_end<4>(B, ledges) : (W == 8 ? rvb_main_end<8>(B, ledges) : rvb_main_end<16>(B, ledges));
}
size_t rvb_split_prod_stride(uint32_t Nb) { return rvb_bm_words(Nb) <= SSE_RVB_BM_MAX ? SSE_RVB_PROD_STRIDE + rvb_bm_words(Nb) : 0u; }
hipError_t launch_rvb_grow(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    if (!B.rvb_prod) return hipErrorInvalidValue;
    if (c.mode == SSE_MODE_LDS_EDGES) return launch_grow_one<true>(c, B, A);
    if (c.mode == SSE_MODE_GENERAL) return launch_grow_one<false>(c, B, A);
    return hipErrorInvalidValue;
}
hipError_t launch_rvb_main(const LaunchCfg &c, const DevBatch &B, const SweepArgs &A) {
    if (!B.rvb_prod) return hipErrorInvalidValue;
    const bool cl = c.mode == SSE_MODE_LDS_EDGES;
    if (!cl && c.mode != SSE_MODE_GENERAL) return hipErrorInvalidValue;
    switch (c.W) {
    case 4: return cl ? launch_main_one<4, true>(c, B, A) : launch_main_one<4, false>(c, B, A);
    case 8: return cl ? launch_main_one<8, true>(c, B, A) : launch_main_one<8, false>(c, B, A);
    case 16: return cl ? launch_main_one<16, true>(c, B, A) : launch_main_one<16, false>(c, B, A);
    default: return hipErrorInvalidValue;
    }
}
} // namespace sse
