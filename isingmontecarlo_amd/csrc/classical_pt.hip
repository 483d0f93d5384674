// classical_pt.hip — what is attached to a handle of classical Monte Carlo, in the C ABI (include/isingmc_hip.h): parallel tempering
// (isingmc_classical_pt_*, classical_pt_rule.h), the overlaps between copies of a realisation (isingmc_classical_overlap_*,
// classical_overlap_rule.h) and the cluster moves between those copies (isingmc_classical_icm_*, classical_icm_rule.h): the three
// attach calls, their checkpoint accessors, and the one round loop on the device that all three run in (steps launch, overlap launch,
// cluster-move launch, tempering launch) without a host synchronisation in between.  The argument checks are shared with the same
// rounds by the sequential rule on the CPU, which live in the device-free unit (classical_host.hip).
#include "classical_handle.h"
#include "classical_icm_rule.h"
#include "classical_overlap_rule.h"
#include "classical_pt_rule.h"

using namespace sse;

// (frees the histograms; the cluster moves pair the copies of the overlaps, so they go with them, and their counts are freed too)
static void detach_overlaps(isingmc_classical *g) { g->ov = CmcOvHandle{}; g->icm = CmcIcmHandle{}; }

// The refusal of entry `who`: on a null handle, or when what it needs attached first is not: tempering (g->pt), the overlaps (g->ov) or
// the cluster moves (g->icm)
enum CmcAttachment { CMC_NEED_PT, CMC_NEED_OV, CMC_NEED_ICM };
static int need(isingmc_classical *g, CmcAttachment what, const char *who) {
    if (!g) return ISINGMC_EINVAL;
    static const char *const attach_call[3] = {"isingmc_classical_pt_attach", "isingmc_classical_overlap_attach", "isingmc_classical_icm_attach"};
    if (what == CMC_NEED_PT ? g->pt.attached : what == CMC_NEED_OV ? g->ov.attached : g->icm.attached) return ISINGMC_OK;
    g->err = std::string(who) + ": call " + attach_call[what] + " first";
    return ISINGMC_EINVAL;
}

// temp_of [R] -> the device maps and the per-slot betas
static int upload_maps(isingmc_classical *g, const uint32_t *temp_of) {
    const uint32_t R = g->dev.R, T = g->pt.dev.T;
    std::vector<uint32_t> slot_at(R);
    std::vector<double> beta_slot(R);
    for (uint32_t r = 0; r < R; ++r) {
        slot_at[(r / T) * T + temp_of[r]] = r % T;
        beta_slot[r] = g->pt.betas[temp_of[r]];
    }
    if (const int rc = copy_up(g, g->pt.dev.temp_of, temp_of, R)) return rc;
    if (const int rc = copy_up(g, g->pt.dev.slot_at, slot_at.data(), R)) return rc;
    return copy_up(g, g->pt.dev.beta_slot, beta_slot.data(), R);
}

// rounds x (steps launch, [overlap launch,] [cluster-move launch,] tempering launch) enqueued back to back, one synchronisation at the
// end: the loop of isingmc_classical_pt_run, isingmc_classical_pt_run_overlaps and isingmc_classical_pt_run_icm.  a.overlaps: the overlap
// launch runs (the handle has overlaps attached); a.cluster_moves: the cluster-move launch runs behind it (... has cluster moves attached)
static int run_rounds(isingmc_classical *g, const CmcRounds &a) {
    if (a.kinds >= CMC_KINDS_COUNT) { g->err = "kinds must be one of ISINGMC_CLASSICAL_KINDS_*"; return ISINGMC_EINVAL; }
    if (a.rounds == 0) return ISINGMC_OK;
    const size_t R = g->dev.R, items = a.overlaps ? (size_t)g->ov.dev.G * g->ov.dev.P * g->pt.dev.T : 0u;
    if ((a.energy_out || a.mag_out || a.q_out || a.ql_out) && a.rounds > (SIZE_MAX / 16u) / std::max(R, items)) { g->err = "the recorded series of this many rounds does not fit"; return ISINGMC_EINVAL; }
    HIP_TRY(g, hipSetDevice(g->device));
    struct Series { void *host; DevBuf dev; size_t row; }; // a recorded series: its rows are `row` bytes a round (per call: freed on every way out)
    Series series[4] = {{a.energy_out, {}, R * 8}, {a.mag_out, {}, R * 4}, {a.q_out, {}, items * 4}, {a.ql_out, {}, items * 4}};
    for (Series &x : series)
        if (x.host && x.dev.alloc((size_t)a.rounds * x.row) != hipSuccess) {
            g->err = "hipMalloc of a recorded series failed (" + std::to_string((size_t)a.rounds * x.row) + " bytes)";
            return ISINGMC_ENODEVICE;
        }
    auto row = [&](int k, uint64_t i) { return series[k].dev ? series[k].dev.as<char>() + i * series[k].row : nullptr; };
    const CmcStepArgs A{a.steps, g->pt.dev.beta_slot, a.nspin, a.nedge, a.nworm, a.kinds, (g->flags & ISINGMC_CLASSICAL_CFG_SERIAL_MOVES) ? 1u : 0u};
    hipError_t e = hipEventRecord(g->ev0, g->stream);
    for (uint64_t i = 0; i < a.rounds && e == hipSuccess; ++i) { // enqueued back to back: the tempering launch leaves the next steps launch its betas
        if (a.steps) e = launch_classical_steps(g->stream, g->dev, g->carve, A);
        if (e == hipSuccess && a.overlaps) // after the steps, before the swaps: the maps still say where every temperature is
            e = launch_classical_overlaps(g->stream, g->dev, g->pt.dev, g->ov.dev, reinterpret_cast<int32_t *>(row(2, i)), reinterpret_cast<int32_t *>(row(3, i)));
        if (e == hipSuccess && a.cluster_moves) // the tempering launch computes E and M from the states the moves leave
            e = launch_classical_icm(g->stream, g->dev, g->pt.dev, g->ov.dev, g->icm.dev, g->pt.step);
        if (e == hipSuccess) e = launch_classical_tempering(g->stream, g->dev, g->pt.dev, g->pt.step, reinterpret_cast<double *>(row(0, i)), reinterpret_cast<int32_t *>(row(1, i)));
        if (e == hipSuccess) g->pt.step++;
    }
    if (e == hipSuccess) e = hipEventRecord(g->ev1, g->stream);
    if (e == hipSuccess) { g->timed = true; e = hipStreamSynchronize(g->stream); }
    for (Series &x : series)
        if (e == hipSuccess && x.dev) e = hipMemcpy(x.host, x.dev.as<void>(), (size_t)a.rounds * x.row, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { g->err = std::string("classical tempering run: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    return ISINGMC_OK;
}

extern "C" {

int isingmc_classical_pt_attach(isingmc_classical *g, uint32_t ntemps, const double *betas) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = cmc_check_pt_args(g->dev.R, g->dev.replica_offset, ntemps, betas, g->err)) return rc;
    if (const int rc = cmc_check_pt_couplings(g->host, g->dev.R, ntemps, g->err)) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    const uint32_t R = g->dev.R;
    CmcPtHandle &P = g->pt;
    if (!P.dev.temp_of) { // once: R entries hold any ladder of this batch
        if (const int rc = cmc_alloc(g, &P.dev.temp_of, R)) return rc;
        if (const int rc = cmc_alloc(g, &P.dev.slot_at, R)) return rc;
        if (const int rc = cmc_alloc(g, &P.dev.beta_slot, R)) return rc;
        if (const int rc = cmc_alloc(g, &P.dev.energy, R)) return rc;
        if (const int rc = cmc_alloc(g, &P.dev.mag, R)) return rc;
        if (const int rc = cmc_alloc(g, &P.dev.attempts, R)) return rc;
        if (const int rc = cmc_alloc(g, &P.dev.accepts, R)) return rc;
        if (const int rc = cmc_alloc(g, &P.d_betas, R)) return rc;
        P.dev.betas = P.d_betas;
    }
    P.attached = false;
    detach_overlaps(g); // the shape of the batch changes: groups, histograms and cluster moves belong to the ladder they were attached under
    P.dev.T = ntemps; P.dev.C = R / ntemps;
    P.betas.assign(betas, betas + ntemps);
    P.step = 0;
    HIP_TRY(g, hipMemcpy(P.d_betas, betas, (size_t)ntemps * 8, hipMemcpyHostToDevice));
    HIP_TRY(g, hipMemset(P.dev.attempts, 0, (size_t)R * 8));
    HIP_TRY(g, hipMemset(P.dev.accepts, 0, (size_t)R * 8));
    std::vector<uint32_t> temp_of(R);
    for (uint32_t r = 0; r < R; ++r) temp_of[r] = r % ntemps;
    if (const int rc = upload_maps(g, temp_of.data())) return rc;
    P.attached = true;
    return ISINGMC_OK;
}

int isingmc_classical_pt_run(isingmc_classical *g, uint64_t rounds, uint64_t steps, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds,
                             double *energy_out, int32_t *mag_out) {
    if (const int rc = need(g, CMC_NEED_PT, "isingmc_classical_pt_run")) return rc;
    return run_rounds(g, CmcRounds{rounds, steps, nspin, nedge, nworm, kinds, energy_out, mag_out});
}

int isingmc_classical_pt_run_overlaps(isingmc_classical *g, uint64_t rounds, uint64_t steps, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds,
                                      double *energy_out, int32_t *mag_out, int32_t *q_out, int32_t *ql_out) {
    if (const int rc = need(g, CMC_NEED_PT, "isingmc_classical_pt_run_overlaps")) return rc;
    if (const int rc = need(g, CMC_NEED_OV, "isingmc_classical_pt_run_overlaps")) return rc;
    CmcRounds a{rounds, steps, nspin, nedge, nworm, kinds, energy_out, mag_out, q_out, ql_out};
    a.overlaps = true;
    return run_rounds(g, a);
}

int isingmc_classical_overlap_attach(isingmc_classical *g, uint32_t ncopies) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    if (ncopies == 0u) { detach_overlaps(g); return ISINGMC_OK; }
    if (const int rc = need(g, CMC_NEED_PT, "isingmc_classical_overlap_attach")) return rc;
    CmcOvShape S{};
    if (const int rc = cmc_check_overlap_args(g->host, g->dev.R, g->dev.replica_offset, g->pt.dev.T, ncopies, S, g->err)) return rc;
    // The old histograms go before the new ones are asked for, on purpose: two sets may not fit where one does.  A failure below
    // therefore leaves the handle without overlaps (and without cluster moves), not with the old ones.
    detach_overlaps(g);
    CmcOvHandle &O = g->ov;
    if (O.hq.alloc(S.hq_count * 8u) != hipSuccess || O.hl.alloc(S.hl_count * 8u) != hipSuccess) {
        detach_overlaps(g);
        g->err = "hipMalloc of the overlap histograms failed (" + std::to_string(S.hq_count * 8u) + " and " + std::to_string(S.hl_count * 8u) + " bytes)";
        return ISINGMC_ENODEVICE;
    }
    O.dev = sse::CmcOvDev{S.K, S.G, S.P, O.hq.as<uint64_t>(), O.hl.as<uint64_t>()};
    O.hq_count = S.hq_count; O.hl_count = S.hl_count;
    HIP_TRY(g, hipMemset(O.dev.hq, 0, S.hq_count * 8u));
    HIP_TRY(g, hipMemset(O.dev.hl, 0, S.hl_count * 8u));
    g->ov.attached = true;
    return ISINGMC_OK;
}

int isingmc_classical_overlap_histograms(isingmc_classical *g, uint64_t *hq, uint64_t *hl) {
    if (const int rc = need(g, CMC_NEED_OV, "isingmc_classical_overlap_histograms")) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    if (hq) if (const int rc = copy_down(g, hq, g->ov.dev.hq, g->ov.hq_count)) return rc;
    return hl ? copy_down(g, hl, g->ov.dev.hl, g->ov.hl_count) : ISINGMC_OK;
}

int isingmc_classical_overlap_set_histograms(isingmc_classical *g, const uint64_t *hq, const uint64_t *hl) {
    if (const int rc = need(g, CMC_NEED_OV, "isingmc_classical_overlap_set_histograms")) return rc;
    if (!hq || !hl) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    if (const int rc = copy_up(g, g->ov.dev.hq, hq, g->ov.hq_count, true)) return rc;
    return copy_up(g, g->ov.dev.hl, hl, g->ov.hl_count);
}

int isingmc_classical_overlap_reset(isingmc_classical *g) {
    if (const int rc = need(g, CMC_NEED_OV, "isingmc_classical_overlap_reset")) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    HIP_TRY(g, hipMemset(g->ov.dev.hq, 0, g->ov.hq_count * 8u));
    HIP_TRY(g, hipMemset(g->ov.dev.hl, 0, g->ov.hl_count * 8u));
    return ISINGMC_OK;
}

int isingmc_classical_icm_launch_plan(isingmc_classical *g, uint32_t out[4]) {
    if (const int rc = need(g, CMC_NEED_ICM, "isingmc_classical_icm_launch_plan")) return rc;
    if (!out) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    cmc_icm_plan_slots(g->icm.dev.C, g->lds_bytes, out);
    return ISINGMC_OK;
}

int isingmc_classical_icm_attach(isingmc_classical *g, uint32_t t_first, uint32_t t_last) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    if (t_first == CMC_NONE && t_last == CMC_NONE) { g->icm = CmcIcmHandle{}; return ISINGMC_OK; }
    if (const int rc = need(g, CMC_NEED_PT, "isingmc_classical_icm_attach")) return rc;
    if (const int rc = need(g, CMC_NEED_OV, "isingmc_classical_icm_attach")) return rc;
    if (const int rc = cmc_check_icm_window(g->pt.dev.T, t_first, t_last, g->err)) return rc;
    const CmcIcmCarve c = cmc_icm_plan(g->host.N, g->lds_bytes / 4u);
    if (c.W == 0u) { g->err = cmc_icm_too_large(g->lds_bytes); return ISINGMC_ENOTIMPL; }
    const uint32_t M = cmc_icm_pairs(g->ov.dev.K);
    const size_t count = (size_t)g->ov.dev.G * M * g->pt.dev.T; // (at most the overlap items: they fit)
    CmcIcmHandle fresh;
    if (fresh.counts.alloc(3u * count * 8u) != hipSuccess) {
        g->err = "hipMalloc of the cluster-move counts failed (" + std::to_string(3u * count * 8u) + " bytes)";
        return ISINGMC_ENODEVICE;
    }
    HIP_TRY(g, hipMemset(fresh.counts.as<void>(), 0, 3u * count * 8u));
    uint64_t *base = fresh.counts.as<uint64_t>();
    fresh.dev = sse::CmcIcmDev{t_first, t_last, M, c, base, base + count, base + 2u * count};
    fresh.count = count;
    fresh.attached = true;
    g->icm = std::move(fresh);
    return ISINGMC_OK;
}

int isingmc_classical_icm_force_waves(isingmc_classical *g, uint32_t waves) {
    if (const int rc = need(g, CMC_NEED_ICM, "isingmc_classical_icm_force_waves")) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    const CmcIcmCarve plan = cmc_icm_plan(g->host.N, g->lds_bytes / 4u);
    if (waves == 0u) { g->icm.dev.C = plan; return ISINGMC_OK; }
    if ((waves != 1u && waves != 2u && waves != 4u) || waves > plan.W) {
        g->err = "cluster moves: waves must be 1, 2 or 4 and at most the " + std::to_string(plan.W) + " that fit LDS (0: as planned)";
        return ISINGMC_EINVAL;
    }
    g->icm.dev.C = cmc_icm_carve(g->host.N, waves);
    return ISINGMC_OK;
}

int isingmc_classical_pt_run_icm(isingmc_classical *g, uint64_t rounds, uint64_t steps, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds,
                                 double *energy_out, int32_t *mag_out, int32_t *q_out, int32_t *ql_out, uint32_t measure) {
    if (const int rc = need(g, CMC_NEED_PT, "isingmc_classical_pt_run_icm")) return rc;
    if (const int rc = need(g, CMC_NEED_OV, "isingmc_classical_pt_run_icm")) return rc;
    if (const int rc = need(g, CMC_NEED_ICM, "isingmc_classical_pt_run_icm")) return rc;
    CmcRounds a{rounds, steps, nspin, nedge, nworm, kinds, energy_out, mag_out, measure ? q_out : nullptr, measure ? ql_out : nullptr};
    a.overlaps = measure != 0u; a.cluster_moves = true;
    return run_rounds(g, a);
}

int isingmc_classical_icm_window(isingmc_classical *g, uint32_t *t_first, uint32_t *t_last) {
    if (const int rc = need(g, CMC_NEED_ICM, "isingmc_classical_icm_window")) return rc;
    if (t_first) *t_first = g->icm.dev.t_first;
    if (t_last) *t_last = g->icm.dev.t_last;
    return ISINGMC_OK;
}

int isingmc_classical_icm_counts(isingmc_classical *g, uint64_t *moves, uint64_t *empty, uint64_t *size_sum) {
    if (const int rc = need(g, CMC_NEED_ICM, "isingmc_classical_icm_counts")) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    if (moves) if (const int rc = copy_down(g, moves, g->icm.dev.moves, g->icm.count)) return rc;
    if (empty) if (const int rc = copy_down(g, empty, g->icm.dev.empty, g->icm.count)) return rc;
    return size_sum ? copy_down(g, size_sum, g->icm.dev.size_sum, g->icm.count) : ISINGMC_OK;
}

int isingmc_classical_icm_set_counts(isingmc_classical *g, const uint64_t *moves, const uint64_t *empty, const uint64_t *size_sum) {
    if (const int rc = need(g, CMC_NEED_ICM, "isingmc_classical_icm_set_counts")) return rc;
    if (!moves || !empty || !size_sum) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    if (const int rc = copy_up(g, g->icm.dev.moves, moves, g->icm.count, true)) return rc;
    if (const int rc = copy_up(g, g->icm.dev.empty, empty, g->icm.count)) return rc;
    return copy_up(g, g->icm.dev.size_sum, size_sum, g->icm.count);
}

int isingmc_classical_icm_reset(isingmc_classical *g) {
    if (const int rc = need(g, CMC_NEED_ICM, "isingmc_classical_icm_reset")) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    HIP_TRY(g, hipMemset(g->icm.counts.as<void>(), 0, 3u * g->icm.count * 8u));
    return ISINGMC_OK;
}

int isingmc_classical_pt_get(isingmc_classical *g, uint32_t *temp_of, uint64_t *pt_step) {
    if (const int rc = need(g, CMC_NEED_PT, "isingmc_classical_pt_get")) return rc;
    if (const int rc = temp_of ? copy_down(g, temp_of, g->pt.dev.temp_of, g->dev.R, true) : isingmc_classical_synchronize(g)) return rc;
    if (pt_step) *pt_step = g->pt.step;
    return ISINGMC_OK;
}

int isingmc_classical_pt_set(isingmc_classical *g, const uint32_t *temp_of, uint64_t pt_step) {
    if (const int rc = need(g, CMC_NEED_PT, "isingmc_classical_pt_set")) return rc;
    if (!temp_of) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    std::vector<uint8_t> seen(g->pt.dev.T);
    if (!cmc_pt_is_permutation(temp_of, g->dev.R, g->pt.dev.T, seen.data())) {
        g->err = "temp_of must be a permutation of the temperatures within every chain";
        return ISINGMC_EINVAL;
    }
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    if (const int rc = upload_maps(g, temp_of)) return rc;
    g->pt.step = pt_step;
    return ISINGMC_OK;
}

int isingmc_classical_pt_swap_counts(isingmc_classical *g, uint64_t *attempts, uint64_t *accepts) {
    if (const int rc = need(g, CMC_NEED_PT, "isingmc_classical_pt_swap_counts")) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    const size_t pairs = (size_t)g->pt.dev.C * (g->pt.dev.T - 1u);
    if (attempts) if (const int rc = copy_down(g, attempts, g->pt.dev.attempts, pairs)) return rc;
    return accepts ? copy_down(g, accepts, g->pt.dev.accepts, pairs) : ISINGMC_OK;
}

int isingmc_classical_pt_set_swap_counts(isingmc_classical *g, const uint64_t *attempts, const uint64_t *accepts) {
    if (const int rc = need(g, CMC_NEED_PT, "isingmc_classical_pt_set_swap_counts")) return rc;
    if (!attempts || !accepts) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    const size_t pairs = (size_t)g->pt.dev.C * (g->pt.dev.T - 1u);
    if (const int rc = copy_up(g, g->pt.dev.attempts, attempts, pairs, true)) return rc;
    return copy_up(g, g->pt.dev.accepts, accepts, pairs);
}

} // extern "C"
