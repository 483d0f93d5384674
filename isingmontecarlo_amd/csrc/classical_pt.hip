// classical_pt.hip — the C ABI of classical parallel tempering (include/isingmc_hip.h, isingmc_classical_pt_*): attach, the run of
// rounds (steps launch, tempering launch) without a host synchronisation in between, the checkpoint accessors, and the same rounds by
// the sequential rule on the CPU (isingmc_classical_host_pt_run).  The rule is classical_pt_rule.h.  The overlaps between copies of a
// realisation (isingmc_classical_overlap_*, classical_overlap_rule.h) are measured inside those rounds, so they live here as well: one
// round loop on the device and one on the host, with and without the measurement.  The cluster moves between those copies
// (isingmc_classical_icm_*, classical_icm_rule.h) are a third launch of the same rounds, so they live here too.
#include "classical_handle.h"
#include "classical_icm_rule.h"
#include "classical_overlap_rule.h"
#include "classical_pt_rule.h"

#include <cmath>

using namespace sse;

// what attach and the host entry ask of a ladder: every error is reachable without a device
static int check_pt_args(uint32_t R, uint32_t replica_offset, uint32_t ntemps, const double *betas, std::string &why) {
    if (ntemps < 2u) { why = "tempering needs ntemps >= 2"; return ISINGMC_EINVAL; }
    if (R % ntemps != 0u) { why = "nreplicas must be a multiple of ntemps (a batch is whole chains)"; return ISINGMC_EINVAL; }
    if (replica_offset % ntemps != 0u) { why = "replica_offset must be a multiple of ntemps (a chain does not straddle batches)"; return ISINGMC_EINVAL; }
    if (!betas) { why = "the ladder (betas) must be non-null"; return ISINGMC_EINVAL; }
    for (uint32_t t = 0; t < ntemps; ++t)
        if (!std::isfinite(betas[t])) { why = "every beta of the ladder must be finite"; return ISINGMC_EINVAL; }
    return ISINGMC_OK;
}

// The swap rule compares energies of one Hamiltonian: with per-replica couplings the T rows of every chain must be the same
// realisation, bit for bit (chains may differ from each other)
static int check_pt_couplings(const CmcHostTables &H, uint32_t R, uint32_t ntemps, std::string &why) {
    const uint32_t c = H.first_mixed_chain(R, ntemps);
    if (c == CMC_NONE) return ISINGMC_OK;
    why = "tempering needs one set of couplings per chain: the coupling rows of chain " + std::to_string(c) + " (replicas " + std::to_string(c * ntemps) + " .. " +
          std::to_string(c * ntemps + ntemps - 1u) + ") differ; tempering between different graphs is not built";
    return ISINGMC_EINVAL;
}

// The batch as groups of copies (classical_overlap_rule.h): what overlap_attach and the host entry ask, and the sizes that follow
static const char *const kNeedCopies = "overlaps need ncopies >= 2 (copies of one realisation are compared in pairs)";
struct CmcOvShape {
    uint32_t K, G, P;
    uint64_t items;            // G P T
    size_t hq_count, hl_count; // entries of the histograms
};
static int check_overlap_args(const CmcHostTables &H, uint32_t R, uint32_t replica_offset, uint32_t T, uint32_t K, CmcOvShape &S, std::string &why) {
    if (K < 2u) { why = kNeedCopies; return ISINGMC_EINVAL; }
    const uint32_t C = R / T;
    if (C % K != 0u) { why = "the number of chains (nreplicas / ntemps) must be a multiple of ncopies (a batch is whole groups)"; return ISINGMC_EINVAL; }
    if ((replica_offset / T) % K != 0u) { why = "replica_offset / ntemps must be a multiple of ncopies (a group does not straddle batches)"; return ISINGMC_EINVAL; }
    // a chain's rows are equal already: the K chains of a group are copies when its K T rows are
    const uint32_t grp = H.first_mixed_chain(R, K * T);
    if (grp != CMC_NONE) {
        why = "overlaps compare copies of one realisation: the coupling rows of group " + std::to_string(grp) + " (replicas " + std::to_string((uint64_t)grp * K * T) +
              " .. " + std::to_string((uint64_t)grp * K * T + (uint64_t)K * T - 1u) + ") differ";
        return ISINGMC_EINVAL;
    }
    S.K = K; S.G = C / K;
    S.items = (uint64_t)S.G * cmc_ov_pairs(K) * T;
    if (S.items > CMC_OV_MAX_ITEMS) { why = "too many overlaps to measure: groups x pairs x temperatures exceeds 2^31"; return ISINGMC_EINVAL; }
    S.P = (uint32_t)cmc_ov_pairs(K);
    const size_t most = SIZE_MAX / 8u / (size_t)S.items;
    if ((size_t)H.N + 1u > most || (size_t)H.E + 1u > most) { why = "the overlap histograms of this batch do not fit a size_t"; return ISINGMC_EINVAL; }
    S.hq_count = (size_t)S.items * ((size_t)H.N + 1u);
    S.hl_count = (size_t)S.items * ((size_t)H.E + 1u);
    return ISINGMC_OK;
}

// (frees the histograms; the cluster moves pair the copies of the overlaps, so they go with them, and their counts are freed too)
static void detach_overlaps(isingmc_classical *g) { g->ov = CmcOvHandle{}; g->icm = CmcIcmHandle{}; }

// The window of cluster moves (classical_icm_rule.h): what icm_attach and the host entry ask.  t_last = 0 means T.
static int check_icm_window(uint32_t T, uint32_t &t_first, uint32_t &t_last, std::string &why) {
    if (t_last == 0u) t_last = T;
    if (t_last > T) { why = "cluster moves: t_last = " + std::to_string(t_last) + " exceeds the " + std::to_string(T) + " temperatures of the ladder"; return ISINGMC_EINVAL; }
    if (t_first >= t_last) { why = "cluster moves need a window t_first < t_last: [" + std::to_string(t_first) + ", " + std::to_string(t_last) + ") is empty or reversed"; return ISINGMC_EINVAL; }
    return ISINGMC_OK;
}
// the refusal of a model whose bit sets exceed LDS
static std::string icm_too_large(size_t total_words, uint32_t lds_bytes) {
    return "model too large for cluster moves: the three bit sets of one item exceed LDS (at most " + std::to_string(cmc_icm_max_vars(total_words)) + " variables in " +
           std::to_string(lds_bytes) + " bytes)";
}

static int need_icm(isingmc_classical *g, const char *who) {
    if (g->icm.attached) return ISINGMC_OK;
    g->err = std::string(who) + ": call isingmc_classical_icm_attach first";
    return ISINGMC_EINVAL;
}

static int need_overlaps(isingmc_classical *g, const char *who) {
    if (g->ov.attached) return ISINGMC_OK;
    g->err = std::string(who) + ": call isingmc_classical_overlap_attach first";
    return ISINGMC_EINVAL;
}

static int need_attached(isingmc_classical *g, const char *who) {
    if (g->pt.attached) return ISINGMC_OK;
    g->err = std::string(who) + ": call isingmc_classical_pt_attach first";
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

struct CmcBytes { // a state as bytes, read only
    const uint8_t *s;
    bool get(uint32_t v) const { return s[v] != 0; }
};

// rounds x (steps launch, [overlap launch,] [cluster-move launch,] tempering launch) enqueued back to back, one synchronisation at the
// end: the loop of isingmc_classical_pt_run, isingmc_classical_pt_run_overlaps and isingmc_classical_pt_run_icm.  measure: the overlap
// launch runs (the handle has overlaps attached); icm: the cluster-move launch runs behind it (the handle has cluster moves attached)
static int run_rounds(isingmc_classical *g, bool measure, bool icm, uint64_t rounds, uint64_t steps, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds,
                      double *energy_out, int32_t *mag_out, int32_t *q_out, int32_t *ql_out) {
    if (kinds >= CMC_KINDS_COUNT) { g->err = "kinds must be one of ISINGMC_CLASSICAL_KINDS_*"; return ISINGMC_EINVAL; }
    if (rounds == 0) return ISINGMC_OK;
    const size_t R = g->dev.R, items = measure ? (size_t)g->ov.dev.G * g->ov.dev.P * g->pt.dev.T : 0u;
    if ((energy_out || mag_out || q_out || ql_out) && rounds > (SIZE_MAX / 16u) / std::max(R, items)) { g->err = "the recorded series of this many rounds does not fit"; return ISINGMC_EINVAL; }
    HIP_TRY(g, hipSetDevice(g->device));
    struct Series { void *host; DevBuf dev; size_t row; }; // a recorded series: its rows are `row` bytes a round (per call: freed on every way out)
    Series series[4] = {{energy_out, {}, R * 8}, {mag_out, {}, R * 4}, {q_out, {}, items * 4}, {ql_out, {}, items * 4}};
    for (Series &x : series)
        if (x.host && x.dev.alloc((size_t)rounds * x.row) != hipSuccess) {
            g->err = "hipMalloc of a recorded series failed (" + std::to_string((size_t)rounds * x.row) + " bytes)";
            return ISINGMC_ENODEVICE;
        }
    auto row = [&](int k, uint64_t i) { return series[k].dev ? series[k].dev.as<char>() + i * series[k].row : nullptr; };
    const CmcStepArgs A{steps, g->pt.dev.beta_slot, nspin, nedge, nworm, kinds, (g->flags & ISINGMC_CLASSICAL_CFG_SERIAL_MOVES) ? 1u : 0u};
    hipError_t e = hipEventRecord(g->ev0, g->stream);
    for (uint64_t i = 0; i < rounds && e == hipSuccess; ++i) { // enqueued back to back: the tempering launch leaves the next steps launch its betas
        if (steps) e = launch_classical_steps(g->stream, g->dev, g->carve, A);
        if (e == hipSuccess && measure) // after the steps, before the swaps: the maps still say where every temperature is
            e = launch_classical_overlaps(g->stream, g->dev, g->pt.dev, g->ov.dev, reinterpret_cast<int32_t *>(row(2, i)), reinterpret_cast<int32_t *>(row(3, i)));
        if (e == hipSuccess && icm) // the tempering launch computes E and M from the states the moves leave
            e = launch_classical_icm(g->stream, g->dev, g->pt.dev, g->ov.dev, g->icm.dev, g->pt.step);
        if (e == hipSuccess) e = launch_classical_tempering(g->stream, g->dev, g->pt.dev, g->pt.step, reinterpret_cast<double *>(row(0, i)), reinterpret_cast<int32_t *>(row(1, i)));
        if (e == hipSuccess) g->pt.step++;
    }
    if (e == hipSuccess) e = hipEventRecord(g->ev1, g->stream);
    if (e == hipSuccess) { g->timed = true; e = hipStreamSynchronize(g->stream); }
    for (Series &x : series)
        if (e == hipSuccess && x.dev) e = hipMemcpy(x.host, x.dev.as<void>(), (size_t)rounds * x.row, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { g->err = std::string("classical tempering run: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    return ISINGMC_OK;
}

extern "C" {

int isingmc_classical_pt_attach(isingmc_classical *g, uint32_t ntemps, const double *betas) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = check_pt_args(g->dev.R, g->dev.replica_offset, ntemps, betas, g->err)) return rc;
    if (const int rc = check_pt_couplings(g->host, g->dev.R, ntemps, g->err)) return rc;
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
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
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_run")) return rc;
    return run_rounds(g, false, false, rounds, steps, nspin, nedge, nworm, kinds, energy_out, mag_out, nullptr, nullptr);
}

int isingmc_classical_pt_run_overlaps(isingmc_classical *g, uint64_t rounds, uint64_t steps, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds,
                                      double *energy_out, int32_t *mag_out, int32_t *q_out, int32_t *ql_out) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_run_overlaps")) return rc;
    if (const int rc = need_overlaps(g, "isingmc_classical_pt_run_overlaps")) return rc;
    return run_rounds(g, true, false, rounds, steps, nspin, nedge, nworm, kinds, energy_out, mag_out, q_out, ql_out);
}

int isingmc_classical_overlap_attach(isingmc_classical *g, uint32_t ncopies) {
    if (!g) return ISINGMC_EINVAL;
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    if (ncopies == 0u) { detach_overlaps(g); return ISINGMC_OK; }
    if (const int rc = need_attached(g, "isingmc_classical_overlap_attach")) return rc;
    CmcOvShape S{};
    if (const int rc = check_overlap_args(g->host, g->dev.R, g->dev.replica_offset, g->pt.dev.T, ncopies, S, g->err)) return rc;
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
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_overlaps(g, "isingmc_classical_overlap_histograms")) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    if (hq) if (const int rc = copy_down(g, hq, g->ov.dev.hq, g->ov.hq_count)) return rc;
    return hl ? copy_down(g, hl, g->ov.dev.hl, g->ov.hl_count) : ISINGMC_OK;
}

int isingmc_classical_overlap_set_histograms(isingmc_classical *g, const uint64_t *hq, const uint64_t *hl) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_overlaps(g, "isingmc_classical_overlap_set_histograms")) return rc;
    if (!hq || !hl) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    if (const int rc = copy_up(g, g->ov.dev.hq, hq, g->ov.hq_count, true)) return rc;
    return copy_up(g, g->ov.dev.hl, hl, g->ov.hl_count);
}

int isingmc_classical_overlap_reset(isingmc_classical *g) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_overlaps(g, "isingmc_classical_overlap_reset")) return rc;
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    HIP_TRY(g, hipMemset(g->ov.dev.hq, 0, g->ov.hq_count * 8u));
    HIP_TRY(g, hipMemset(g->ov.dev.hl, 0, g->ov.hl_count * 8u));
    return ISINGMC_OK;
}

int isingmc_classical_icm_plan(uint32_t nvars, uint32_t lds_bytes, uint32_t out[4]) {
    if (!out) return cmc_refuse(ISINGMC_EINVAL, "null output");
    if (nvars == 0u || nvars > CMC_MAX_VARS) return cmc_refuse(ISINGMC_EINVAL, "nvars must be 1 .. 2^24");
    const CmcIcmCarve c = cmc_icm_plan(nvars, lds_bytes / 4u);
    if (c.W == 0u) return cmc_refuse(ISINGMC_ENOTIMPL, icm_too_large(lds_bytes / 4u, lds_bytes));
    out[0] = c.W; out[1] = c.words; out[2] = c.wave_words; out[3] = cmc_icm_max_vars(lds_bytes / 4u);
    return ISINGMC_OK;
}

int isingmc_classical_icm_launch_plan(isingmc_classical *g, uint32_t out[4]) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_icm(g, "isingmc_classical_icm_launch_plan")) return rc;
    if (!out) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    const CmcIcmCarve &c = g->icm.dev.C;
    out[0] = c.W; out[1] = c.words; out[2] = c.wave_words; out[3] = cmc_icm_max_vars(g->lds_bytes / 4u);
    return ISINGMC_OK;
}

int isingmc_classical_icm_attach(isingmc_classical *g, uint32_t t_first, uint32_t t_last) {
    if (!g) return ISINGMC_EINVAL;
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    if (t_first == CMC_NONE && t_last == CMC_NONE) { g->icm = CmcIcmHandle{}; return ISINGMC_OK; }
    if (const int rc = need_attached(g, "isingmc_classical_icm_attach")) return rc;
    if (const int rc = need_overlaps(g, "isingmc_classical_icm_attach")) return rc;
    if (const int rc = check_icm_window(g->pt.dev.T, t_first, t_last, g->err)) return rc;
    const CmcIcmCarve c = cmc_icm_plan(g->host.N, g->lds_bytes / 4u);
    if (c.W == 0u) { g->err = icm_too_large(g->lds_bytes / 4u, g->lds_bytes); return ISINGMC_ENOTIMPL; }
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
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_icm(g, "isingmc_classical_icm_force_waves")) return rc;
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
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
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_run_icm")) return rc;
    if (const int rc = need_overlaps(g, "isingmc_classical_pt_run_icm")) return rc;
    if (const int rc = need_icm(g, "isingmc_classical_pt_run_icm")) return rc;
    return run_rounds(g, measure != 0u, true, rounds, steps, nspin, nedge, nworm, kinds, energy_out, mag_out, measure ? q_out : nullptr, measure ? ql_out : nullptr);
}

int isingmc_classical_icm_window(isingmc_classical *g, uint32_t *t_first, uint32_t *t_last) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_icm(g, "isingmc_classical_icm_window")) return rc;
    if (t_first) *t_first = g->icm.dev.t_first;
    if (t_last) *t_last = g->icm.dev.t_last;
    return ISINGMC_OK;
}

int isingmc_classical_icm_counts(isingmc_classical *g, uint64_t *moves, uint64_t *empty, uint64_t *size_sum) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_icm(g, "isingmc_classical_icm_counts")) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    if (moves) if (const int rc = copy_down(g, moves, g->icm.dev.moves, g->icm.count)) return rc;
    if (empty) if (const int rc = copy_down(g, empty, g->icm.dev.empty, g->icm.count)) return rc;
    return size_sum ? copy_down(g, size_sum, g->icm.dev.size_sum, g->icm.count) : ISINGMC_OK;
}

int isingmc_classical_icm_set_counts(isingmc_classical *g, const uint64_t *moves, const uint64_t *empty, const uint64_t *size_sum) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_icm(g, "isingmc_classical_icm_set_counts")) return rc;
    if (!moves || !empty || !size_sum) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    if (const int rc = copy_up(g, g->icm.dev.moves, moves, g->icm.count, true)) return rc;
    if (const int rc = copy_up(g, g->icm.dev.empty, empty, g->icm.count)) return rc;
    return copy_up(g, g->icm.dev.size_sum, size_sum, g->icm.count);
}

int isingmc_classical_icm_reset(isingmc_classical *g) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_icm(g, "isingmc_classical_icm_reset")) return rc;
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    HIP_TRY(g, hipMemset(g->icm.counts.as<void>(), 0, 3u * g->icm.count * 8u));
    return ISINGMC_OK;
}

int isingmc_classical_pt_get(isingmc_classical *g, uint32_t *temp_of, uint64_t *pt_step) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_get")) return rc;
    if (const int rc = temp_of ? copy_down(g, temp_of, g->pt.dev.temp_of, g->dev.R, true) : isingmc_classical_synchronize(g)) return rc;
    if (pt_step) *pt_step = g->pt.step;
    return ISINGMC_OK;
}

int isingmc_classical_pt_set(isingmc_classical *g, const uint32_t *temp_of, uint64_t pt_step) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_set")) return rc;
    if (!temp_of) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    std::vector<uint8_t> seen(g->pt.dev.T);
    if (!cmc_pt_is_permutation(temp_of, g->dev.R, g->pt.dev.T, seen.data())) {
        g->err = "temp_of must be a permutation of the temperatures within every chain";
        return ISINGMC_EINVAL;
    }
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    if (const int rc = upload_maps(g, temp_of)) return rc;
    g->pt.step = pt_step;
    return ISINGMC_OK;
}

int isingmc_classical_pt_swap_counts(isingmc_classical *g, uint64_t *attempts, uint64_t *accepts) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_swap_counts")) return rc;
    if (const int rc = isingmc_classical_synchronize(g)) return rc;
    const size_t pairs = (size_t)g->pt.dev.C * (g->pt.dev.T - 1u);
    if (attempts) if (const int rc = copy_down(g, attempts, g->pt.dev.attempts, pairs)) return rc;
    return accepts ? copy_down(g, accepts, g->pt.dev.accepts, pairs) : ISINGMC_OK;
}

int isingmc_classical_pt_set_swap_counts(isingmc_classical *g, const uint64_t *attempts, const uint64_t *accepts) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_set_swap_counts")) return rc;
    if (!attempts || !accepts) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    const size_t pairs = (size_t)g->pt.dev.C * (g->pt.dev.T - 1u);
    if (const int rc = copy_up(g, g->pt.dev.attempts, attempts, pairs, true)) return rc;
    return copy_up(g, g->pt.dev.accepts, accepts, pairs);
}

} // extern "C"

// the cluster moves of the host rounds: the window and the three counts (each may be null)
struct CmcIcmHostArgs {
    uint32_t t_first, t_last;
    uint64_t *moves, *empty, *size_sum;
};

// The cluster of the rank-th differing variable of the states a and b ([N] bytes) into mark ([N], zeroed on entry); diff and stack
// are [N] scratch.  Returns its size, or 0 when fewer than rank + 1 variables differ.
static uint32_t host_cluster(const CmcGraphMem &g, const uint8_t *a, const uint8_t *b, bool draw, const uint32_t c[4], uint64_t seed, uint32_t rank, uint8_t *diff,
                             uint8_t *mark, uint32_t *stack) {
    uint32_t nq = 0;
    for (uint32_t v = 0; v < g.N(); ++v) { diff[v] = (a[v] != 0) != (b[v] != 0) ? 1u : 0u; nq += diff[v]; }
    if (draw && nq) rank = cmc_range(CmcHostDraw{(uint32_t)seed, (uint32_t)(seed >> 32), c[2], c[1], c[3] & 0xFFFFFFu}(c[3] >> 24, c[0], 0), nq);
    return rank < nq ? cmc_icm_grow(g, diff, rank, mark, stack) : 0u;
}

// The rounds of isingmc_classical_host_pt_run, isingmc_classical_host_pt_run_overlaps and isingmc_classical_host_pt_run_icm: ncopies = 0
// has no groups; measure: the overlaps are measured; icm: the cluster moves run (null: none)
static int host_rounds(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint32_t ncopies, bool measure, const CmcIcmHostArgs *icm_in,
                       uint64_t rounds, uint64_t steps,
                       uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                       uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out,
                       int32_t *q_out, int32_t *ql_out, uint64_t *hq, uint64_t *hl) {
    if (const int rc = cmc_check_config(cfg)) return rc;
    std::string why;
    if (const int rc = check_pt_args(cfg->nreplicas, cfg->replica_offset, ntemps, betas, why)) return cmc_refuse(rc, why);
    if (!states || !epochs || !temp_of || !pt_step) return cmc_refuse(ISINGMC_EINVAL, "states, epochs, temp_of and pt_step must be non-null");
    if (kinds >= CMC_KINDS_COUNT) return cmc_refuse(ISINGMC_EINVAL, "kinds must be one of ISINGMC_CLASSICAL_KINDS_*");
    const uint32_t R = cfg->nreplicas, T = ntemps, C = R / T;
    std::vector<uint8_t> seen(T);
    if (!cmc_pt_is_permutation(temp_of, R, T, seen.data())) return cmc_refuse(ISINGMC_EINVAL, "temp_of must be a permutation of the temperatures within every chain");
    CmcHostTables H;
    cmc_build_tables(cfg, H);
    if (const int rc = check_pt_couplings(H, R, T, why)) return cmc_refuse(rc, why);
    CmcOvShape ov{};
    if (ncopies != 0u)
        if (const int rc = check_overlap_args(H, R, cfg->replica_offset, T, ncopies, ov, why)) return cmc_refuse(rc, why);
    CmcIcmHostArgs icm{};
    if (icm_in) {
        icm = *icm_in;
        if (ncopies == 0u) return cmc_refuse(ISINGMC_EINVAL, "cluster moves need ncopies >= 2 (they exchange clusters between the copies of a group)");
        if (const int rc = check_icm_window(T, icm.t_first, icm.t_last, why)) return cmc_refuse(rc, why);
    }
    const uint32_t N = H.N;
    std::vector<uint8_t> diff(icm_in ? N : 0u), cluster(icm_in ? N : 0u, 0);
    std::vector<uint32_t> stack(icm_in ? N : 0u);
    const CmcHostMoves m{cmc_default_moves(nspin, N / 2u), cmc_default_moves(nedge, H.E / 2u), cmc_default_moves(nworm, 1u), kinds};
    std::vector<uint8_t> mark(N, 0);
    std::vector<uint32_t> slot_at(R);
    std::vector<double> energy(R);
    for (uint32_t r = 0; r < R; ++r) slot_at[(r / T) * T + temp_of[r]] = r % T;
    for (uint64_t round = 0; round < rounds; ++round, ++*pt_step) {
        for (uint32_t r = 0; r < R; ++r) {
            uint64_t ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const CmcGraphMem g = cmc_graph_mem(H.view(), r);
            cmc_host_replica_steps(g, cfg->seed, cfg->replica_offset + r, steps, betas[temp_of[r]], m, states + (size_t)r * N, mark.data(), &epochs[r], ctr);
            for (int i = 0; counters && i < 8; ++i) counters[(size_t)r * 8 + i] += ctr[i];
            const CmcBytes s{states + (size_t)r * N};
            energy[r] = cmc_pt_energy(g, s);
            const size_t at = (size_t)round * R + (r / T) * T + temp_of[r];
            if (energy_out) energy_out[at] = energy[r];
            if (mag_out) mag_out[at] = cmc_pt_magnetization(g, s);
        }
        for (uint64_t item = 0; measure && item < ov.items; ++item) { // after the steps, before the swaps (ncopies = 0: no items)
            uint32_t grp, p, t, a, b;
            cmc_ov_item(item, ov.P, T, grp, p, t);
            cmc_ov_pair(ov.K, p, a, b);
            const uint32_t ra = cmc_ov_slot(slot_at.data(), T, grp * ov.K + a, t), rb = cmc_ov_slot(slot_at.data(), T, grp * ov.K + b, t);
            const CmcBytes A{states + (size_t)ra * N}, B{states + (size_t)rb * N};
            const uint32_t nq = cmc_ov_count_spins(N, A, B, 0u, 1u), nl = cmc_ov_count_links(cmc_graph_mem(H.view(), ra), A, B, 0u, 1u);
            if (q_out) q_out[(size_t)round * ov.items + item] = cmc_ov_overlap(N, nq);
            if (ql_out) ql_out[(size_t)round * ov.items + item] = cmc_ov_overlap(H.E, nl);
            if (hq) hq[(size_t)item * ((size_t)N + 1u) + nq] += 1u;
            if (hl) hl[(size_t)item * ((size_t)H.E + 1u) + nl] += 1u;
        }
        const uint32_t M = cmc_icm_pairs(ov.K);
        for (uint64_t item = 0, items = icm_in ? (uint64_t)ov.G * M * (icm.t_last - icm.t_first) : 0u; item < items; ++item) { // behind the measurement
            uint32_t grp, p, t, a, b, ctr[4];
            cmc_icm_item(item, M, icm.t_first, icm.t_last, grp, p, t);
            cmc_icm_pair(ov.K, *pt_step, p, a, b);
            const uint32_t ra = cmc_ov_slot(slot_at.data(), T, grp * ov.K + a, t), rb = cmc_ov_slot(slot_at.data(), T, grp * ov.K + b, t);
            uint8_t *A = states + (size_t)ra * N, *B = states + (size_t)rb * N;
            cmc_icm_counter(T, *pt_step, (cfg->replica_offset / T + grp * ov.K) / ov.K, p, t, ctr);
            const uint32_t size = host_cluster(cmc_graph_mem(H.view(), ra), A, B, true, ctr, cfg->seed, 0u, diff.data(), cluster.data(), stack.data());
            const size_t at = cmc_icm_count_index(M, T, grp, p, t);
            if (size == 0u) { if (icm.empty) icm.empty[at] += 1u; continue; }
            if (icm.moves) icm.moves[at] += 1u;
            if (icm.size_sum) icm.size_sum[at] += size;
            for (uint32_t v = 0; v < N; ++v)
                if (cluster[v]) { A[v] = A[v] ? 0u : 1u; B[v] = B[v] ? 0u : 1u; cluster[v] = 0u; }
            for (const uint32_t r : {ra, rb}) { // E and M of the round are those the swaps see: after the moves
                const CmcGraphMem g = cmc_graph_mem(H.view(), r);
                const CmcBytes s{states + (size_t)r * N};
                energy[r] = cmc_pt_energy(g, s);
                const size_t row = (size_t)round * R + (r / T) * T + temp_of[r];
                if (energy_out) energy_out[row] = energy[r];
                if (mag_out) mag_out[row] = cmc_pt_magnetization(g, s);
            }
        }
        for (uint32_t c = 0; c < C; ++c) {
            const size_t base = (size_t)c * T, cbase = (size_t)c * (T - 1u);
            const CmcPtChainView cv{T, betas, temp_of + base, slot_at.data() + base, energy.data() + base, attempts ? attempts + cbase : nullptr,
                                    accepts ? accepts + cbase : nullptr};
            cmc_pt_chain_step(cfg->seed, *pt_step, cfg->replica_offset / T + c, cv, PtHostDraw{});
        }
    }
    return ISINGMC_OK;
}

extern "C" {

int isingmc_classical_host_pt_run(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint64_t rounds, uint64_t steps,
                                  uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                                  uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out) {
    return host_rounds(cfg, ntemps, betas, 0u, false, nullptr, rounds, steps, nspin, nedge, nworm, kinds, states, epochs, temp_of, pt_step, counters, attempts, accepts, energy_out, mag_out,
                       nullptr, nullptr, nullptr, nullptr);
}

int isingmc_classical_host_pt_run_overlaps(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint32_t ncopies, uint64_t rounds, uint64_t steps,
                                           uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                                           uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out,
                                           int32_t *q_out, int32_t *ql_out, uint64_t *hq, uint64_t *hl) {
    if (const int rc = cmc_check_config(cfg)) return rc;
    if (ncopies == 0u) return cmc_refuse(ISINGMC_EINVAL, kNeedCopies);
    return host_rounds(cfg, ntemps, betas, ncopies, true, nullptr, rounds, steps, nspin, nedge, nworm, kinds, states, epochs, temp_of, pt_step, counters, attempts, accepts, energy_out,
                       mag_out, q_out, ql_out, hq, hl);
}

int isingmc_classical_host_pt_run_icm(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint32_t ncopies, uint64_t rounds, uint64_t steps,
                                      uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                                      uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out,
                                      int32_t *q_out, int32_t *ql_out, uint64_t *hq, uint64_t *hl, uint32_t measure, uint32_t t_first, uint32_t t_last,
                                      uint64_t *moves, uint64_t *empty, uint64_t *size_sum) {
    if (const int rc = cmc_check_config(cfg)) return rc;
    const CmcIcmHostArgs icm{t_first, t_last, moves, empty, size_sum};
    return host_rounds(cfg, ntemps, betas, ncopies, measure != 0u, &icm, rounds, steps, nspin, nedge, nworm, kinds, states, epochs, temp_of, pt_step, counters, attempts,
                       accepts, energy_out, mag_out, q_out, ql_out, hq, hl);
}

int isingmc_classical_host_icm_cluster(const isingmc_classical_config *cfg, const uint8_t *state_a, const uint8_t *state_b, uint32_t rank, uint8_t *mask_out,
                                       uint32_t *size_out) {
    if (const int rc = cmc_check_config(cfg)) return rc;
    if (!state_a || !state_b || !mask_out) return cmc_refuse(ISINGMC_EINVAL, "state_a, state_b and mask_out must be non-null");
    CmcHostTables H;
    cmc_build_tables(cfg, H);
    std::vector<uint8_t> diff(H.N);
    std::vector<uint32_t> stack(H.N);
    std::fill(mask_out, mask_out + H.N, (uint8_t)0);
    const uint32_t none[4] = {0, 0, 0, 0};
    const uint32_t size = host_cluster(cmc_graph_mem(H.view(), 0u), state_a, state_b, false, none, 0u, rank, diff.data(), mask_out, stack.data());
    if (size == 0u) return cmc_refuse(ISINGMC_EINVAL, "rank must be below the number of variables in which the two states differ");
    if (size_out) *size_out = size;
    return ISINGMC_OK;
}

} // extern "C"
