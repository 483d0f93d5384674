// classical_pt.hip — the C ABI of classical parallel tempering (include/isingmc_hip.h, isingmc_classical_pt_*): attach, the run of
// rounds (steps launch, tempering launch) without a host synchronisation in between, the checkpoint accessors, and the same rounds by
// the sequential rule on the CPU (isingmc_classical_host_pt_run).  The rule is classical_pt_rule.h.
#include "classical_handle.h"
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
    CMC_TRY(g, hipMemcpy(g->pt.dev.temp_of, temp_of, (size_t)R * 4, hipMemcpyHostToDevice));
    CMC_TRY(g, hipMemcpy(g->pt.dev.slot_at, slot_at.data(), (size_t)R * 4, hipMemcpyHostToDevice));
    CMC_TRY(g, hipMemcpy(g->pt.dev.beta_slot, beta_slot.data(), (size_t)R * 8, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}

struct CmcBytes { // a state as bytes, read only
    const uint8_t *s;
    bool get(uint32_t v) const { return s[v] != 0; }
};

extern "C" {

int isingmc_classical_pt_attach(isingmc_classical *g, uint32_t ntemps, const double *betas) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = check_pt_args(g->dev.R, g->dev.replica_offset, ntemps, betas, g->err)) return rc;
    if (const int rc = check_pt_couplings(g->host, g->dev.R, ntemps, g->err)) return rc;
    CMC_TRY(g, hipSetDevice(g->device));
    CMC_TRY(g, hipStreamSynchronize(g->stream));
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
    P.dev.T = ntemps; P.dev.C = R / ntemps;
    P.betas.assign(betas, betas + ntemps);
    P.step = 0;
    CMC_TRY(g, hipMemcpy(P.d_betas, betas, (size_t)ntemps * 8, hipMemcpyHostToDevice));
    CMC_TRY(g, hipMemset(P.dev.attempts, 0, (size_t)R * 8));
    CMC_TRY(g, hipMemset(P.dev.accepts, 0, (size_t)R * 8));
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
    if (kinds >= CMC_KINDS_COUNT) { g->err = "kinds must be one of ISINGMC_CLASSICAL_KINDS_*"; return ISINGMC_EINVAL; }
    if (rounds == 0) return ISINGMC_OK;
    const size_t R = g->dev.R;
    if ((energy_out || mag_out) && rounds > (SIZE_MAX / 16u) / R) { g->err = "the recorded series of this many rounds does not fit"; return ISINGMC_EINVAL; }
    CMC_TRY(g, hipSetDevice(g->device));
    double *d_e = nullptr;
    int32_t *d_m = nullptr;
    auto release = [&]() { if (d_e) (void)hipFree(d_e); if (d_m) (void)hipFree(d_m); };
    if (energy_out) CMC_TRY(g, hipMalloc(reinterpret_cast<void **>(&d_e), (size_t)rounds * R * 8));
    if (mag_out && hipMalloc(reinterpret_cast<void **>(&d_m), (size_t)rounds * R * 4) != hipSuccess) { release(); g->err = "hipMalloc of the magnetisation series failed"; return ISINGMC_ENODEVICE; }
    const CmcStepArgs A{steps, g->pt.dev.beta_slot, nspin, nedge, nworm, kinds, (g->flags & ISINGMC_CLASSICAL_CFG_SERIAL_MOVES) ? 1u : 0u};
    hipError_t e = hipEventRecord(g->ev0, g->stream);
    for (uint64_t i = 0; i < rounds && e == hipSuccess; ++i) { // enqueued back to back: the tempering launch leaves the next steps launch its betas
        if (steps) e = launch_classical_steps(g->stream, g->dev, g->carve, A);
        if (e == hipSuccess) e = launch_classical_tempering(g->stream, g->dev, g->pt.dev, g->pt.step, d_e ? d_e + i * R : nullptr, d_m ? d_m + i * R : nullptr);
        if (e == hipSuccess) g->pt.step++;
    }
    if (e == hipSuccess) e = hipEventRecord(g->ev1, g->stream);
    if (e == hipSuccess) { g->timed = true; e = hipStreamSynchronize(g->stream); }
    if (e == hipSuccess && d_e) e = hipMemcpy(energy_out, d_e, (size_t)rounds * R * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && d_m) e = hipMemcpy(mag_out, d_m, (size_t)rounds * R * 4, hipMemcpyDeviceToHost);
    release();
    if (e != hipSuccess) { g->err = std::string("classical tempering run: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    return ISINGMC_OK;
}

int isingmc_classical_pt_get(isingmc_classical *g, uint32_t *temp_of, uint64_t *pt_step) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_get")) return rc;
    CMC_TRY(g, hipSetDevice(g->device));
    CMC_TRY(g, hipStreamSynchronize(g->stream));
    if (temp_of) CMC_TRY(g, hipMemcpy(temp_of, g->pt.dev.temp_of, (size_t)g->dev.R * 4, hipMemcpyDeviceToHost));
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
    CMC_TRY(g, hipSetDevice(g->device));
    CMC_TRY(g, hipStreamSynchronize(g->stream));
    if (const int rc = upload_maps(g, temp_of)) return rc;
    g->pt.step = pt_step;
    return ISINGMC_OK;
}

int isingmc_classical_pt_swap_counts(isingmc_classical *g, uint64_t *attempts, uint64_t *accepts) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_swap_counts")) return rc;
    CMC_TRY(g, hipSetDevice(g->device));
    CMC_TRY(g, hipStreamSynchronize(g->stream));
    const size_t bytes = (size_t)g->pt.dev.C * (g->pt.dev.T - 1u) * 8;
    if (attempts) CMC_TRY(g, hipMemcpy(attempts, g->pt.dev.attempts, bytes, hipMemcpyDeviceToHost));
    if (accepts) CMC_TRY(g, hipMemcpy(accepts, g->pt.dev.accepts, bytes, hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}

int isingmc_classical_pt_set_swap_counts(isingmc_classical *g, const uint64_t *attempts, const uint64_t *accepts) {
    if (!g) return ISINGMC_EINVAL;
    if (const int rc = need_attached(g, "isingmc_classical_pt_set_swap_counts")) return rc;
    if (!attempts || !accepts) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    CMC_TRY(g, hipSetDevice(g->device));
    CMC_TRY(g, hipStreamSynchronize(g->stream));
    const size_t bytes = (size_t)g->pt.dev.C * (g->pt.dev.T - 1u) * 8;
    CMC_TRY(g, hipMemcpy(g->pt.dev.attempts, attempts, bytes, hipMemcpyHostToDevice));
    CMC_TRY(g, hipMemcpy(g->pt.dev.accepts, accepts, bytes, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}

int isingmc_classical_host_pt_run(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint64_t rounds, uint64_t steps,
                                  uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                                  uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out) {
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
    const uint32_t N = H.N;
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
        for (uint32_t c = 0; c < C; ++c) {
            const size_t base = (size_t)c * T, cbase = (size_t)c * (T - 1u);
            const CmcPtChainView cv{T, betas, temp_of + base, slot_at.data() + base, energy.data() + base, attempts ? attempts + cbase : nullptr,
                                    accepts ? accepts + cbase : nullptr};
            cmc_pt_chain_step(cfg->seed, *pt_step, cfg->replica_offset / T + c, cv, PtHostDraw{});
        }
    }
    return ISINGMC_OK;
}

} // extern "C"
