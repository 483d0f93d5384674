// classical.hip — the handle of classical Monte Carlo in the C ABI (include/isingmc_hip.h, isingmc_classical_*): create and destroy,
// the time steps, the accessors and isingmc_classical_launch_plan.  The checks, the tables and the plan that create relies on are the
// device-free unit's (classical_host.hip, through classical_host.h); the kernels are seen through classical_launch.h alone; the
// handle, shared with classical_pt.hip, is classical_handle.h.
#include "classical_handle.h"

#include <cmath>

using namespace sse;

static int allocate_and_upload(isingmc_classical *g, const isingmc_classical_config *cfg) {
    const CmcHostTables &H = g->host;
    CmcDev &D = g->dev;
    D.R = cfg->nreplicas; D.nwords = (H.N + 31u) / 32u;
    D.seed_lo = (uint32_t)cfg->seed; D.seed_hi = (uint32_t)(cfg->seed >> 32); D.replica_offset = cfg->replica_offset;
    D.T = H.view();
    if (const int rc = cmc_upload(g, &D.T.row, H.row)) return rc;
    if (const int rc = cmc_upload(g, &D.T.ent, H.ent)) return rc;
    if (const int rc = cmc_upload(g, &D.T.jv, H.jv)) return rc;
    if (const int rc = cmc_upload(g, &D.T.edges, H.edges)) return rc;
    D.T.bias = nullptr; D.T.cum = nullptr; D.T.jcode = nullptr; D.T.jr = nullptr; D.T.totalw_r = nullptr;
    if (!H.jcode.empty()) if (const int rc = cmc_upload(g, &D.T.jcode, H.jcode)) return rc;
    if (!H.jr.empty()) if (const int rc = cmc_upload(g, &D.T.jr, H.jr)) return rc;
    if (!H.totalw_r.empty()) if (const int rc = cmc_upload(g, &D.T.totalw_r, H.totalw_r)) return rc;
    if (!H.bias.empty()) if (const int rc = cmc_upload(g, &D.T.bias, H.bias)) return rc;
    if (!H.cum.empty()) if (const int rc = cmc_upload(g, &D.T.cum, H.cum)) return rc;
    if (const int rc = cmc_alloc(g, &D.state, (size_t)D.R * D.nwords)) return rc;
    if (const int rc = cmc_alloc(g, &D.epoch, D.R)) return rc;
    if (const int rc = cmc_alloc(g, &D.counters, (size_t)D.R * 8)) return rc;
    if (const int rc = cmc_alloc(g, &D.err, D.R)) return rc;
    if (const int rc = cmc_alloc(g, &g->d_beta, D.R)) return rc;
    if (const int rc = cmc_alloc(g, &g->d_energy, D.R)) return rc;
    HIP_TRY(g, hipEventCreate(&g->ev0));
    HIP_TRY(g, hipEventCreate(&g->ev1));
    if (cfg->init_state) {
        std::vector<uint32_t> words((size_t)D.R * D.nwords);
        pack_bits(cfg->init_state, D.R, H.N, D.nwords, words.data());
        HIP_TRY(g, hipMemcpy(D.state, words.data(), words.size() * 4, hipMemcpyHostToDevice));
    } else {
        HIP_TRY(g, launch_classical_init_state(nullptr, D, H.N));
        HIP_TRY(g, hipDeviceSynchronize());
    }
    return ISINGMC_OK;
}

extern "C" {

int isingmc_classical_launch_plan(isingmc_classical *g, uint32_t out[8]) {
    if (!g) return ISINGMC_EINVAL;
    if (!out) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    cmc_plan_slots(g->carve, g->host.flags, out);
    return ISINGMC_OK;
}

int isingmc_classical_create(const isingmc_classical_config *cfg, isingmc_classical **out) {
    if (!out) return cmc_refuse(ISINGMC_EINVAL, "null output");
    *out = nullptr;
    if (const int rc = cmc_check_config(cfg)) return rc;
    int dev = 0, max_lds = 0;
    if (const char *why = probe_device(cfg->device, &dev, &max_lds)) return cmc_refuse(ISINGMC_ENODEVICE, why);
    isingmc_classical *g = new isingmc_classical();
    g->device = dev; g->flags = cfg->flags; g->lds_bytes = (uint32_t)max_lds;
    if (const int rc = cmc_plan_config(cfg, (uint32_t)max_lds, g->host, g->carve)) { delete g; return rc; }
    if (const int rc = allocate_and_upload(g, cfg)) { cmc_refuse(rc, g->err); isingmc_classical_destroy(g); return rc; }
    *out = g;
    return ISINGMC_OK;
}

void isingmc_classical_destroy(isingmc_classical *g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->ev0) (void)hipEventDestroy(g->ev0);
    if (g->ev1) (void)hipEventDestroy(g->ev1);
    delete g;
}

const char *isingmc_classical_last_error(const isingmc_classical *g) { return g ? g->err.c_str() : cmc_last_refusal(); }

int isingmc_classical_timesteps(isingmc_classical *g, uint64_t t, const double *beta, uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds) {
    if (!g) return ISINGMC_EINVAL;
    if (!beta) { g->err = "beta must be non-null"; return ISINGMC_EINVAL; }
    if (kinds >= CMC_KINDS_COUNT) { g->err = "kinds must be one of ISINGMC_CLASSICAL_KINDS_*"; return ISINGMC_EINVAL; }
    for (uint32_t r = 0; r < g->dev.R; ++r)
        if (std::isnan(beta[r])) { g->err = "beta must not be NaN"; return ISINGMC_EINVAL; }
    if (t == 0) return ISINGMC_OK;
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipMemcpyAsync(g->d_beta, beta, (size_t)g->dev.R * sizeof(double), hipMemcpyHostToDevice, g->stream));
    const CmcStepArgs A{t, g->d_beta, nspin, nedge, nworm, kinds, (g->flags & ISINGMC_CLASSICAL_CFG_SERIAL_MOVES) ? 1u : 0u};
    HIP_TRY(g, hipEventRecord(g->ev0, g->stream));
    const hipError_t e = launch_classical_steps(g->stream, g->dev, g->carve, A);
    if (e != hipSuccess) { g->err = std::string("classical steps launch: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    HIP_TRY(g, hipEventRecord(g->ev1, g->stream));
    g->timed = true;
    // beta is borrowed for the call only, and its copy was asynchronous from pageable memory: wait for the stream
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    return ISINGMC_OK;
}

int isingmc_classical_get_state(isingmc_classical *g, uint32_t r, uint8_t *out) {
    if (!g) return ISINGMC_EINVAL;
    if (!out || (r != UINT32_MAX && r >= g->dev.R)) { g->err = "bad replica index or null buffer"; return ISINGMC_EINVAL; }
    const uint32_t r0 = r == UINT32_MAX ? 0u : r, rows = r == UINT32_MAX ? g->dev.R : 1u, nw = g->dev.nwords;
    std::vector<uint32_t> words((size_t)rows * nw);
    if (const int rc = copy_down(g, words.data(), g->dev.state + (size_t)r0 * nw, words.size(), true)) return rc;
    unpack_bits(words.data(), rows, g->host.N, nw, out);
    return ISINGMC_OK;
}

int isingmc_classical_set_state(isingmc_classical *g, uint32_t r, const uint8_t *in) {
    if (!g) return ISINGMC_EINVAL;
    if (!in || (r != UINT32_MAX && r >= g->dev.R)) { g->err = "bad replica index or null buffer"; return ISINGMC_EINVAL; }
    const uint32_t r0 = r == UINT32_MAX ? 0u : r, rows = r == UINT32_MAX ? g->dev.R : 1u, nw = g->dev.nwords;
    std::vector<uint32_t> words((size_t)rows * nw);
    pack_bits(in, rows, g->host.N, nw, words.data());
    return copy_up(g, g->dev.state + (size_t)r0 * nw, words.data(), words.size(), true);
}

int isingmc_classical_get_epoch(isingmc_classical *g, uint64_t *out) {
    if (!g) return ISINGMC_EINVAL;
    if (!out) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    return copy_down(g, out, g->dev.epoch, g->dev.R, true);
}

int isingmc_classical_set_epoch(isingmc_classical *g, const uint64_t *epochs) {
    if (!g) return ISINGMC_EINVAL;
    if (!epochs) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    return copy_up(g, g->dev.epoch, epochs, g->dev.R, true);
}

int isingmc_classical_energies(isingmc_classical *g, double *out) {
    if (!g) return ISINGMC_EINVAL;
    if (!out) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    HIP_TRY(g, hipSetDevice(g->device));
    const hipError_t e = launch_classical_energies(g->stream, g->dev, g->d_energy);
    if (e != hipSuccess) { g->err = std::string("classical energies launch: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    return copy_down(g, out, g->d_energy, g->dev.R, true);
}

int isingmc_classical_counters(isingmc_classical *g, uint64_t *out) {
    if (!g) return ISINGMC_EINVAL;
    if (!out) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    return copy_down(g, out, g->dev.counters, (size_t)g->dev.R * 8, true);
}

int isingmc_classical_set_stream(isingmc_classical *g, void *hip_stream) {
    if (!g) return ISINGMC_EINVAL;
    g->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return ISINGMC_OK;
}

int isingmc_classical_synchronize(isingmc_classical *g) {
    if (!g) return ISINGMC_EINVAL;
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    return ISINGMC_OK;
}

int isingmc_classical_last_kernel_ms(isingmc_classical *g, float *ms) {
    if (!g) return ISINGMC_EINVAL;
    if (!ms) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    *ms = 0.f;
    if (!g->timed) return ISINGMC_OK;
    HIP_TRY(g, hipSetDevice(g->device));
    HIP_TRY(g, hipEventSynchronize(g->ev1));
    HIP_TRY(g, hipEventElapsedTime(ms, g->ev0, g->ev1));
    return ISINGMC_OK;
}

} // extern "C"
