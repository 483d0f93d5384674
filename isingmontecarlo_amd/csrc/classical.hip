// classical.hip — the C ABI of classical Monte Carlo (include/isingmc_hip.h, isingmc_classical_*): the config checks, the graph tables,
// the launch plan (isingmc_classical_plan reports it), allocation, the accessors, and the sequential rule on the CPU
// (isingmc_classical_host_steps).  The kernels are seen through classical_launch.h alone; the handle and what tempering
// (classical_pt.hip) shares with this file are in classical_handle.h.
#include "classical_handle.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

using namespace sse;

static_assert(ISINGMC_CLASSICAL_KINDS_ALL == CMC_KINDS_ALL && ISINGMC_CLASSICAL_KINDS_BASIC == CMC_KINDS_BASIC && ISINGMC_CLASSICAL_KINDS_SPIN == CMC_KINDS_SPIN &&
              ISINGMC_CLASSICAL_KINDS_EDGE == CMC_KINDS_EDGE && ISINGMC_CLASSICAL_KINDS_WORM == CMC_KINDS_WORM &&
              ISINGMC_CLASSICAL_KINDS_WORM_NO_DOUBLES == CMC_KINDS_WORM_NO_DOUBLES, "the header's kinds are the rule's");

static thread_local std::string g_classical_error;
int cmc_refuse(int rc, const std::string &why) { g_classical_error = why; return rc; }

int cmc_check_config(const isingmc_classical_config *cfg) {
    if (!cfg || cfg->struct_size != sizeof(isingmc_classical_config)) return cmc_refuse(ISINGMC_EINVAL, "bad config pointer or struct_size");
    if (cfg->nreplicas == 0 || cfg->nvars == 0) return cmc_refuse(ISINGMC_EINVAL, "nreplicas and nvars must be > 0");
    if (cfg->nedges == 0) return cmc_refuse(ISINGMC_EINVAL, "a classical graph needs at least one edge (the reference's edge move would panic)");
    if (!cfg->edges || !cfg->J) return cmc_refuse(ISINGMC_EINVAL, "edges and J must be non-null");
    if (cfg->nvars > CMC_MAX_VARS) return cmc_refuse(ISINGMC_EINVAL, "too many variables (at most 2^24)");
    if (cfg->nedges > 0x3FFFFFFFu) return cmc_refuse(ISINGMC_EINVAL, "too many edges");
    if (cfg->flags & ~(ISINGMC_CLASSICAL_CFG_EDGE_IMPORTANCE | ISINGMC_CLASSICAL_CFG_GLOBAL_TABLES | ISINGMC_CLASSICAL_CFG_SERIAL_MOVES |
                       ISINGMC_CLASSICAL_CFG_PER_REPLICA_J | ISINGMC_CLASSICAL_CFG_GLOBAL_CODES))
        return cmc_refuse(ISINGMC_EINVAL, "unknown flag");
    for (uint32_t e = 0; e < cfg->nedges; ++e) {
        const uint32_t a = cfg->edges[2 * e], b = cfg->edges[2 * e + 1];
        if (a >= cfg->nvars || b >= cfg->nvars) return cmc_refuse(ISINGMC_EINVAL, "edge endpoint out of range");
        if (a == b) return cmc_refuse(ISINGMC_EINVAL, "edge joins a variable to itself (self-loop)");
    }
    const bool per_replica = (cfg->flags & ISINGMC_CLASSICAL_CFG_PER_REPLICA_J) != 0u;
    for (uint32_t r = 0; r < (per_replica ? cfg->nreplicas : 1u); ++r) // J is [R][E] with per-replica couplings: every row is checked
        for (uint32_t e = 0; e < cfg->nedges; ++e) {
            const double j = cfg->J[(size_t)r * cfg->nedges + e];
            auto where = [&]() { return per_replica ? " (couplings row of replica " + std::to_string(r) + ")" : std::string(); };
            if (!std::isfinite(j)) return cmc_refuse(ISINGMC_EINVAL, "couplings must be finite" + where());
            if ((cfg->flags & ISINGMC_CLASSICAL_CFG_EDGE_IMPORTANCE) && !(j > 0.0))
                return cmc_refuse(ISINGMC_EINVAL, "edge importance sampling needs every J > 0 (the reference searches their running sums)" + where());
        }
    for (uint32_t v = 0; cfg->biases && v < cfg->nvars; ++v)
        if (!std::isfinite(cfg->biases[v])) return cmc_refuse(ISINGMC_EINVAL, "biases must be finite");
    return ISINGMC_OK;
}

// binding_mat (graph.rs:69-78) and what goes with it, in the packed form of classical_rule.h
void cmc_build_tables(const isingmc_classical_config *cfg, CmcHostTables &H) {
    const uint32_t N = cfg->nvars, E = cfg->nedges;
    const bool per_replica = (cfg->flags & ISINGMC_CLASSICAL_CFG_PER_REPLICA_J) != 0u;
    const size_t rows = per_replica ? cfg->nreplicas : 1u; // rows of J
    H.N = N; H.E = E; H.flags = per_replica ? CMC_T_PER_REPLICA : 0u;
    // distinct couplings by bit pattern, in order of first appearance (over the rows of J one after the other); the codes matter only
    // while there are at most 256 of them
    std::map<uint64_t, uint32_t> code_of;
    std::vector<uint32_t> code(rows * E);
    std::vector<double> dict;
    for (size_t i = 0; i < rows * E && dict.size() <= 256; ++i) {
        uint64_t bits;
        std::memcpy(&bits, &cfg->J[i], 8);
        auto it = code_of.find(bits);
        if (it == code_of.end()) { it = code_of.emplace(bits, (uint32_t)dict.size()).first; dict.push_back(cfg->J[i]); }
        code[i] = it->second;
    }
    const bool compact = dict.size() <= 256;
    if (compact) H.flags |= CMC_T_COMPACT;
    H.row.assign((size_t)N + 1, 0);
    for (uint32_t e = 0; e < E; ++e) { H.row[cfg->edges[2 * e] + 1]++; H.row[cfg->edges[2 * e + 1] + 1]++; }
    for (uint32_t v = 0; v < N; ++v) H.row[v + 1] += H.row[v];
    struct Ent { uint32_t nbr, edge; };
    std::vector<Ent> ents(2 * (size_t)E);
    std::vector<uint32_t> fill(H.row.begin(), H.row.end() - 1);
    for (uint32_t e = 0; e < E; ++e) { // pushes in edge order ...
        const uint32_t a = cfg->edges[2 * e], b = cfg->edges[2 * e + 1];
        ents[fill[a]++] = Ent{b, e};
        ents[fill[b]++] = Ent{a, e};
    }
    for (uint32_t v = 0; v < N; ++v) // ... then the stable sort by neighbour
        std::stable_sort(ents.begin() + H.row[v], ents.begin() + H.row[v + 1], [](const Ent &x, const Ent &y) { return x.nbr < y.nbr; });
    H.ent.resize(ents.size());
    H.jcode.clear(); H.jr.clear();
    if (!per_replica) {
        H.jv = compact ? dict : std::vector<double>(ents.size());
        for (size_t k = 0; k < ents.size(); ++k) {
            H.ent[k] = ents[k].nbr | (compact ? code[ents[k].edge] << 24 : 0u);
            if (!compact) H.jv[k] = cfg->J[ents[k].edge];
        }
    } else { // the entries hold the neighbour alone; the couplings are a table by (replica, entry)
        for (size_t k = 0; k < ents.size(); ++k) H.ent[k] = ents[k].nbr;
        const size_t stride = 4 * (size_t)cmc_code_words(E);
        if (compact) {
            H.jv = dict;
            H.jcode.assign(rows * stride, 0);
            for (size_t r = 0; r < rows; ++r)
                for (size_t k = 0; k < ents.size(); ++k) H.jcode[r * stride + k] = (uint8_t)code[r * E + ents[k].edge];
        } else {
            H.jv.clear();
            H.jr.resize(rows * ents.size());
            for (size_t r = 0; r < rows; ++r)
                for (size_t k = 0; k < ents.size(); ++k) H.jr[r * ents.size() + k] = cfg->J[r * E + ents[k].edge];
        }
    }
    if (N <= 65536u) {
        H.flags |= CMC_T_EDGE16;
        H.edges.resize(E);
        for (uint32_t e = 0; e < E; ++e) H.edges[e] = cfg->edges[2 * e] | (cfg->edges[2 * e + 1] << 16);
    } else H.edges.assign(cfg->edges, cfg->edges + 2 * (size_t)E);
    H.bias.clear();
    if (cfg->biases && std::any_of(cfg->biases, cfg->biases + N, [](double h) { return h != 0.0; })) {
        H.flags |= CMC_T_BIAS;
        H.bias.assign(cfg->biases, cfg->biases + N);
    }
    H.cum.clear(); H.totalw_r.clear(); H.totalw = 0.0;
    if (cfg->flags & ISINGMC_CLASSICAL_CFG_EDGE_IMPORTANCE) { // the fold of graph.rs:324-331, row by row
        H.flags |= CMC_T_CUM;
        H.cum.resize(rows * E);
        for (size_t r = 0; r < rows; ++r) {
            double accw = 0.0;
            for (uint32_t e = 0; e < E; ++e) { accw = accw + cfg->J[r * E + e]; H.cum[r * E + e] = accw; }
            if (per_replica) H.totalw_r.push_back(accw); else H.totalw = accw;
        }
    }
}

uint32_t CmcHostTables::first_mixed_chain(uint32_t R, uint32_t T) const {
    if (!(flags & CMC_T_PER_REPLICA)) return CMC_NONE;
    // equal codes are equal bit patterns (the dictionary is keyed by them); the doubles are compared as bytes
    const uint8_t *base = (flags & CMC_T_COMPACT) ? jcode.data() : reinterpret_cast<const uint8_t *>(jr.data());
    const size_t stride = (flags & CMC_T_COMPACT) ? 4 * (size_t)cmc_code_words(E) : 16 * (size_t)E;
    for (uint32_t r = 0; r < R; ++r)
        if (r % T != 0u && std::memcmp(base + (size_t)r * stride, base + (size_t)(r - r % T) * stride, stride) != 0) return r / T;
    return CMC_NONE;
}

// checks, tables and the launch plan: everything isingmc_classical_create decides before it touches a device
static int plan_config(const isingmc_classical_config *cfg, uint32_t lds_bytes, CmcHostTables &H, CmcCarve &C) {
    if (const int rc = cmc_check_config(cfg)) return rc;
    cmc_build_tables(cfg, H);
    const size_t total_words = lds_bytes / 4;
    C = cmc_plan(H.view(), total_words, ((cfg->flags & ISINGMC_CLASSICAL_CFG_GLOBAL_TABLES) ? (uint32_t)CMC_FORCE_GLOBAL : 0u) |
                                            ((cfg->flags & ISINGMC_CLASSICAL_CFG_GLOBAL_CODES) ? (uint32_t)CMC_FORCE_GLOBAL_CODES : 0u));
    if (C.W == 0u) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "model too large: the state bits and move stamps of one replica exceed LDS (at most %u variables in %u bytes)",
                      cmc_max_vars(total_words), lds_bytes);
        return cmc_refuse(ISINGMC_ENOTIMPL, msg);
    }
    return ISINGMC_OK;
}

// the eight slots of isingmc_classical_plan / isingmc_classical_launch_plan
static void plan_slots(const CmcCarve &C, uint32_t table_flags, uint32_t out[8]) {
    const uint32_t format = !(table_flags & CMC_T_PER_REPLICA) ? 0u : (table_flags & CMC_T_COMPACT) ? 1u : 2u;
    const uint32_t slots[8] = {C.W, C.in_lds, C.words, C.wave_words + (C.o_jcode != CMC_NONE ? C.code_words : 0u), C.has, (table_flags & CMC_T_COMPACT) ? 1u : 0u,
                               (table_flags & CMC_T_EDGE16) ? 1u : 0u, format};
    std::copy(slots, slots + 8, out);
}

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

// the sequential rule on the CPU: t time steps of one replica (isingmc_classical_host_steps, isingmc_classical_host_pt_run)
void cmc_host_replica_steps(const CmcGraphMem &g, uint64_t seed, uint32_t replica, uint64_t t, double beta, const CmcHostMoves &m, uint8_t *state,
                            uint8_t *mark, uint64_t *epoch, uint64_t *ctr) {
    const uint32_t N = g.N();
    CmcHostState s{state, mark};
    CmcHostDraw draw{(uint32_t)seed, (uint32_t)(seed >> 32), replica, 0u, 0u};
    for (uint64_t step = 0; step < t; ++step, ++*epoch) {
        draw.epoch_lo = (uint32_t)*epoch; draw.epoch_hi24 = (uint32_t)(*epoch >> 32) & 0xFFFFFFu;
        const uint32_t kind = cmc_step_kind(m.kinds, draw);
        if (kind == 2u) {
            uint32_t ndraw = 0;
            for (uint32_t i = 0; i < m.nworm; ++i) cmc_worm(g, s, beta, m.kinds != CMC_KINDS_WORM_NO_DOUBLES, draw, &ndraw, ctr);
            continue;
        }
        const uint32_t n = kind == 0u ? m.nspin : m.nedge;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t choice = draw(SSE_TAG_CLASSICAL, cmc_index_move(i), 0), uword = draw(SSE_TAG_CLASSICAL, cmc_index_move(i), 1);
            uint32_t a, b = CMC_NONE;
            if (kind == 0u) a = cmc_range(choice, N); else g.edge(cmc_pick_edge(g, choice), a, b);
            const double de = kind == 0u ? cmc_spin_de(g, s, a) : cmc_edge_de(g, s, a, b);
            const bool acc = cmc_should_flip(beta, de, uword);
            if (acc) { s.s[a] ^= 1u; if (kind == 1u) s.s[b] ^= 1u; }
            ctr[kind == 0u ? CMC_C_SPIN : CMC_C_EDGE] += 1;
            ctr[kind == 0u ? CMC_C_SPIN_ACC : CMC_C_EDGE_ACC] += acc ? 1u : 0u;
        }
    }
}

extern "C" {

int isingmc_classical_plan(const isingmc_classical_config *cfg, uint32_t lds_bytes, uint32_t out[8]) {
    if (!out) return cmc_refuse(ISINGMC_EINVAL, "null output");
    CmcHostTables H; CmcCarve C;
    if (const int rc = plan_config(cfg, lds_bytes, H, C)) return rc;
    plan_slots(C, H.flags, out);
    return ISINGMC_OK;
}

int isingmc_classical_launch_plan(isingmc_classical *g, uint32_t out[8]) {
    if (!g) return ISINGMC_EINVAL;
    if (!out) { g->err = "null buffer"; return ISINGMC_EINVAL; }
    plan_slots(g->carve, g->host.flags, out);
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
    if (const int rc = plan_config(cfg, (uint32_t)max_lds, g->host, g->carve)) { delete g; return rc; }
    if (const int rc = allocate_and_upload(g, cfg)) { g_classical_error = g->err; isingmc_classical_destroy(g); return rc; }
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

const char *isingmc_classical_last_error(const isingmc_classical *g) { return g ? g->err.c_str() : g_classical_error.c_str(); }

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

int isingmc_classical_host_steps(const isingmc_classical_config *cfg, uint64_t t, const double *beta, uint32_t nspin, uint32_t nedge,
                                 uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint64_t *counters) {
    if (const int rc = cmc_check_config(cfg)) return rc;
    if (!beta || !states || !epochs) return cmc_refuse(ISINGMC_EINVAL, "beta, states and epochs must be non-null");
    if (kinds >= CMC_KINDS_COUNT) return cmc_refuse(ISINGMC_EINVAL, "kinds must be one of ISINGMC_CLASSICAL_KINDS_*");
    CmcHostTables H;
    cmc_build_tables(cfg, H);
    const uint32_t N = H.N;
    const CmcHostMoves m{cmc_default_moves(nspin, N / 2u), cmc_default_moves(nedge, H.E / 2u), cmc_default_moves(nworm, 1u), kinds};
    std::vector<uint8_t> mark(N, 0);
    for (uint32_t r = 0; r < cfg->nreplicas; ++r) {
        uint64_t ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        cmc_host_replica_steps(cmc_graph_mem(H.view(), r), cfg->seed, cfg->replica_offset + r, t, beta[r], m, states + (size_t)r * N, mark.data(), &epochs[r], ctr);
        for (int i = 0; counters && i < 8; ++i) counters[(size_t)r * 8 + i] += ctr[i];
    }
    return ISINGMC_OK;
}

} // extern "C"
