// create.hip — isingmc_create and isingmc_destroy: the config checks, the bond tables, the batch plan (isingmc_plan_batch reports it),
// every allocation and upload, the initial state.  LDS sizes come from lds_plan.h, the kernels' limits from sse_launch.h.
#include "batch.hip.h"
#include "sse_core.hip.h" // Rng
#include "sse_launch.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

using namespace sse;

static thread_local std::string g_create_error;

// All that plan_batch() chooses (isingmc_plan_batch reports it): the geometry, and what isingmc_create sizes its allocations by or
// hands to the DevBatch, which owns those values from then on
struct BatchPlan : BatchGeometry {
    uint32_t Wmax = 0;                  // most waves any launch may use: sizes the row stride, the HBM tables and the union-find scratch
    uint32_t CH = 0, nchunks = 0, stride = 0; // isingmc_plan_geometry(cap, W, K, Wmax)
    uint32_t pm_words = 0;              // +-J decode: sign words per bond-table row (0 = another decode)
    uint32_t tbl_stride = 0;            // bytes per replica of the per-variable tables in HBM (0 = they live in LDS)
    size_t ufstride = 0;                // words per replica of the union-find scratch in HBM: Wmax N + cap ids and two bit arrays over them
    uint32_t lds_ufcap = 0;             // ids of the LDS union-find of the first general launch
};

__global__ void init_state_kernel(DevBatch B) {
    // classical/graph.rs:451-453 make_random_spin_state: one fair bit per variable (Philox tag INIT, epoch 0)
    const uint32_t r = blockIdx.x;
    const Rng rng = make_rng(B, r, 0ull);
    for (uint32_t i = threadIdx.x; i < B.nwords; i += blockDim.x) {
        uint32_t s = 0;
        for (uint32_t j = 0; j < 32 && i * 32 + j < B.N; ++j) s |= (rng.draw(SSE_TAG_INIT, i * 32 + j).x >> 31) << j;
        B.state[(size_t)r * B.nwords + i] = s;
    }
}

// ---- isingmc_create in four parts: check_config, build_tables, plan_batch, allocate_and_upload -------------------------------
// Everything up to the plan reads the config alone and touches no device, so that isingmc_plan_batch can run it on any host.
static int refuse(int rc, const char *why) { g_create_error = why; return rc; }
static bool per_replica_J(const isingmc_config *cfg) { return (cfg->flags & ISINGMC_CFG_PER_REPLICA_J) != 0; }
static double gamma_of(const isingmc_config *cfg, uint32_t row) { return cfg->transverse_r ? cfg->transverse_r[row] : cfg->transverse; }
static double hfield_of(const isingmc_config *cfg, uint32_t row) { return cfg->longitudinal_r ? cfg->longitudinal_r[row] : cfg->longitudinal; }
static bool has_longitudinal(const isingmc_config *cfg) { return !cfg->interactions && std::fabs(hfield_of(cfg, 0)) > DBL_EPSILON; } // qmc_ising.rs:230

// The argument checks that isingmc_create makes before it looks for a device (cfg itself is readable: the entry points see to that)
static int check_config(const isingmc_config *cfg) {
    const bool generic = cfg->interactions != nullptr;
    if (generic) {
        if (cfg->nreplicas == 0 || cfg->nvars == 0 || cfg->ninteractions == 0) return refuse(ISINGMC_EINVAL, "nreplicas, nvars, ninteractions must be > 0");
        if (per_replica_J(cfg)) return refuse(ISINGMC_EINVAL, "per-replica couplings are not available with generic interactions");
        for (uint32_t i = 0; i < cfg->ninteractions; ++i) {
            const isingmc_interaction &it = cfg->interactions[i];
            if (it.nvars > 2) // qmc_runner.rs:415-680 allows any k; the 32-bit operator word holds two variables
                return refuse(ISINGMC_ENOTIMPL, "interactions on more than two variables are not implemented (operator word = 2 in + 2 out bits)");
            if ((it.nvars != 1 && it.nvars != 2) || !it.mat || it.vars[0] >= cfg->nvars || (it.nvars == 2 && (it.vars[1] >= cfg->nvars || it.vars[1] == it.vars[0])))
                return refuse(ISINGMC_EINVAL, "interaction must act on 1 or 2 distinct variables inside the model and carry a matrix");
            for (uint32_t k = 0; k < (it.diagonal_only ? (1u << it.nvars) : (1u << (2 * it.nvars))); ++k)
                if (!(it.mat[k] >= 0.0) || !std::isfinite(it.mat[k])) return refuse(ISINGMC_EINVAL, "interaction matrix entries must be finite and >= 0");
        }
    } else if (cfg->nreplicas == 0 || cfg->nvars == 0 || (cfg->nedges != 0 && (!cfg->edges || !cfg->J)))
        return refuse(ISINGMC_EINVAL, "nreplicas and nvars must be > 0 and edges/J non-null when nedges > 0");
    if (cfg->capacity == 0) return refuse(ISINGMC_EINVAL, "capacity must be > 0");
    if (cfg->cutoff0 > cfg->capacity) return refuse(ISINGMC_EINVAL, "cutoff0 exceeds capacity");
    if (cfg->nvars > SSE_VAR_MASK) return refuse(ISINGMC_EINVAL, "too many variables");
    if (!generic && !(cfg->transverse >= 0.0)) return refuse(ISINGMC_EINVAL, "transverse field must be >= 0");
    for (uint32_t e = 0; !generic && e < cfg->nedges; ++e)
        if (cfg->edges[2 * e] >= cfg->nvars || cfg->edges[2 * e + 1] >= cfg->nvars || cfg->edges[2 * e] == cfg->edges[2 * e + 1])
            return refuse(ISINGMC_EINVAL, cfg->edges[2 * e] == cfg->edges[2 * e + 1] ? "edge joins a variable to itself (self-loop)" : "edge endpoint out of range");
    return ISINGMC_OK;
}
// The model fields of a DevBatch (its shape and fields; the tables add uniformJ / wJ / wtot, the plan its geometry)
static DevBatch model_of(const isingmc_config *cfg) {
    const bool generic = cfg->interactions != nullptr, has_long = has_longitudinal(cfg);
    DevBatch D{};
    D.R = cfg->nreplicas; D.N = cfg->nvars; D.E = generic ? 0u : cfg->nedges;
    D.Nb = generic ? cfg->ninteractions : cfg->nedges + cfg->nvars + (has_long ? cfg->nvars : 0);
    D.cap = cfg->capacity; D.nwords = (cfg->nvars + 31) / 32;
    D.seed_lo = (uint32_t)cfg->seed; D.seed_hi = (uint32_t)(cfg->seed >> 32);
    D.replica_offset = cfg->replica_offset;
    D.gamma = cfg->transverse; D.wh = 2.0 * std::fabs(cfg->longitudinal); D.hpos = cfg->longitudinal > 0.0 ? 1u : 0u;
    D.has_long = has_long ? 1u : 0u;
    D.bond_stride = per_replica_J(cfg) ? D.Nb : 0u;
    D.rvb_growers = (cfg->flags & ISINGMC_CFG_RVB_SERIAL_GROWTH) ? 0u : 64u;
    return D;
}

// The checks behind the device probe that need no plan: fields, bond count, the geometry wishes (plan_batch refuses the rest where it
// meets them, in the order they always had)
static int check_config_model(const isingmc_config *cfg) {
    const bool generic = cfg->interactions != nullptr, perJ = per_replica_J(cfg), has_long = has_longitudinal(cfg);
    if ((cfg->transverse_r || cfg->longitudinal_r) && (!perJ || generic)) return refuse(ISINGMC_EINVAL, "per-replica fields need ISINGMC_CFG_PER_REPLICA_J (per-replica bond tables)");
    for (uint32_t r = 0; !generic && r < (perJ ? cfg->nreplicas : 1u); ++r) {
        if (!(gamma_of(cfg, r) >= 0.0) || !std::isfinite(gamma_of(cfg, r)) || !std::isfinite(hfield_of(cfg, r))) return refuse(ISINGMC_EINVAL, "fields must be finite, transverse field >= 0");
        if ((std::fabs(hfield_of(cfg, r)) > DBL_EPSILON) != has_long) return refuse(ISINGMC_EINVAL, "longitudinal fields must be all zero or all non-zero within a batch");
    }
    if (model_of(cfg).Nb > SSE_MAX_BONDS) return refuse(ISINGMC_EINVAL, "too many bonds");
    if (wave_index(cfg->waves_per_replica ? cfg->waves_per_replica : 4) < 0) return refuse(ISINGMC_EINVAL, "waves_per_replica must be 1, 4, 6, 8 or 16");
    const uint32_t K = cfg->slots_per_lane ? cfg->slots_per_lane : 4;
    if (K != 1 && K != 2 && K != 4) return refuse(ISINGMC_EINVAL, "slots_per_lane must be 1, 2 or 4");
    return ISINGMC_OK;
}

// Everything that create uploads, on the host: made from the config alone
struct Tables {
    std::vector<BondRec> bonds;          // [nH][Nb], nH = one row, or one per replica (ISINGMC_CFG_PER_REPLICA_J: cfg->J is [R][E])
    std::vector<double> cum, wtots;      // [nH][Nb] heat-bath cumulative weights; [nH] their totals
    std::vector<double> offsets;         // [nH] energy offsets (per-replica J only)
    double offset = 0.0;                 // ... of row 0
    std::vector<double> mats;            // generic interactions: [Nb][16] in | out<<2
    bool generic_sym = false;            // ... all of them symmetric under a global spin flip
    uint32_t uniformJ = 1u; double wJ = 0.0; // one |J| on every edge of every row (the kernels keep 2|J| in a scalar register)
    std::vector<double> edge_w;          // [E] 2|J| of row 0
    std::vector<uint32_t> edges_compact; // [E] a | c << 15 | prefers_aligned << 30 (N <= SSE_CE_MAX_VARS, else zeros)
    std::vector<uint32_t> signs;         // [nH][ceil(E / 32)] bit e = prefers aligned (J < 0): the +-J decode's rows
    std::vector<uint32_t> adj_start, adj; // [N + 2], [2 E + 1] bonds_for_var (make_classical_bonds, qmc_ising.rs:421-432): edge order
};
// bond b = interaction b.  Weights go to mats[b][in | out<<2] (bit 0 = first variable); the reference's index is (out0 out1 in0 in1)
// with the first variable most significant (Interaction::index_from_state, qmc_runner.rs:666-679).  Kinds only feed the
// transverse-op counters: a one-variable interaction with four equal entries is a cluster edge (cluster.rs:284-286).
static void generic_tables(const isingmc_config *cfg, uint32_t Nb, Tables &T) {
    T.mats.assign((size_t)Nb * 16, 0.0);
    T.generic_sym = true;
    double c = 0.0;
    for (uint32_t i = 0; i < Nb; ++i) {
        const isingmc_interaction &it = cfg->interactions[i];
        double *mb = T.mats.data() + (size_t)i * 16;
        for (uint32_t in = 0; in < (1u << it.nvars); ++in)      // device layout: bit 0 = first variable
            for (uint32_t out = 0; out < (1u << it.nvars); ++out) {
                const uint8_t ib[2] = {(uint8_t)(in & 1u), (uint8_t)((in >> 1) & 1u)}, ob[2] = {(uint8_t)(out & 1u), (uint8_t)((out >> 1) & 1u)};
                (void)isingmc_interaction_at(&it, ib, ob, &mb[in | (out << 2)]);
            }
        double maxw = 0.0; // heatbath.rs:130-146 make_bond_weights: largest diagonal element
        for (uint32_t st = 0; st < (it.nvars == 2 ? 4u : 2u); ++st) maxw = std::max(maxw, mb[st | (st << 2)]);
        const uint32_t kind = it.nvars == 2 ? SSE_BOND_TWO_SITE
                              : ((mb[0] == mb[1] && mb[0] == mb[4] && mb[0] == mb[5]) ? SSE_BOND_TRANSVERSE : SSE_BOND_LONGITUDINAL);
        T.bonds[i].a_info = it.vars[0] | (kind << SSE_INFO_SHIFT);
        T.bonds[i].c = it.nvars == 2 ? it.vars[1] : SSE_NO_VAR;
        T.bonds[i].w = maxw;
        c = (i == 0) ? maxw : maxw + c;
        T.cum[i] = c;
        // EVERY weight equals the weight with all spins flipped.  (Not isingmc_interaction_sym_under_ising: like the reference's
        // Interaction::sym_under_ising, qmc_runner.rs:639-664, that one only compares the entries whose outputs are all 0, and
        // passes two-variable matrices that break the symmetry elsewhere.)
        const uint32_t mask = it.nvars == 2 ? 0xFu : 0x5u;
        for (uint32_t idx = 0; idx < 16; ++idx)
            if ((idx & ~mask) == 0 && std::fabs(mb[idx] - mb[idx ^ mask]) >= DBL_EPSILON) T.generic_sym = false;
    }
    T.wtots[0] = c;
    T.offset = cfg->energy_offset;
}
// Bond-table row hI of an Ising model (qmc_ising.rs:186-205,228-246; weights :863-888; offsets :97-99): edges, transverse bonds,
// longitudinal bonds when there is a field
static void ising_row(const isingmc_config *cfg, const DevBatch &D, uint32_t hI, Tables &T) {
    BondRec *t0 = T.bonds.data() + (size_t)hI * D.Nb;
    const double *Jh = cfg->J + (size_t)hI * D.E;
    double off = 0.0;
    for (uint32_t e = 0; e < D.E; ++e) {
        const double J = Jh[e];
        t0[e].a_info = cfg->edges[2 * e] | ((SSE_BOND_TWO_SITE | (J < 0.0 ? SSE_BOND_PREF_BIT : 0u)) << SSE_INFO_SHIFT);
        t0[e].c = cfg->edges[2 * e + 1];
        t0[e].w = 2.0 * std::fabs(J);
        off += std::fabs(J);
        if (J < 0.0) T.signs[(size_t)hI * ((D.E + 31u) / 32u) + (e >> 5)] |= 1u << (e & 31);
    }
    const double gam = gamma_of(cfg, hI), hl = hfield_of(cfg, hI);
    for (uint32_t v = 0; v < D.N; ++v) {
        BondRec &t = t0[D.E + v];
        t.a_info = v | (SSE_BOND_TRANSVERSE << SSE_INFO_SHIFT); t.c = SSE_NO_VAR; t.w = gam;
    }
    for (uint32_t v = 0; D.has_long && v < D.N; ++v) {
        BondRec &t = t0[D.E + D.N + v];
        t.a_info = v | ((SSE_BOND_LONGITUDINAL | (hl > 0.0 ? SSE_BOND_PREF_BIT : 0u)) << SSE_INFO_SHIFT);
        t.c = SSE_NO_VAR; t.w = 2.0 * std::fabs(hl);
    }
    const double offset = off + (double)D.N * (gam + std::fabs(hl));
    if (hI == 0) T.offset = offset;
    if (D.bond_stride) T.offsets[hI] = offset;
    double c = 0.0;
    for (uint32_t i = 0; i < D.Nb; ++i) { c = (i == 0) ? t0[0].w : t0[i].w + c; T.cum[(size_t)hI * D.Nb + i] = c; }
    T.wtots[hI] = c;
}
static Tables build_tables(const isingmc_config *cfg, const DevBatch &D) {
    const bool generic = cfg->interactions != nullptr;
    const uint32_t nH = D.bond_stride ? D.R : 1u;
    Tables T;
    T.bonds.resize((size_t)nH * D.Nb); T.cum.resize((size_t)nH * D.Nb); T.wtots.resize(nH);
    if (D.bond_stride) T.offsets.resize(nH);
    T.signs.assign((size_t)nH * ((D.E + 31u) / 32u), 0u);
    if (generic) generic_tables(cfg, D.Nb, T);
    else for (uint32_t hI = 0; hI < nH; ++hI) ising_row(cfg, D, hI, T);
    T.wJ = T.bonds[0].w;
    for (uint32_t hI = 0; hI < nH && T.uniformJ; ++hI)
        for (uint32_t e = 0; e < D.E; ++e) if (T.bonds[(size_t)hI * D.Nb + e].w != T.bonds[0].w) { T.uniformJ = 0u; break; }
    T.edge_w.resize(D.E); T.edges_compact.assign(D.E, 0u);
    for (uint32_t e = 0; e < D.E; ++e) {
        const BondRec &t = T.bonds[e];
        T.edge_w[e] = t.w;
        if (D.N <= SSE_CE_MAX_VARS)
            T.edges_compact[e] = (t.a_info & SSE_CE_VAR_MASK) | ((t.c & SSE_CE_VAR_MASK) << 15) | (((t.a_info >> (SSE_INFO_SHIFT + 2)) & 1u) << 30);
    }
    std::vector<uint32_t> &as = T.adj_start, &ad = T.adj, fill(D.N, 0u);
    as.assign(D.N + 2, 0u); ad.resize(2 * (size_t)D.E + 1);
    for (uint32_t e = 0; e < D.E; ++e) { as[cfg->edges[2 * e] + 1]++; as[cfg->edges[2 * e + 1] + 1]++; }
    for (uint32_t v = 0; v < D.N; ++v) as[v + 1] += as[v];
    for (uint32_t e = 0; e < D.E; ++e) {
        const uint32_t a = cfg->edges[2 * e], c2 = cfg->edges[2 * e + 1];
        ad[as[a] + fill[a]++] = e;
        ad[as[c2] + fill[c2]++] = e;
    }
    return T;
}

// Where the per-variable scan tables live when the caller wishes for W_wish waves (0 = no wish) and `ledges` words of compact edge
// table share the LDS: the wave count to run with, and whether the engine moves the tables to HBM by itself (they do not fit)
struct TablesHome { uint32_t W; bool hbm; };
static TablesHome tables_home(const DevBatch &D, uint32_t W_wish, uint32_t ledges, size_t total_words) {
    auto fixed_lds = [&](uint32_t w) { return general_lds_words(w, D, ledges, false, 0u, 0u); }; // (tables in LDS, no union-find)
    uint32_t W = W_wish ? W_wish : 4;
    if (fixed_lds(W) + 4096 <= total_words) return {W, false};
    if (!W_wish) return {W, true};
    // explicit geometry: keep the LDS tables if a smaller W makes them fit
    while (W > 1 && fixed_lds(W) + 4096 > total_words) W = (W == 4) ? 1 : (W == 6 ? 4 : W >> 1);
    if (fixed_lds(W) + 64 <= total_words) return {W, false};
    return {W_wish, true};
}
// What plan_batch reads: the model's shape (D: N, E, Nb, cap, nwords, has_long, uniformJ), its kind, the caller's flags and geometry
// wishes, the LDS bytes of a workgroup
struct PlanInputs {
    DevBatch D;
    bool generic, perJ, fields_r; // interaction matrices; per-replica bond tables; per-replica fields among them
    uint32_t flags, waves_per_replica, slots_per_lane, waves_offdiag, lds_uf_ids_limit, lds_bytes;
};
static PlanInputs plan_inputs(const isingmc_config *cfg, const DevBatch &D, uint32_t lds_bytes) {
    return {D, cfg->interactions != nullptr, per_replica_J(cfg), cfg->transverse_r || cfg->longitudinal_r,
            cfg->flags, cfg->waves_per_replica, cfg->slots_per_lane, cfg->waves_offdiag, cfg->lds_uf_ids_limit, lds_bytes};
}
// Every launch geometry and mode of a batch.  Reads its inputs and nothing else: no device, no batch.  The configs it cannot serve
// it refuses like the checks do, where their order among them has always been.
static int plan_batch(const PlanInputs &in, BatchPlan &p) {
    DevBatch D = in.D; // (gains pm_words below)
    const uint32_t flags = in.flags;
    const size_t total_words = (size_t)in.lds_bytes / 4; // all of LDS for one workgroup
    p = BatchPlan{};
    p.lds_total_words = total_words; p.uf_ids_limit = in.lds_uf_ids_limit;
    p.fused_launch = (flags & ISINGMC_CFG_FUSED_LAUNCH) != 0;
    // default 4 waves per replica: with 16-bit union-find parents the footprint at the headline size stays below half
    // of the 160 KB LDS, so two workgroups share a CU and overlap each other's barriers (measured best on MI355X)
    uint32_t W = in.waves_per_replica ? in.waves_per_replica : 4;
    uint32_t K = in.slots_per_lane ? in.slots_per_lane : 4;
    // compact edge table staged in LDS when it is small enough (a|c<<15|pref<<30 needs N <= 32768)
    bool CL = !in.generic && !in.perJ && D.uniformJ && D.N <= SSE_CE_MAX_VARS && (size_t)D.E * 4 <= 48 * 1024 && !(flags & ISINGMC_CFG_NO_LDS_TABLES);
    // Per-variable scan tables: in LDS while W copies of them fit (with room for a union-find), otherwise in a per-replica
    // HBM scratch served by L2 / Infinity Cache (MODE 2; ISINGMC_CFG_GLOBAL_TABLES forces it on any model).
    bool TG = (flags & ISINGMC_CFG_GLOBAL_TABLES) != 0;
    if (!TG) {
        TablesHome h = tables_home(D, in.waves_per_replica, CL ? D.E : 0u, total_words);
        // The tables do not fit next to the compact edge table (a long chain: up to 48 KB of edges): the edge table leaves LDS first
        // (the general bond table serves the model), and the HBM tables, which need the general bond table, come without it too.
        if (h.hbm && CL) { CL = false; h = tables_home(D, in.waves_per_replica, 0u, total_words); }
        W = h.W; TG = h.hbm;
    }
    const uint32_t ledges = CL ? D.E : 0u;
    // (only with the caller's own ISINGMC_CFG_GLOBAL_TABLES)
    if (TG && CL) return refuse(ISINGMC_EINVAL, "ISINGMC_CFG_GLOBAL_TABLES needs the general bond table: combine it with ISINGMC_CFG_NO_LDS_TABLES");
    if (TG && K == 2) K = 4;
    const uint32_t pm_room = TG ? (D.E + 31u) / 32u : 0u; // (room for the +-J decode's signs, decided below)
    if (general_lds_words(W, D, ledges, TG, pm_room, 0u) + 64 > total_words) return refuse(ISINGMC_ENOTIMPL, "model too large: the spin-state bit arrays alone exceed LDS");
    // off-diagonal launches may use their own wave count (see plan_off()): explicit, or decided per launch (then up to 16)
    uint32_t W_off = in.waves_offdiag;
    // (a check of the wish alone; it stands here, behind the two refusals above, because that has always been its place among them)
    if (W_off != 0 && wave_index(W_off) < 0) return refuse(ISINGMC_EINVAL, "waves_offdiag must be 0, 1, 4, 6, 8 or 16");
    if (!W_off && in.waves_per_replica) W_off = W; // an explicit waves_per_replica pins both kinds of launch
    if (TG) W_off = W;                             // tables in HBM: one geometry for every launch
    if (W_off && general_lds_words(W_off, D, ledges, TG, 0u, 0u) + 64 > total_words) W_off = W;
    auto fits_in_lds = [&](uint32_t w) { return !TG && general_lds_words(w, D, ledges, false, 0u, 0u) + 64 <= total_words; };
    const bool w16_possible = fits_in_lds(16);
    // (8 waves without an LDS union-find: the geometry of launches whose cluster ids need the 32-bit union-find in HBM anyway)
    const bool w8_possible = W < 8 && (K == 4 || K == 1) && fits_in_lds(8);
    p.w8_ok = w8_possible && !W_off;
    const uint32_t Wmax = W_off ? (W_off > W ? W_off : W) : ((W < 16 && w16_possible) ? 16u : (w8_possible ? 8u : W));
    p.W = W; p.K = K; p.W_off = W_off; p.Wmax = Wmax;
    p.mode = TG ? SSE_MODE_GLOBAL_TABLES : (CL ? SSE_MODE_LDS_EDGES : SSE_MODE_GENERAL);
    // "+-J" decode for large disorder batches (BASELINE configs[4]): every replica its own coupling signs on one graph with uniform
    // |J|, Gamma, h.  The general decode fetches a 16-byte record per op and pass from a per-replica table of megabytes — one random
    // HBM sector each time, in a mode that is bound by exactly those; here the variables come from the shared compact edge table
    // (L2-resident), the sign from 12 KB of LDS.  Default geometry only.
    if (TG && in.perJ && D.uniformJ && !in.generic && W == 4 && K == 4 && D.N <= SSE_CE_MAX_VARS && !in.fields_r && !(flags & ISINGMC_CFG_NO_PM_DECODE)) {
        p.mode = SSE_MODE_PM_GLOBAL_TABLES;
        p.pm_words = D.pm_words = (D.E + 31u) / 32u;
        // the diagonal launch keeps its per-wave spin bytes in LDS when W * N bytes fit next to the small arrays
        const size_t words = diag_lds_words(W, D, 0u, false, D.pm_words, true);
        p.lds_words_pm_diag = (words + 64 <= total_words && !(flags & ISINGMC_CFG_GLOBAL_TABLES)) ? words : 0;
    }
    uint32_t geo[4]; // chunk grid and row stride: one function (also exported for the CPU-side bound checks of tests/test_abi_cpu.py)
    if (isingmc_plan_geometry(D.cap, W, K, Wmax, geo) != ISINGMC_OK) return refuse(ISINGMC_EINVAL, "capacity too large for the row stride");
    p.CH = geo[0]; p.nchunks = geo[1]; p.stride = geo[2];
    p.lds_words_diag = diag_lds_words(W, D, ledges, TG, pm_room);
    p.lds_words_fast = fast_lds_words(D);
    p.fast_diag = CL && !TG && W == 4 && (K == 4 || K == 2) && D.N <= fast_max_vars() && !p.fused_launch &&
                  !(flags & ISINGMC_CFG_NO_FAST_DIAG) && lds_bytes_of(p.lds_words_fast) <= 40 * 1024; // 4 workgroups per CU
    // the cluster update of that geometry has its own kernel too (16 waves, packed tables; sse_cluster.hip.h)
    p.lean_cluster = CL && !TG && !in.generic && D.N <= cluster_max_vars() && !p.fused_launch && !in.waves_offdiag && !in.waves_per_replica &&
                     !(flags & ISINGMC_CFG_NO_LEAN_CLUSTER);
    p.defer = p.lean_cluster && p.fast_diag && !(flags & ISINGMC_CFG_NO_DEFERRED_FLIPS);
    // the RVB pass reuses everything from the scan tables on: launches that run it get enough LDS for its scratch
    // and constant-op table (other launches keep the smaller footprint, which decides workgroups per CU)
    p.lds_words_rvb = std::min(rvb_lds_words(W, D, ledges, TG, pm_room), total_words);
    p.rvb_global = (flags & ISINGMC_CFG_RVB_GLOBAL_TABLES) != 0; // (the two-launch form keeps its tables in LDS: never with this flag)
    p.rvb_split = !in.generic && !TG && !p.fused_launch && !(flags & ISINGMC_CFG_RVB_FUSED) && !p.rvb_global;
    // waves of the RVB main launch: as many as keep about 16 waves on a CU (its LDS footprint decides how many replicas share one)
    const size_t w4 = 4 * (size_t)rvb_main_lds_words(4, D, ledges);
    const size_t per_cu = w4 ? (size_t)in.lds_bytes / w4 : 0;
    p.rvb_main_W = per_cu >= 4 ? 4u : (per_cu >= 2 ? 8u : 16u);
    if (in.waves_per_replica == 4 || in.waves_per_replica == 8 || in.waves_per_replica == 16) p.rvb_main_W = in.waves_per_replica; // an explicit geometry is honoured here too
    if (TG) p.tbl_stride = (uint32_t)((((size_t)Wmax * D.N * 4 + D.N) + 15) & ~(size_t)15); // 4-byte scan records per (wave, variable)
    const size_t ids_max = (size_t)Wmax * D.N + D.cap;
    p.ufstride = ids_max + 2 * ((ids_max + 31) / 32);
    const LdsPlan first = plan_lds(LdsNeeds{D, p.mode, total_words, p.uf_ids_limit, 0u}, W); // (prepare() sizes again from the ops seen by then)
    p.lds_words = first.words; p.lds_ufcap = first.ufcap;
    return ISINGMC_OK;
}
// check_config_model, build_tables and plan_batch for a config that passed check_config: what isingmc_create and isingmc_plan_batch share
static int plan_config(const isingmc_config *cfg, uint32_t lds_bytes, DevBatch &D, Tables &T, BatchPlan &p) {
    if (const int rc = check_config_model(cfg)) return rc;
    D = model_of(cfg);
    T = build_tables(cfg, D);
    D.uniformJ = T.uniformJ; D.wJ = T.wJ; D.wtot = T.wtots[0];
    return plan_batch(plan_inputs(cfg, D, lds_bytes), p);
}

// Apply the plan to the batch, make every allocation and every upload, set the initial state
#define CREATE_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)
template <typename T>
static int copy_up(isingmc_batch *b, T *dst, const T *host, size_t count, const char *what) {
    if (hipMemcpy(dst, host, sizeof(T) * count, hipMemcpyHostToDevice) == hipSuccess) return ISINGMC_OK;
    b->err = std::string(what) + " upload failed";
    return ISINGMC_ENODEVICE;
}
// allocate, copy this host array, or fail with "<what> upload failed"
template <typename T, typename P>
static int upload(isingmc_batch *b, P &dst, const std::vector<T> &host, const char *what) {
    T *q = nullptr;
    CREATE_TRY(dalloc(b, &q, host.size(), false));
    dst = q;
    return copy_up(b, q, host.data(), host.size(), what);
}
static int allocate_and_upload(isingmc_batch *b, const isingmc_config *cfg, const DevBatch &model, Tables &T, const BatchPlan &plan) {
    static_cast<BatchGeometry &>(*b) = plan;
    DevBatch &D = b->dev;
    D = model;
    D.CH = plan.CH; D.nchunks = plan.nchunks; D.stride = plan.stride; D.pm_words = plan.pm_words; D.tbl_stride = plan.tbl_stride; D.lds_ufcap = plan.lds_ufcap;
    b->generic = cfg->interactions != nullptr; b->generic_sym = T.generic_sym;
    b->per_replica_J = D.bond_stride != 0; b->offset = T.offset; b->offsets = std::move(T.offsets);
    const size_t R = D.R;
    CREATE_TRY(dalloc(b, &D.ops, R * D.stride));
    CREATE_TRY(dalloc(b, &D.state, R * D.nwords));
    CREATE_TRY(dalloc(b, &D.n, R));
    CREATE_TRY(dalloc(b, &D.ntrans, R));
    CREATE_TRY(dalloc(b, &D.cutoff, R));
    CREATE_TRY(dalloc(b, &D.err, R));
    CREATE_TRY(dalloc(b, &D.aux, R));
    CREATE_TRY(dalloc(b, &D.epoch, R));
    CREATE_TRY(dalloc(b, &D.acc, R * 8, true, &b->acc));
    b->acc_rows = D.R;
    std::vector<uint32_t> ident(R);
    for (uint32_t i = 0; i < R; ++i) ident[i] = i;
    CREATE_TRY(dalloc(b, &b->d_acc_row, R));
    CREATE_TRY(copy_up(b, b->d_acc_row, ident.data(), R, "acc_row"));
    D.acc_row = b->d_acc_row;
    CREATE_TRY(dalloc(b, &D.chunks, R * 2 * SSE_MAX_CHUNKS));
    CREATE_TRY(dalloc(b, &D.segs, R * D.stride, false));
    if (b->defer) { // flip bytes start (and stay, beyond every cutoff) zero
        CREATE_TRY(dalloc(b, &D.flipb, R * D.stride));
        CREATE_TRY(dalloc(b, &D.pend, R));
    }
    CREATE_TRY(dalloc(b, &D.dbg, R * 16));
    if (D.bond_stride) CREATE_TRY(upload(b, D.wtot_r, T.wtots, "weight"));
    CREATE_TRY(upload(b, D.edge_w, T.edge_w, "edge table"));
    CREATE_TRY(upload(b, D.edges_compact, T.edges_compact, "edge table"));
    if (is_pm(b)) CREATE_TRY(upload(b, D.pm_signs, T.signs, "sign")); // coupling signs of every bond-table row
    CREATE_TRY(upload(b, D.adj_start, T.adj_start, "adjacency"));
    CREATE_TRY(upload(b, D.adj, T.adj, "adjacency"));
    CREATE_TRY(dalloc(b, &D.uf_scratch, R * plan.ufstride, false));
    if (plan.tbl_stride) CREATE_TRY(dalloc(b, &D.tbl, R * D.tbl_stride));
    CREATE_TRY(dalloc(b, &b->d_beta, R));
    CREATE_TRY(dalloc(b, &b->d_out, R));
    CREATE_TRY(dalloc(b, &b->d_vstate, R * D.nwords));
    CREATE_TRY(dalloc(b, &b->d_ok, R));
    CREATE_TRY(upload(b, D.bonds, T.bonds, "table"));
    CREATE_TRY(upload(b, D.cumw, T.cum, "table"));
    if (b->generic) CREATE_TRY(upload(b, D.mats, T.mats, "matrix"));
    b->bonds_host = std::move(T.bonds); b->mats_host = std::move(T.mats); // (import_ops, tempering)
    CREATE_TRY(copy_up(b, D.cutoff, std::vector<uint32_t>(R, cfg->cutoff0).data(), R, "cutoff"));
    if (hipEventCreate(&b->ev0) != hipSuccess || hipEventCreate(&b->ev1) != hipSuccess) { b->err = "hipEventCreate failed"; return ISINGMC_ENODEVICE; }
    if (cfg->init_state) return isingmc_set_state(b, UINT32_MAX, cfg->init_state);
    hipLaunchKernelGGL(init_state_kernel, dim3(D.R), dim3(64), 0, b->stream, D);
    if (hipDeviceSynchronize() != hipSuccess) { b->err = "init_state_kernel failed"; return ISINGMC_ENODEVICE; }
    return ISINGMC_OK;
}
#undef CREATE_TRY

extern "C" {

int isingmc_interaction_at(const isingmc_interaction *it, const uint8_t *inputs, const uint8_t *outputs, double *out) {
    if (!it || !it->mat || !inputs || !outputs || !out || it->nvars == 0 || it->nvars > 2) return ISINGMC_EINVAL;
    // index_from_state (qmc_runner.rs:666-679): outputs then inputs, first variable most significant
    uint32_t iin = 0, iout = 0;
    for (uint32_t k = 0; k < it->nvars; ++k) { iin = (iin << 1) | (inputs[k] ? 1u : 0u); iout = (iout << 1) | (outputs[k] ? 1u : 0u); }
    if (it->diagonal_only) *out = (iin == iout) ? it->mat[iin] : 0.0;
    else *out = it->mat[(iout << it->nvars) | iin];
    return ISINGMC_OK;
}
int isingmc_interaction_sym_under_ising(const isingmc_interaction *it, int *out) {
    if (!it || !it->mat || !out || it->nvars == 0 || it->nvars > 2) return ISINGMC_EINVAL;
    const uint32_t n = it->nvars;
    const uint32_t mask = it->diagonal_only ? ((1u << n) - 1u) : ((1u << (2 * n)) - 1u);
    const uint32_t upto = it->diagonal_only ? (1u << (n >> 1)) : (1u << n);
    int sym = 1;
    for (uint32_t i = 0; i < upto; ++i)
        if (!(std::fabs(it->mat[i] - it->mat[(~i) & mask]) < DBL_EPSILON)) sym = 0;
    *out = sym;
    return ISINGMC_OK;
}

// Chunk grid of the per-chunk counters and the row stride of the op-string (and of every per-slot scratch row) for a batch whose
// kernels run with W waves (diagonal launches) and up to Wmax waves (off-diagonal launches) of K slots per lane.
//   CH      chunk size: <= SSE_MAX_CHUNKS chunks cover the capacity, CH a multiple of 256 (= a wave's tile at K = 4, two at K = 2)
//   stride  whole tiles of EITHER geometry (full-tile loads and stores never leave the row) and at least the chunk-rounded
//           capacity + 256: a cluster-scan wave whose chunk range is empty still prefetches one wave-tile at its range start
int isingmc_plan_geometry(uint32_t capacity, uint32_t W, uint32_t K, uint32_t Wmax, uint32_t out[4]) {
    if (!out || capacity == 0 || W == 0 || K == 0 || Wmax < W) return ISINGMC_EINVAL;
    const size_t CH = (((size_t)capacity + SSE_MAX_CHUNKS - 1) / SSE_MAX_CHUNKS + 255) / 256 * 256;
    const size_t nchunks = ((size_t)capacity + CH - 1) / CH;
    const size_t tile = (Wmax % W == 0 ? (size_t)Wmax : (size_t)Wmax * W) * 64 * K; // whole tiles of either launch geometry
    const size_t need1 = ((size_t)capacity + tile - 1) / tile * tile;
    const size_t need2 = ((size_t)capacity + CH - 1) / CH * CH + 256;
    const size_t need = need1 > need2 ? need1 : need2;
    const size_t stride = (need + tile - 1) / tile * tile;
    if (stride > 0xFFFFFFFFull / 4) return ISINGMC_EINVAL; // byte offsets inside a row are 32-bit (row_ld / row_st)
    out[0] = (uint32_t)CH; out[1] = (uint32_t)nchunks; out[2] = (uint32_t)stride; out[3] = (uint32_t)tile;
    return ISINGMC_OK;
}

int isingmc_create(const isingmc_config *cfg, isingmc_batch **out) {
    if (!cfg || !out || cfg->struct_size != sizeof(isingmc_config)) return refuse(ISINGMC_EINVAL, "bad config pointer or struct_size");
    *out = nullptr;
    if (const int rc = check_config(cfg)) return rc;
    int dev = 0, max_lds = 0;
    if (const char *why = probe_device(cfg->device, &dev, &max_lds)) return refuse(ISINGMC_ENODEVICE, why);
    DevBatch model; Tables tables; BatchPlan plan;
    if (const int rc = plan_config(cfg, (uint32_t)max_lds, model, tables, plan)) return rc;
    isingmc_batch *b = new isingmc_batch();
    b->device = dev;
    if (const int rc = allocate_and_upload(b, cfg, model, tables, plan)) { g_create_error = b->err; isingmc_destroy(b); return rc; }
    *out = b;
    return ISINGMC_OK;
}

// The plan isingmc_create would make for cfg on a device whose workgroups have lds_bytes of LDS, or the code and message it would
// refuse cfg with.  Host only: no device is looked for, nothing is allocated.  Slots: include/isingmc_hip.h.
int isingmc_plan_batch(const isingmc_config *cfg, uint32_t lds_bytes, uint32_t out[32]) {
    if (!cfg || !out || cfg->struct_size != sizeof(isingmc_config)) return refuse(ISINGMC_EINVAL, "bad config pointer or struct_size");
    if (const int rc = check_config(cfg)) return rc;
    DevBatch model; Tables tables; BatchPlan p;
    if (const int rc = plan_config(cfg, lds_bytes, model, tables, p)) return rc;
    const uint32_t slots[32] = {p.W, p.K, p.mode, p.W_off, p.Wmax, p.w8_ok, p.CH, p.nchunks, p.stride, p.pm_words, (uint32_t)p.lds_words_pm_diag,
                                (uint32_t)p.lds_words_diag, (uint32_t)p.lds_words_fast, p.fast_diag, p.lean_cluster, p.defer, (uint32_t)p.lds_words_rvb,
                                p.rvb_global, p.rvb_split, p.rvb_main_W, p.tbl_stride, (uint32_t)p.ufstride, (uint32_t)((uint64_t)p.ufstride >> 32),
                                (uint32_t)p.lds_words, p.lds_ufcap, model.nwords, model.Nb};
    std::copy(slots, slots + 32, out);
    return ISINGMC_OK;
}

void isingmc_destroy(isingmc_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    pt_free(b);
    for (hipEvent_t ev : b->evpool) (void)hipEventDestroy(ev);
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    delete b;
}

const char *isingmc_last_error(const isingmc_batch *b) { return b ? b->err.c_str() : g_create_error.c_str(); }

} // extern "C"
