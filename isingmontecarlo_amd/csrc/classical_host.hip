// classical_host.hip — the device-free half of the classical C ABI (include/isingmc_hip.h): the config checks, the graph tables, the
// launch plans (isingmc_classical_plan, isingmc_classical_icm_plan), the argument checks that the attach calls share with the CPU
// entries, and the sequential rule on the CPU: isingmc_classical_host_steps, the rounds of isingmc_classical_host_pt_run,
// isingmc_classical_host_pt_run_overlaps and isingmc_classical_host_pt_run_icm, and isingmc_classical_host_icm_cluster.  Every GPU
// parity test compares against these entries bit for bit.  Plain C++: no call of the HIP runtime, no launcher, no handle.  The rules are
// classical_rule.h, classical_pt_rule.h, classical_overlap_rule.h and classical_icm_rule.h.
#include "classical_host.h"
#include "classical_icm_rule.h"
#include "classical_overlap_rule.h"
#include "classical_pt_rule.h"

#include <cmath>
#include <cstring>
#include <map>

using namespace sse;

static_assert(ISINGMC_CLASSICAL_KINDS_ALL == CMC_KINDS_ALL && ISINGMC_CLASSICAL_KINDS_BASIC == CMC_KINDS_BASIC && ISINGMC_CLASSICAL_KINDS_SPIN == CMC_KINDS_SPIN &&
              ISINGMC_CLASSICAL_KINDS_EDGE == CMC_KINDS_EDGE && ISINGMC_CLASSICAL_KINDS_WORM == CMC_KINDS_WORM &&
              ISINGMC_CLASSICAL_KINDS_WORM_NO_DOUBLES == CMC_KINDS_WORM_NO_DOUBLES, "the header's kinds are the rule's");

static thread_local std::string g_classical_error;
int cmc_refuse(int rc, const std::string &why) { g_classical_error = why; return rc; }
const char *cmc_last_refusal() { return g_classical_error.c_str(); }

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
    H = CmcHostTables{};
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
    if (cfg->biases && std::any_of(cfg->biases, cfg->biases + N, [](double h) { return h != 0.0; })) {
        H.flags |= CMC_T_BIAS;
        H.bias.assign(cfg->biases, cfg->biases + N);
    }
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

// ---- the launch plans ----
int cmc_plan_config(const isingmc_classical_config *cfg, uint32_t lds_bytes, CmcHostTables &H, CmcCarve &C) {
    if (const int rc = cmc_check_config(cfg)) return rc;
    cmc_build_tables(cfg, H);
    const size_t total_words = lds_bytes / 4;
    C = cmc_plan(H.view(), total_words, ((cfg->flags & ISINGMC_CLASSICAL_CFG_GLOBAL_TABLES) ? (uint32_t)CMC_FORCE_GLOBAL : 0u) |
                                            ((cfg->flags & ISINGMC_CLASSICAL_CFG_GLOBAL_CODES) ? (uint32_t)CMC_FORCE_GLOBAL_CODES : 0u));
    if (C.W != 0u) return ISINGMC_OK;
    return cmc_refuse(ISINGMC_ENOTIMPL, "model too large: the state bits and move stamps of one replica exceed LDS (at most " + std::to_string(cmc_max_vars(total_words)) +
                                            " variables in " + std::to_string(lds_bytes) + " bytes)");
}

void cmc_plan_slots(const CmcCarve &C, uint32_t table_flags, uint32_t out[8]) {
    const uint32_t format = !(table_flags & CMC_T_PER_REPLICA) ? 0u : (table_flags & CMC_T_COMPACT) ? 1u : 2u;
    const uint32_t slots[8] = {C.W, C.in_lds, C.words, C.wave_words + (C.o_jcode != CMC_NONE ? C.code_words : 0u), C.has, (table_flags & CMC_T_COMPACT) ? 1u : 0u,
                               (table_flags & CMC_T_EDGE16) ? 1u : 0u, format};
    std::copy(slots, slots + 8, out);
}

void cmc_icm_plan_slots(const CmcIcmCarve &C, uint32_t lds_bytes, uint32_t out[4]) {
    out[0] = C.W; out[1] = C.words; out[2] = C.wave_words; out[3] = cmc_icm_max_vars(lds_bytes / 4u);
}

std::string cmc_icm_too_large(uint32_t lds_bytes) {
    return "model too large for cluster moves: the three bit sets of one item exceed LDS (at most " + std::to_string(cmc_icm_max_vars(lds_bytes / 4u)) + " variables in " +
           std::to_string(lds_bytes) + " bytes)";
}

// ---- the argument checks ----
int cmc_check_pt_args(uint32_t R, uint32_t replica_offset, uint32_t ntemps, const double *betas, std::string &why) {
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
int cmc_check_pt_couplings(const CmcHostTables &H, uint32_t R, uint32_t ntemps, std::string &why) {
    const uint32_t c = H.first_mixed_chain(R, ntemps);
    if (c == CMC_NONE) return ISINGMC_OK;
    why = "tempering needs one set of couplings per chain: the coupling rows of chain " + std::to_string(c) + " (replicas " + std::to_string(c * ntemps) + " .. " +
          std::to_string(c * ntemps + ntemps - 1u) + ") differ; tempering between different graphs is not built";
    return ISINGMC_EINVAL;
}

static const char *const kNeedCopies = "overlaps need ncopies >= 2 (copies of one realisation are compared in pairs)";
int cmc_check_overlap_args(const CmcHostTables &H, uint32_t R, uint32_t replica_offset, uint32_t T, uint32_t K, CmcOvShape &S, std::string &why) {
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

int cmc_check_icm_window(uint32_t T, uint32_t &t_first, uint32_t &t_last, std::string &why) {
    if (t_last == 0u) t_last = T;
    if (t_last > T) { why = "cluster moves: t_last = " + std::to_string(t_last) + " exceeds the " + std::to_string(T) + " temperatures of the ladder"; return ISINGMC_EINVAL; }
    if (t_first >= t_last) { why = "cluster moves need a window t_first < t_last: [" + std::to_string(t_first) + ", " + std::to_string(t_last) + ") is empty or reversed"; return ISINGMC_EINVAL; }
    return ISINGMC_OK;
}

// ---- the sequential rule ----
// a replica's state as bytes, with the marks of the worm next to them (a reader of the state leaves the marks alone)
struct CmcHostState {
    uint8_t *s, *mark;
    bool get(uint32_t v) const { return s[v] != 0; }
    void flip(uint32_t v) { s[v] ^= 1u; mark[v] ^= 1u; }
    bool marked(uint32_t v) const { return mark[v] != 0; }
    void unmark(uint32_t v) { mark[v] = 0; }
};
// t time steps, and the move counts of one as the launches resolve them (CMC_NONE: the reference's default for the graph of H)
struct CmcHostSteps { uint64_t t; uint32_t nspin, nedge, nworm, kinds; };

// The steps A of replica r of cfg's batch at beta: s is its state [N] with zeroed marks, *epoch is advanced, ctr [8] is added to (or null)
static void replica_steps(const isingmc_classical_config *cfg, const CmcHostTables &H, uint32_t r, const CmcHostSteps &A, double beta, CmcHostState s, uint64_t *epoch,
                          uint64_t *ctr) {
    uint64_t unread[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!ctr) ctr = unread;
    const CmcGraphMem g = cmc_graph_mem(H.view(), r);
    CmcHostDraw draw{(uint32_t)cfg->seed, (uint32_t)(cfg->seed >> 32), cfg->replica_offset + r, 0u, 0u};
    for (uint64_t step = 0; step < A.t; ++step, ++*epoch) {
        draw.epoch_lo = (uint32_t)*epoch; draw.epoch_hi24 = (uint32_t)(*epoch >> 32) & 0xFFFFFFu;
        const uint32_t kind = cmc_step_kind(A.kinds, draw);
        if (kind == 2u) {
            uint32_t ndraw = 0;
            for (uint32_t i = 0; i < A.nworm; ++i) cmc_worm(g, s, beta, A.kinds != CMC_KINDS_WORM_NO_DOUBLES, draw, &ndraw, ctr);
            continue;
        }
        const uint32_t n = kind == 0u ? A.nspin : A.nedge;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t choice = draw(SSE_TAG_CLASSICAL, cmc_index_move(i), 0), uword = draw(SSE_TAG_CLASSICAL, cmc_index_move(i), 1);
            uint32_t a, b = CMC_NONE;
            if (kind == 0u) a = cmc_range(choice, H.N); else g.edge(cmc_pick_edge(g, choice), a, b);
            const double de = kind == 0u ? cmc_spin_de(g, s, a) : cmc_edge_de(g, s, a, b);
            const bool acc = cmc_should_flip(beta, de, uword);
            if (acc) { s.s[a] ^= 1u; if (kind == 1u) s.s[b] ^= 1u; }
            ctr[kind == 0u ? CMC_C_SPIN : CMC_C_EDGE] += 1;
            ctr[kind == 0u ? CMC_C_SPIN_ACC : CMC_C_EDGE_ACC] += acc ? 1u : 0u;
        }
    }
}

// The cluster of the rank-th differing variable of the states a and b ([N] bytes) into mark ([N], zeroed on entry), rank =
// rank_of(nq) of the nq > 0 variables that differ; diff and stack are [N] scratch.  Returns its size, or 0 when fewer than rank + 1
// variables differ.
template <class Rank>
static uint32_t host_cluster(const CmcGraphMem &g, const uint8_t *a, const uint8_t *b, Rank rank_of, uint8_t *diff, uint8_t *mark, uint32_t *stack) {
    uint32_t nq = 0;
    for (uint32_t v = 0; v < g.N(); ++v) { diff[v] = (a[v] != 0) != (b[v] != 0) ? 1u : 0u; nq += diff[v]; }
    const uint32_t rank = nq ? rank_of(nq) : 0u;
    return rank < nq ? cmc_icm_grow(g, diff, rank, mark, stack) : 0u;
}

// One run of the CPU rounds, as the three isingmc_classical_host_pt_run* entries describe it (include/isingmc_hip.h has the shapes):
// the rounds r on the batch of cfg, in the entries' own order, so that an entry initialises the struct from its arguments.  counters,
// every pointer below it and every series of r may be null: that output is not written.
struct CmcHostRun {
    CmcRounds r;
    const isingmc_classical_config *cfg;
    uint32_t ntemps;
    const double *betas;                     // the ladder
    uint8_t *states;                         // in and out: [R][N]
    uint64_t *epochs;                        // [R]
    uint32_t *temp_of;                       // [R]
    uint64_t *pt_step;
    uint64_t *counters, *attempts, *accepts; // added to: [R][8], [C][T - 1]
    uint32_t ncopies = 0;                    // copies a group; 0: the batch has no groups
    uint64_t *hq = nullptr, *hl = nullptr;   // the histograms, added to
    uint32_t t_first = 0, t_last = 0;        // the window of the cluster moves
    uint64_t *moves = nullptr, *empty = nullptr, *size_sum = nullptr; // their counts, added to
};

// what the rounds of one run share: the run (its window resolved), the tables, the maps and energies by slot, the scratch
struct HostRounds {
    CmcHostRun &a;
    CmcHostTables H;
    CmcOvShape ov{}; // ncopies = 0: no groups, no items
    std::vector<uint32_t> slot_at, stack;
    std::vector<double> energy;
    std::vector<uint8_t> mark, diff, cluster;
    explicit HostRounds(CmcHostRun &run) : a(run) {}

    uint8_t *bytes(uint32_t i) const { return a.states + (size_t)i * H.N; }
    CmcHostState state(uint32_t i) { return CmcHostState{bytes(i), mark.data()}; }
    uint32_t slot(uint32_t grp, uint32_t copy, uint32_t t) const { return cmc_ov_slot(slot_at.data(), a.ntemps, grp * ov.K + copy, t); }

    // E and M of slot i as they stand: what the round's swaps see and its rows of the series hold
    void record(uint64_t round, uint32_t i) {
        const CmcGraphMem g = cmc_graph_mem(H.view(), i);
        energy[i] = cmc_pt_energy(g, state(i));
        const size_t at = ((size_t)round * a.cfg->nreplicas + i) - i % a.ntemps + a.temp_of[i];
        if (a.r.energy_out) a.r.energy_out[at] = energy[i];
        if (a.r.mag_out) a.r.mag_out[at] = cmc_pt_magnetization(g, state(i));
    }

    void steps(uint64_t round) {
        const CmcHostSteps A{a.r.steps, cmc_default_moves(a.r.nspin, H.N / 2u), cmc_default_moves(a.r.nedge, H.E / 2u), cmc_default_moves(a.r.nworm, 1u), a.r.kinds};
        for (uint32_t i = 0; i < a.cfg->nreplicas; ++i) {
            replica_steps(a.cfg, H, i, A, a.betas[a.temp_of[i]], state(i), &a.epochs[i], a.counters ? a.counters + (size_t)i * 8 : nullptr);
            record(round, i);
        }
    }

    void measure(uint64_t round) { // after the steps, before the swaps: the maps still say where every temperature is
        for (uint64_t item = 0; item < ov.items; ++item) {
            uint32_t grp, p, t, ca, cb;
            cmc_ov_item(item, ov.P, a.ntemps, grp, p, t);
            cmc_ov_pair(ov.K, p, ca, cb);
            const uint32_t ra = slot(grp, ca, t);
            const CmcHostState A = state(ra), B = state(slot(grp, cb, t));
            const uint32_t nq = cmc_ov_count_spins(H.N, A, B, 0u, 1u), nl = cmc_ov_count_links(cmc_graph_mem(H.view(), ra), A, B, 0u, 1u);
            if (a.r.q_out) a.r.q_out[(size_t)round * ov.items + item] = cmc_ov_overlap(H.N, nq);
            if (a.r.ql_out) a.r.ql_out[(size_t)round * ov.items + item] = cmc_ov_overlap(H.E, nl);
            if (a.hq) a.hq[(size_t)item * ((size_t)H.N + 1u) + nq] += 1u;
            if (a.hl) a.hl[(size_t)item * ((size_t)H.E + 1u) + nl] += 1u;
        }
    }

    void cluster_moves(uint64_t round) { // behind the measurement
        const uint32_t T = a.ntemps, M = cmc_icm_pairs(ov.K);
        for (uint64_t item = 0, items = (uint64_t)ov.G * M * (a.t_last - a.t_first); item < items; ++item) {
            uint32_t grp, p, t, ca, cb, c[4];
            cmc_icm_item(item, M, a.t_first, a.t_last, grp, p, t);
            cmc_icm_pair(ov.K, *a.pt_step, p, ca, cb);
            const uint32_t ra = slot(grp, ca, t), rb = slot(grp, cb, t);
            cmc_icm_counter(T, *a.pt_step, (a.cfg->replica_offset / T + grp * ov.K) / ov.K, p, t, c);
            const uint32_t word = CmcHostDraw{(uint32_t)a.cfg->seed, (uint32_t)(a.cfg->seed >> 32), c[2], c[1], c[3] & 0xFFFFFFu}(c[3] >> 24, c[0], 0);
            uint8_t *A = bytes(ra), *B = bytes(rb);
            const uint32_t size = host_cluster(cmc_graph_mem(H.view(), ra), A, B, [&](uint32_t nq) { return cmc_range(word, nq); }, diff.data(), cluster.data(), stack.data());
            const size_t at = cmc_icm_count_index(M, T, grp, p, t);
            if (size == 0u) { if (a.empty) a.empty[at] += 1u; continue; }
            if (a.moves) a.moves[at] += 1u;
            if (a.size_sum) a.size_sum[at] += size;
            for (uint32_t v = 0; v < H.N; ++v)
                if (cluster[v]) { A[v] = A[v] ? 0u : 1u; B[v] = B[v] ? 0u : 1u; cluster[v] = 0u; }
            record(round, ra); // E and M of the round are those the swaps see: after the moves
            record(round, rb);
        }
    }

    void swaps() {
        const uint32_t T = a.ntemps;
        for (uint32_t c = 0; c < a.cfg->nreplicas / T; ++c) {
            const size_t base = (size_t)c * T, cbase = (size_t)c * (T - 1u);
            const CmcPtChainView cv{T, a.betas, a.temp_of + base, slot_at.data() + base, energy.data() + base, a.attempts ? a.attempts + cbase : nullptr,
                                    a.accepts ? a.accepts + cbase : nullptr};
            cmc_pt_chain_step(a.cfg->seed, *a.pt_step, a.cfg->replica_offset / T + c, cv, PtHostDraw{});
        }
    }
};

// The rounds of isingmc_classical_host_pt_run, isingmc_classical_host_pt_run_overlaps and isingmc_classical_host_pt_run_icm.  The
// checks come in the order of the attach calls: the ladder, the batch, the couplings, the groups, the window (resolved in a).
static int host_rounds(CmcHostRun a) {
    if (const int rc = cmc_check_config(a.cfg)) return rc;
    std::string why;
    if (const int rc = cmc_check_pt_args(a.cfg->nreplicas, a.cfg->replica_offset, a.ntemps, a.betas, why)) return cmc_refuse(rc, why);
    if (!a.states || !a.epochs || !a.temp_of || !a.pt_step) return cmc_refuse(ISINGMC_EINVAL, "states, epochs, temp_of and pt_step must be non-null");
    if (a.r.kinds >= CMC_KINDS_COUNT) return cmc_refuse(ISINGMC_EINVAL, "kinds must be one of ISINGMC_CLASSICAL_KINDS_*");
    const uint32_t R = a.cfg->nreplicas, T = a.ntemps;
    std::vector<uint8_t> seen(T);
    if (!cmc_pt_is_permutation(a.temp_of, R, T, seen.data())) return cmc_refuse(ISINGMC_EINVAL, "temp_of must be a permutation of the temperatures within every chain");
    HostRounds c(a);
    cmc_build_tables(a.cfg, c.H);
    if (const int rc = cmc_check_pt_couplings(c.H, R, T, why)) return cmc_refuse(rc, why);
    if (a.ncopies != 0u)
        if (const int rc = cmc_check_overlap_args(c.H, R, a.cfg->replica_offset, T, a.ncopies, c.ov, why)) return cmc_refuse(rc, why);
    if (a.r.cluster_moves) {
        if (a.ncopies == 0u) return cmc_refuse(ISINGMC_EINVAL, "cluster moves need ncopies >= 2 (they exchange clusters between the copies of a group)");
        if (const int rc = cmc_check_icm_window(T, a.t_first, a.t_last, why)) return cmc_refuse(rc, why);
        c.diff.resize(c.H.N); c.cluster.assign(c.H.N, 0); c.stack.resize(c.H.N);
    }
    c.mark.assign(c.H.N, 0); c.slot_at.resize(R); c.energy.resize(R);
    for (uint32_t i = 0; i < R; ++i) c.slot_at[i - i % T + a.temp_of[i]] = i % T;
    for (uint64_t round = 0; round < a.r.rounds; ++round, ++*a.pt_step) {
        c.steps(round);
        if (a.r.overlaps) c.measure(round);
        if (a.r.cluster_moves) c.cluster_moves(round);
        c.swaps();
    }
    return ISINGMC_OK;
}

extern "C" {

int isingmc_classical_plan(const isingmc_classical_config *cfg, uint32_t lds_bytes, uint32_t out[8]) {
    if (!out) return cmc_refuse(ISINGMC_EINVAL, "null output");
    CmcHostTables H; CmcCarve C;
    if (const int rc = cmc_plan_config(cfg, lds_bytes, H, C)) return rc;
    cmc_plan_slots(C, H.flags, out);
    return ISINGMC_OK;
}

int isingmc_classical_icm_plan(uint32_t nvars, uint32_t lds_bytes, uint32_t out[4]) {
    if (!out) return cmc_refuse(ISINGMC_EINVAL, "null output");
    if (nvars == 0u || nvars > CMC_MAX_VARS) return cmc_refuse(ISINGMC_EINVAL, "nvars must be 1 .. 2^24");
    const CmcIcmCarve c = cmc_icm_plan(nvars, lds_bytes / 4u);
    if (c.W == 0u) return cmc_refuse(ISINGMC_ENOTIMPL, cmc_icm_too_large(lds_bytes));
    cmc_icm_plan_slots(c, lds_bytes, out);
    return ISINGMC_OK;
}

int isingmc_classical_host_steps(const isingmc_classical_config *cfg, uint64_t t, const double *beta, uint32_t nspin, uint32_t nedge,
                                 uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint64_t *counters) {
    if (const int rc = cmc_check_config(cfg)) return rc;
    if (!beta || !states || !epochs) return cmc_refuse(ISINGMC_EINVAL, "beta, states and epochs must be non-null");
    if (kinds >= CMC_KINDS_COUNT) return cmc_refuse(ISINGMC_EINVAL, "kinds must be one of ISINGMC_CLASSICAL_KINDS_*");
    CmcHostTables H;
    cmc_build_tables(cfg, H);
    const CmcHostSteps A{t, cmc_default_moves(nspin, H.N / 2u), cmc_default_moves(nedge, H.E / 2u), cmc_default_moves(nworm, 1u), kinds};
    std::vector<uint8_t> mark(H.N, 0);
    for (uint32_t r = 0; r < cfg->nreplicas; ++r)
        replica_steps(cfg, H, r, A, beta[r], CmcHostState{states + (size_t)r * H.N, mark.data()}, &epochs[r], counters ? counters + (size_t)r * 8 : nullptr);
    return ISINGMC_OK;
}

int isingmc_classical_host_pt_run(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint64_t rounds, uint64_t steps,
                                  uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                                  uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out) {
    return host_rounds(CmcHostRun{CmcRounds{rounds, steps, nspin, nedge, nworm, kinds, energy_out, mag_out}, cfg, ntemps, betas, states, epochs, temp_of, pt_step,
                                  counters, attempts, accepts});
}

int isingmc_classical_host_pt_run_overlaps(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint32_t ncopies, uint64_t rounds, uint64_t steps,
                                           uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                                           uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out,
                                           int32_t *q_out, int32_t *ql_out, uint64_t *hq, uint64_t *hl) {
    if (const int rc = cmc_check_config(cfg)) return rc;
    if (ncopies == 0u) return cmc_refuse(ISINGMC_EINVAL, kNeedCopies); // (before the ladder's refusals: host_rounds takes 0 as "no groups")
    CmcHostRun a{CmcRounds{rounds, steps, nspin, nedge, nworm, kinds, energy_out, mag_out, q_out, ql_out}, cfg, ntemps, betas, states, epochs, temp_of, pt_step,
                 counters, attempts, accepts, ncopies, hq, hl};
    a.r.overlaps = true;
    return host_rounds(a);
}

int isingmc_classical_host_pt_run_icm(const isingmc_classical_config *cfg, uint32_t ntemps, const double *betas, uint32_t ncopies, uint64_t rounds, uint64_t steps,
                                      uint32_t nspin, uint32_t nedge, uint32_t nworm, uint32_t kinds, uint8_t *states, uint64_t *epochs, uint32_t *temp_of,
                                      uint64_t *pt_step, uint64_t *counters, uint64_t *attempts, uint64_t *accepts, double *energy_out, int32_t *mag_out,
                                      int32_t *q_out, int32_t *ql_out, uint64_t *hq, uint64_t *hl, uint32_t measure, uint32_t t_first, uint32_t t_last,
                                      uint64_t *moves, uint64_t *empty, uint64_t *size_sum) {
    CmcHostRun a{CmcRounds{rounds, steps, nspin, nedge, nworm, kinds, energy_out, mag_out, q_out, ql_out}, cfg, ntemps, betas, states, epochs, temp_of, pt_step,
                 counters, attempts, accepts, ncopies, hq, hl, t_first, t_last, moves, empty, size_sum};
    a.r.overlaps = measure != 0u; a.r.cluster_moves = true;
    return host_rounds(a);
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
    const uint32_t size = host_cluster(cmc_graph_mem(H.view(), 0u), state_a, state_b, [&](uint32_t) { return rank; }, diff.data(), mask_out, stack.data());
    if (size == 0u) return cmc_refuse(ISINGMC_EINVAL, "rank must be below the number of variables in which the two states differ");
    if (size_out) *size_out = size;
    return ISINGMC_OK;
}

} // extern "C"
