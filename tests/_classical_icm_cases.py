"""The cases that the cluster-move tests share (CPU: isingmc_classical_host_pt_run_icm, GPU: classical_icm_kernel), and a numpy
restatement of a round with isoenergetic cluster moves (csrc/classical_icm_rule.h): IcmRef, built on OverlapRef of
_classical_overlap_cases (its TemperingRef, its measurement), with the moves between the measurement and the swaps.  Also the
transition matrix of one move over all pairs of states of a small system, for the exactness tests.  Test infrastructure only."""
import functools

import numpy as np

import _classical_cases as cc
import _classical_overlap_cases as oc
import _classical_pt_cases as pc
import _classical_reference as CR
import _lattices as lat

TAG_ICM = 10
RULES = ("right", "neighbours", "satisfied")  # the rule and two wrong ones (tests of the test)
COUNTS = ("cluster_moves", "cluster_empty", "cluster_size_sum")
LDS_BYTES = 160 * 1024


def adjacency(edges, nvars):
    """[(neighbour, J)] per variable: every entry of the edge list, both ways."""
    return CR.binding_mat(edges, nvars)


def cluster_mask(adj, d, seed, rule="right", a=None):
    """bool [N]: the cluster of `seed`.  "right": its connected component among the variables with d set, over every entry of the edge
    list.  "neighbours": growth stops at the seed's neighbours.  "satisfied": grown over the satisfied bonds of state `a`
    (J s_i s_j < 0) instead of over d."""
    mask = np.zeros(len(d), dtype=bool)
    mask[seed] = True
    if rule == "neighbours":
        for u, _ in adj[seed]:
            mask[u] |= bool(d[u])
        return mask
    stack = [int(seed)]
    while stack:
        v = stack.pop()
        for u, j in adj[v]:
            ok = bool(d[u]) if rule == "right" else (j * (1.0 if a[v] == a[u] else -1.0) < 0.0)
            if ok and not mask[u]:
                mask[u] = True
                stack.append(u)
    return mask


class IcmRef:
    """OverlapRef (`ov`; its TemperingRef is `ref`) with cluster moves in the window [t_first, t_last) of every round, after the
    measurement (when `measure`) and before the energies that the swaps and the series see.  `states` [R][N] places the initial
    states."""

    def __init__(self, edges, biases, seed, betas, nchains, ncopies, window=(0, None), replica_offset=0, basic=True, measure=True, states=None):
        self.ov = oc.OverlapRef(edges, biases, seed, betas, nchains, ncopies, replica_offset, basic=basic)
        self.ref = self.ov.ref
        self.ref._tempering_step = self.ov._swaps  # round() below measures for itself
        self.K, self.G, self.T, self.N, self.M = ncopies, self.ov.G, self.ov.T, self.ov.N, ncopies // 2
        self.t_first, self.t_last = int(window[0]), self.T if window[1] is None else int(window[1])
        assert 0 <= self.t_first < self.t_last <= self.T
        self.measure, self.seed = measure, int(seed)
        self.group0 = (replica_offset // self.T) // self.K
        self.adj = adjacency(edges, self.N)
        self.moves, self.empty, self.size_sum = (np.zeros((self.G, self.M, self.T), dtype=np.uint64) for _ in range(3))
        if states is not None:
            self._set_states(np.asarray(states).astype(bool).reshape(self.ref.R, self.N))

    def _set_states(self, st, rows=None):
        if self.ref.basic:
            self.ref.batch.state = st.copy()
        else:
            for r in (range(self.ref.R) if rows is None else rows):
                self.ref.reps[r].state = [bool(x) for x in st[r]]

    def cluster_moves(self):
        ref, K, T = self.ref, self.K, self.T
        st = ref.states().astype(bool)
        touched = set()
        o = ref.pt_step % K
        for g in range(self.G):
            for m in range(self.M):
                a, b = (o + 2 * m) % K, (o + 2 * m + 1) % K
                for t in range(self.t_first, self.t_last):
                    ra, rb = ((g * K + c) * T + int(ref.slot_at[g * K + c, t]) for c in (a, b))
                    d = st[ra] ^ st[rb]
                    nq = int(d.sum())
                    if nq == 0:
                        self.empty[g, m, t] += np.uint64(1)
                        continue
                    word = int(CR.philox_np(self.seed, m * T + t, ref.pt_step, self.group0 + g, TAG_ICM)[0])
                    mask = cluster_mask(self.adj, d, np.flatnonzero(d)[(word * nq) >> 32])
                    st[ra] ^= mask
                    st[rb] ^= mask
                    touched.update((ra, rb))
                    self.moves[g, m, t] += np.uint64(1)
                    self.size_sum[g, m, t] += np.uint64(mask.sum())
        self._set_states(st, sorted(touched))

    def round(self, steps):
        ref = self.ref
        beta = ref.betas[ref.temp_of.reshape(-1)]
        if ref.basic:
            ref.batch.timesteps(steps, beta)
        else:
            for g, b in zip(ref.reps, beta):
                g.timesteps(steps, float(b), kinds=CR.KINDS_ALL)
        row = self.ov.measure() if self.measure else None
        self.cluster_moves()
        st = ref.states()
        energy = pc.slot_energies(ref.batch, st).reshape(ref.C, ref.T)
        mag = pc.magnetizations(st).reshape(ref.C, ref.T)
        e_row, m_row = np.take_along_axis(energy, ref.slot_at, axis=1), np.take_along_axis(mag, ref.slot_at, axis=1)
        ref._tempering_step(energy)
        ref.pt_step += 1
        return e_row, m_row, row

    def run(self, rounds, steps):
        """dict: energy, magnetization [rounds][C][T] and, when measuring, overlap, link_overlap [rounds][G][P][T]"""
        rows = [self.round(steps) for _ in range(rounds)]
        out = dict(energy=np.stack([r[0] for r in rows]), magnetization=np.stack([r[1] for r in rows]))
        if self.measure:
            out.update(overlap=np.stack([r[2][0] for r in rows]), link_overlap=np.stack([r[2][1] for r in rows]))
        return out


# ---- the parity cases: 6 rounds of 2 KINDS_ALL steps unless said, at replica_offset = K T ----
def _case(graph, betas, ncopies, chains, window=(0, None), rounds=pc.PT_ROUNDS, steps=pc.PT_STEPS, couplings=None, global_tables=False, states=None, gate=None):
    graph = (None, None) if graph is None else graph  # (a gate case: case() makes its ring)
    return dict(edges=graph[0], biases=graph[1], betas=[float(b) for b in betas], ncopies=ncopies, chains=chains, window=window, rounds=rounds, steps=steps,
                couplings=couplings, global_tables=global_tables, states=states, gate=gate)


def _complete65():
    rng = np.random.default_rng(65)
    edges = lat.complete(65)
    return [(ab, float(j)) for (ab, _), j in zip(edges, cc._dyadic(rng, len(edges)))], [0.0] * 65


def _ring200_states(equal):
    """R = 4 slots: chain 0 (copy a) all zeros, chain 1 (copy b) all ones except variable 0: the differing variables 1 .. 199 are one
    path.  equal: every state all zeros."""
    st = np.zeros((4, 200), dtype=np.uint8)
    if not equal:
        st[2:, 1:] = 1
    return st


def _cases():
    rnd = cc.RANDOM_CASES["random129x4"]
    ring200 = cc._ring(200, 200)
    c = {}
    c["k8_T2_K2"] = _case(cc.CASES["k8"], [0.3, 1.0], 2, 2, window=(0, 1))                  # one item
    c["ring33_T3_K2"] = _case(cc.CASES["ring33"], [0.2, 0.7, 1.5], 2, 4, window=(1, 3))      # one live bit in the last word; the window leaves a temperature out
    c["ring64_T2_K2"] = _case(cc.CASES["ring64"], [0.3, 0.4], 2, 2)                          # a full last word
    c["ring65_T3_K3"] = _case(cc.CASES["ring65"], [0.2, 0.7, 1.5], 3, 6)                     # one pair a round, rotating over 6 rounds, with an idle copy
    c["lattice4x4_T8_K4"] = _case(cc.CASES["lattice4x4"], oc._ladder(8, 0.1, 1.0), 4, 8)     # two pairs a round with alternating partners
    c["lattice4x4_T8_K4_global"] = _case(cc.CASES["lattice4x4"], oc._ladder(8, 0.1, 1.0), 4, 8, global_tables=True)
    c["complete65_T2_K2"] = _case(_complete65(), [0.05, 0.1], 2, 2, rounds=3, steps=0)       # the whole frontier in one pass; all lanes OR into three words
    c["random129x4_T4_K2"] = _case((rnd["edges"], rnd["biases"]), [0.2, 0.5, 1.0, 2.0], 2, 4)  # multi-edges; variables without an edge: a cluster of one
    c["duplicate_edge_T4_K2"] = _case(cc.CASES["duplicate_edge"], [0.2, 0.5, 1.0, 2.0], 2, 4)
    c["ring2081_T2_K2"] = _case(cc._ring(2081, 2081), [0.3, 0.31], 2, 2)                     # 66 state words: a second trip of every word loop
    c["ring200_path_T2_K2"] = _case(ring200, [0.3, 1.0], 2, 2, rounds=2, steps=0, states=_ring200_states(False))  # one cluster of 199 on a path
    c["ring200_equal_T2_K2"] = _case(ring200, [0.3, 1.0], 2, 2, rounds=2, steps=0, states=_ring200_states(True))  # nq = 0: every item empty
    c["ring65537_T2_K2"] = _case(cc._ring(65537, 65537), [0.3, 1.0], 2, 2, rounds=2, steps=0)  # the two-word edge format
    c["ring_past_4_waves_T2_K2"] = _case(None, [0.3, 1.0], 2, 2, rounds=2, steps=0, gate=4)   # the two-wave launch
    c["ring_past_2_waves_T2_K2"] = _case(None, [0.3, 1.0], 2, 2, rounds=2, steps=0, gate=2)   # the one-wave launch
    c["k8_per_replica_T2_K2"] = _case(cc.CASES["k8"], [0.3, 1.0], 2, 4, couplings=oc._k8_two_realisations())  # each group on its own realisation
    c["ring33_T65_K2"] = _case(cc.CASES["ring33"], oc._ladder(65), 2, 2)                     # 65 items a launch
    return c


CASES = _cases()
SERIES = oc.SERIES
HISTS = oc.HISTS
STATE = oc.STATE


@functools.lru_cache(maxsize=None)
def gate(waves):
    """The largest N whose cluster-move launch has `waves` waves a workgroup at 160 KB of LDS, from isingmc_classical_icm_plan."""
    import isingmontecarlo_amd.classical as cl

    def fits(n):
        try:
            return cl.icm_plan(n, LDS_BYTES)["waves"] >= waves
        except cl.IsingMcError:
            return False
    lo, hi = 1, 1 << 24
    assert fits(lo)
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid - 1)
    return lo


@functools.lru_cache(maxsize=None)
def case(name):
    """The case with its graph: a gate case is the ring one variable past the gate.  Callers do not write into it."""
    c = dict(CASES[name])
    if c["gate"] is not None:
        n = gate(c["gate"]) + 1
        c["edges"], c["biases"] = cc._ring(n, n)
    return c


def offset(name):
    """The replica offset of a parity case: one group's worth, K T, so that the global group indices start at 1."""
    return CASES[name]["ncopies"] * len(CASES[name]["betas"])


def initial(c, replica_offset):
    if c["states"] is not None:
        return c["states"]
    return pc.initial_states(cc.SEED, c["chains"] * len(c["betas"]), len(c["biases"]), replica_offset)


def host_run(cl, c, rounds=None, replica_offset=0, measure=True, **kw):
    """host_tempering_run with the cluster moves of case dict `c`, from its initial states."""
    return cl.host_tempering_run(c["edges"], c["biases"], cc.SEED, initial(c, replica_offset), 0, c["betas"], c["rounds"] if rounds is None else rounds, c["steps"],
                                 replica_offset=replica_offset, ncopies=c["ncopies"], cluster_moves=c["window"], kinds=CR.KINDS_ALL, couplings=c["couplings"],
                                 measure=measure, **kw)


@functools.lru_cache(maxsize=None)
def host_parity_reference(name):
    """The parity run of a case through isingmc_classical_host_pt_run_icm.  Cached; callers do not write into it."""
    import isingmontecarlo_amd.classical as cl
    return host_run(cl, case(name), replica_offset=offset(name))


def restatement_run(name):
    """The parity run of a case on IcmRef, as the dict of host_tempering_run (counters only for runs that take steps).  A case with
    per-replica couplings is one IcmRef per group, each on its own realisation at its own replica offset (groups share nothing)."""
    c = case(name)
    t, k = len(c["betas"]), c["ncopies"]
    st = None if c["states"] is None else np.asarray(c["states"])
    if c["couplings"] is None:
        groups = [(c["edges"], c["chains"], offset(name), st)]
    else:
        groups = [([(ab, float(j)) for (ab, _), j in zip(c["edges"], c["couplings"][g * k * t])], k, offset(name) + g * k * t, None) for g in range(c["chains"] // k)]
    refs = [IcmRef(e, c["biases"], cc.SEED, c["betas"], n, k, c["window"], off, basic=c["steps"] == 0, states=s) for e, n, off, s in groups]
    outs = [r.run(c["rounds"], c["steps"]) for r in refs]
    out = {key: np.concatenate([o[key] for o in outs], axis=1) for key in SERIES}
    out.update(overlap_hist=np.concatenate([r.ov.hq for r in refs]), link_hist=np.concatenate([r.ov.hl for r in refs]),
               cluster_moves=np.concatenate([r.moves for r in refs]), cluster_empty=np.concatenate([r.empty for r in refs]),
               cluster_size_sum=np.concatenate([r.size_sum for r in refs]),
               states=np.concatenate([r.ref.states() for r in refs]), epochs=np.concatenate([r.ref.epochs() for r in refs]),
               temp_of=np.concatenate([r.ref.temp_of.reshape(-1) for r in refs]).astype(np.uint32), pt_step=refs[0].ref.pt_step,
               attempts=np.concatenate([r.ref.attempts for r in refs]), accepts=np.concatenate([r.ref.accepts for r in refs]))
    if c["steps"]:
        out["counters"] = np.concatenate([r.ref.counters() for r in refs])
    return out


# ---- exactness of one move: the transition matrix over all pairs of states of a small system ----
# five variables; a frustrated triangle 0-1-2, a multi-edge on (1, 2), a zero coupling on (3, 4), non-zero biases; integers
TINY = ([((0, 1), 8.0), ((1, 2), 8.0), ((2, 0), 8.0), ((2, 3), -4.0), ((3, 4), 0.0), ((4, 0), 6.0), ((1, 2), 4.0)], [2.0, -4.0, 1.0, 0.0, 3.0])
TINY_FLOAT = ([(ab, 0.1 * j) for ab, j in TINY[0]], [0.1 * h for h in TINY[1]])  # the same in tenths: sums round
TINY_BETAS = (0.03, 0.11)


def bits_of(n):
    """bool [2^n][n]: state s has variable v = bit v of s"""
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(bool)


def energies(edges, biases, states):
    """get_energy of states [S][N]"""
    spin = np.where(states, 1.0, -1.0)
    en = np.zeros(len(spin))
    for (a, b), j in edges:
        en += j * spin[:, a] * spin[:, b]
    return en - (spin * np.asarray(biases, dtype=np.float64)[None, :]).sum(axis=1)


def pair_transitions(nvars, cluster):
    """The move as a Markov matrix over the pairs of states (index a * 2^n + b): from (a, b) with nq differing variables, every rank
    k < nq has probability 1 / nq and leads to (a ^ c, b ^ c), c = cluster(a_bits, b_bits, k) (bool [N]); nq = 0 stays.  Also returns
    the list of (pair, rank, mask) it visited."""
    st = bits_of(nvars)
    size = 1 << nvars
    weights = 1 << np.arange(nvars)
    p = np.zeros((size * size, size * size))
    seen = []
    for a in range(size):
        for b in range(size):
            nq = int((st[a] ^ st[b]).sum())
            if nq == 0:
                p[a * size + b, a * size + b] = 1.0
                continue
            for k in range(nq):
                mask = np.asarray(cluster(st[a], st[b], k)).astype(bool)
                c = int((mask * weights).sum())
                p[a * size + b, (a ^ c) * size + (b ^ c)] += 1.0 / nq
                seen.append((a, b, k, mask))
    return p, seen


def product_weight(edges, biases, beta):
    """The Boltzmann weight of two independent copies over the pairs of states, normalised."""
    en = energies(edges, biases, bits_of(len(biases)))
    w = np.exp(-beta * (en - en.min()))
    w /= w.sum()
    return (w[:, None] * w[None, :]).reshape(-1)


def restated_cluster(edges, biases, rule):
    adj = adjacency(edges, len(biases))

    def cluster(a, b, k):
        d = a ^ b
        return cluster_mask(adj, d, np.flatnonzero(d)[k], rule, a)
    return cluster


# ---- exact enumeration under cluster moves: the inputs of the overlap enumeration test, cluster moves at every temperature ----
def enum_icm_sigmas(name, overlap, link_overlap, energy):
    """The miss of the sampled means in exact standard deviations over sqrt(G), per temperature: [(q2, ql, E of copy 0, E of copy 1)].
    overlap, link_overlap [G][T] and energy [C][T] of one round (C = 2 G: chains 2 g and 2 g + 1 are the copies of group g)."""
    edges, biases = cc.ENUM_SYSTEMS[name]
    out = []
    for t, (q2, ql) in enumerate(oc.enum_overlap_sigmas(name, overlap, link_overlap)):
        mean, sd = CR.exact_moments(edges, biases, cc.enum_beta(name, pc.ENUM_PT_BETAJ[t]))["E"]  # the enumeration of exact_overlap_moments, for E
        e = [float(abs(energy[copy::2, t].mean() - mean) / (sd / np.sqrt(len(energy[copy::2, t])))) for copy in (0, 1)]
        out.append((q2, ql, e[0], e[1]))
    return out
