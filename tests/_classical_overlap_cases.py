"""The cases that the overlap tests share (CPU: isingmc_classical_host_pt_run_overlaps, GPU: classical_overlap_kernel), and a numpy
restatement of the measurement (csrc/classical_overlap_rule.h): TemperingRef of _classical_pt_cases, extended by composition with
the two overlaps and their histograms.  Test infrastructure only."""
import functools

import numpy as np

import _classical_cases as cc
import _classical_pt_cases as pc

PAIRINGS = ("temperature", "slot")  # the rule and a wrong one (a test of the test): copies paired by slot index


def pairs_of(ncopies):
    """[(a, b)], a < b, a-major: the order of the pair index p."""
    return [(a, b) for a in range(ncopies) for b in range(a + 1, ncopies)]


class OverlapRef:
    """G = nchains / ncopies groups of `ncopies` consecutive chains of a TemperingRef (`ref`).  A round measures between the round's
    time steps and its swaps, which is the moment TemperingRef enters its tempering step.  pairing "slot" compares the states of equal
    slot index instead of those that hold the same temperature."""

    def __init__(self, edges, biases, seed, betas, nchains, ncopies, replica_offset=0, basic=True, pairing="temperature"):
        assert pairing in PAIRINGS and ncopies >= 2 and nchains % ncopies == 0 and (replica_offset // len(betas)) % ncopies == 0
        self.ref = pc.TemperingRef(edges, biases, seed, betas, nchains, replica_offset, basic=basic)
        self.K, self.G, self.T, self.N, self.E = ncopies, nchains // ncopies, len(betas), len(biases), len(edges)
        self.pairing = pairing
        self.pa, self.pb = (np.array(x, dtype=np.int64) for x in zip(*pairs_of(ncopies)))
        self.P = len(self.pa)
        self.ends = np.array([ab for ab, _ in edges], dtype=np.int64).reshape(-1, 2)
        self.hq = np.zeros((self.G, self.P, self.T, self.N + 1), dtype=np.uint64)
        self.hl = np.zeros((self.G, self.P, self.T, self.E + 1), dtype=np.uint64)
        self.rows = []
        self._swaps = self.ref._tempering_step
        self.ref._tempering_step = self._measure_then_swap

    def _measure_then_swap(self, energy):
        self.rows.append(self.measure())
        self._swaps(energy)

    def measure(self):
        """(Q, QL), int32 [G][P][T] each, of the states as they stand; the histograms gain one count per item."""
        st = self.ref.states().astype(bool).reshape(self.G * self.K, self.T, self.N)
        if self.pairing == "temperature":
            st = np.take_along_axis(st, self.ref.slot_at[:, :, None], axis=1)
        st = st.reshape(self.G, self.K, self.T, self.N)
        d = st[:, self.pa] ^ st[:, self.pb]                                       # [G][P][T][N]
        nq = d.sum(axis=-1)
        nl = (d[..., self.ends[:, 0]] != d[..., self.ends[:, 1]]).sum(axis=-1)  # every entry of the edge list once
        g, p, t = np.meshgrid(np.arange(self.G), np.arange(self.P), np.arange(self.T), indexing="ij")
        np.add.at(self.hq, (g, p, t, nq), np.uint64(1))
        np.add.at(self.hl, (g, p, t, nl), np.uint64(1))
        return (self.N - 2 * nq).astype(np.int32), (self.E - 2 * nl).astype(np.int32)

    def run(self, rounds, steps):
        """dict: energy, magnetization [rounds][C][T] and overlap, link_overlap [rounds][G][P][T]"""
        first = len(self.rows)
        energy, mag = self.ref.run(rounds, steps)
        rows = self.rows[first:]
        shape = (0, self.G, self.P, self.T)
        q = np.stack([r[0] for r in rows]) if rows else np.zeros(shape, dtype=np.int32)
        ql = np.stack([r[1] for r in rows]) if rows else np.zeros(shape, dtype=np.int32)
        return dict(energy=energy, magnetization=mag, overlap=q, link_overlap=ql)


# ---- the parity cases: 6 rounds of 2 KINDS_ALL steps unless said, at replica_offset = K T ----
def _ladder(t, lo=0.1, hi=3.0):
    return [float(b) for b in np.linspace(lo, hi, t)]


def _case(graph, betas, ncopies, chains, rounds=pc.PT_ROUNDS, steps=pc.PT_STEPS, couplings=None, global_tables=False):
    return dict(edges=graph[0], biases=graph[1], betas=[float(b) for b in betas], ncopies=ncopies, chains=chains, rounds=rounds, steps=steps,
                couplings=couplings, global_tables=global_tables)


def _k8_two_realisations():
    """k8, two groups of two copies, each group on its own realisation: the rows of a group are equal, the groups differ."""
    edges, _ = cc.CASES["k8"]
    js = np.array([j for _, j in edges], dtype=np.float64)
    rows = np.stack([js, -js[::-1]])  # (dyadic: every sum stays exact)
    return np.ascontiguousarray(np.repeat(rows, 2 * 2, axis=0))  # [G = 2] x (K = 2 chains x T = 2 slots)


def _cases():
    rnd = cc.RANDOM_CASES["random129x4"]
    c = {}
    c["k8_T2_K2"] = _case(cc.CASES["k8"], [0.3, 1.0], 2, 2)                              # one item: the smallest launch
    c["ring33_T3_K2"] = _case(cc.CASES["ring33"], [0.2, 0.7, 1.5], 2, 4)                 # one live bit in the last word; 6 items: a half-empty second workgroup
    c["ring64_T2_K2"] = _case(cc.CASES["ring64"], [0.3, 0.4], 2, 2)                      # the last word is full: the unmasked branch
    c["ring65_T3_K3"] = _case(cc.CASES["ring65"], [0.2, 0.7, 1.5], 3, 6)                 # three pairs a group; 65 edges: a second trip of the edge loop with one live lane
    c["random129x4_T4_K2"] = _case((rnd["edges"], rnd["biases"]), [0.2, 0.5, 1.0, 2.0], 2, 4)  # multi-edges, variables without an edge
    c["duplicate_edge_T4_K2"] = _case(cc.CASES["duplicate_edge"], [0.2, 0.5, 1.0, 2.0], 2, 4)  # multi-edges count apiece
    c["lattice4x4_T8_K2"] = _case(cc.CASES["lattice4x4"], _ladder(8, 0.1, 1.0), 2, 4)
    c["lattice4x4_T8_K2_global"] = _case(cc.CASES["lattice4x4"], _ladder(8, 0.1, 1.0), 2, 4, global_tables=True)  # the steps launch's table placement does not matter
    c["ring33_T65_K2"] = _case(cc.CASES["ring33"], _ladder(65), 2, 2)                    # 65 items
    c["ring2081_T2_K2"] = _case(cc._ring(2081, 2081), [0.3, 0.31], 2, 2)                 # 66 state words: a second trip of the word loop
    c["ring65537_T2_K2"] = _case(cc._ring(65537, 65537), [0.3, 1.0], 2, 2, rounds=2, steps=0)  # the two-word edge format; steps = 0 keeps the host run cheap
    c["k8_per_replica_T2_K2"] = _case(cc.CASES["k8"], [0.3, 1.0], 2, 4, couplings=_k8_two_realisations())  # each group on its own realisation
    return c


CASES = _cases()
SERIES = ("energy", "magnetization", "overlap", "link_overlap")
HISTS = ("overlap_hist", "link_hist")
STATE = ("states", "epochs", "temp_of", "pt_step", "counters", "attempts", "accepts")


def offset(name):
    """The replica offset of a parity case: one group's worth, K T, so that the global group indices start at 1."""
    return CASES[name]["ncopies"] * len(CASES[name]["betas"])


def host_run(cl, edges, biases, betas, chains, ncopies, rounds, steps, replica_offset=0, **kw):
    """host_tempering_run with `ncopies` from the random initial states."""
    init = pc.initial_states(cc.SEED, chains * len(betas), len(biases), replica_offset)
    return cl.host_tempering_run(edges, biases, cc.SEED, init, 0, betas, rounds, steps, replica_offset=replica_offset, ncopies=ncopies, **kw)


@functools.lru_cache(maxsize=None)
def host_parity_reference(name):
    """The parity run of a case through isingmc_classical_host_pt_run_overlaps.  Cached; callers do not write into it."""
    import isingmontecarlo_amd.classical as cl
    c = CASES[name]
    return host_run(cl, c["edges"], c["biases"], c["betas"], c["chains"], c["ncopies"], c["rounds"], c["steps"], replica_offset=offset(name), kinds=cl.KINDS_ALL,
                    couplings=c["couplings"])


def restatement_run(name):
    """The parity run of a case on OverlapRef: (dict of the four series, hq, hl).  A case with per-replica couplings is one OverlapRef
    per group, each on its own realisation at its own replica offset (groups share nothing)."""
    c = CASES[name]
    t, k = len(c["betas"]), c["ncopies"]
    if c["couplings"] is None:
        groups = [(c["edges"], c["chains"], offset(name))]
    else:
        groups = [([(ab, float(j)) for (ab, _), j in zip(c["edges"], c["couplings"][g * k * t])], k, offset(name) + g * k * t) for g in range(c["chains"] // k)]
    refs = [OverlapRef(e, c["biases"], cc.SEED, c["betas"], n, k, off, basic=False) for e, n, off in groups]
    outs = [r.run(c["rounds"], c["steps"]) for r in refs]
    return ({key: np.concatenate([o[key] for o in outs], axis=1) for key in SERIES}, np.concatenate([r.hq for r in refs]), np.concatenate([r.hl for r in refs]))


# ---- exact enumeration: G = 1024 groups of 2 copies under the ladder of the tempering tests, the last round's overlaps ----
ENUM_GROUPS = pc.ENUM_PT_CHAINS // 2


def exact_overlap_moments(edges, biases, beta):
    """Boltzmann mean and standard deviation of one sample of Q^2 / N^2 and of QL for two independent copies, by enumerating the pairs
    of states (N <= ~10): {"q2": (mean, sd), "ql": (mean, sd)}."""
    n = len(biases)
    states = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(bool)
    spin = np.where(states, 1.0, -1.0)
    en = np.zeros(1 << n)
    for (a, b), j in edges:
        en += j * spin[:, a] * spin[:, b]
    en += -(spin * np.asarray(biases, dtype=np.float64)[None, :]).sum(axis=1)
    w = np.exp(-beta * (en - en.min()))
    w /= w.sum()
    ww = w[:, None] * w[None, :]
    link = np.stack([spin[:, a] * spin[:, b] for (a, b), _ in edges], axis=1)
    out = {}
    for key, x in (("q2", (spin @ spin.T) ** 2 / float(n * n)), ("ql", link @ link.T)):
        mean = float((ww * x).sum())
        out[key] = (mean, float(np.sqrt(max((ww * (x - mean) ** 2).sum(), 0.0))))
    return out


def enum_overlap_sigmas(name, overlap, link_overlap):
    """The miss of the sampled means of Q^2 / N^2 and QL over the groups, in exact standard deviations over sqrt(G), per temperature:
    [(sigmas of q2, sigmas of ql)].  overlap, link_overlap: [G][T] of one round (one sample per group: groups are independent)."""
    edges, biases = cc.ENUM_SYSTEMS[name]
    n = len(biases)
    out = []
    for t, bj in enumerate(pc.ENUM_PT_BETAJ):
        exact = exact_overlap_moments(edges, biases, cc.enum_beta(name, bj))
        got = {"q2": (overlap[:, t].astype(np.float64) / n) ** 2, "ql": link_overlap[:, t].astype(np.float64)}
        out.append(tuple(float(abs(got[k].mean() - exact[k][0]) / (exact[k][1] / np.sqrt(len(got[k])))) for k in ("q2", "ql")))
    return out
