"""The cases that the classical tempering tests share (CPU: isingmc_classical_host_pt_run, GPU: classical_tempering_kernel), and a
numpy restatement of a tempering round (csrc/classical_pt_rule.h) built on _classical_reference: BatchRef or RefGraphState for the
time steps, the project's numpy Philox for the swap stream, and the kernel's order of additions for the energy.  Test
infrastructure only."""
import functools

import numpy as np

import _classical_cases as cc
import _classical_reference as CR

TAG_PT = 6
RULES = ("right", "always", "reversed", "position")  # the rule and three wrong ones (tests of the tests)


def slot_energies(tables, states):
    """get_energy of states [R][N] (bool) in the order of classical_pt_rule.h: lane l of 64 folds e = e + energy_of(v) + bias term
    over v = l, l + 64, ...; a tree over the offsets 32 .. 1 adds p[l] += p[l + o].  `tables`: a BatchRef (its nbr, J, valid, h)."""
    st = np.asarray(states).astype(bool)
    nrep, n = st.shape
    en = np.zeros((nrep, n))
    for k in range(tables.nbr.shape[1]):  # energy_of: row order, from 0.0
        term = tables.J[None, :, k] * np.where(st == st[:, tables.nbr[:, k]], 1.0, -1.0) / 2.0
        en = np.where(tables.valid[None, :, k], en + term, en)
    bias = np.where(st, -tables.h[None, :], tables.h[None, :])
    p = np.zeros((nrep, 64))
    for lo in range(0, n, 64):
        w = min(64, n - lo)
        p[:, :w] = p[:, :w] + en[:, lo:lo + w] + bias[:, lo:lo + w]
    o = 32
    while o:
        p[:, :o] += p[:, o:2 * o]
        o >>= 1
    return p[:, 0].copy()


def magnetizations(states):
    st = np.asarray(states).astype(bool)
    return (2 * st.sum(axis=1) - st.shape[1]).astype(np.int32)


class TemperingRef:
    """C chains of T = len(betas) temperatures, slot r = c T + i, from the random initial states.  basic = True: BatchRef
    (only_basic_moves steps with the default move counts, any R); False: one RefGraphState per slot, KINDS_ALL steps with worms, and
    move counters.  rule: "right", or a wrong one: "always" accepts every swap, "reversed" has the exponent's sign reversed,
    "position" reads the energies by temperature position as they stood before the round's swaps instead of by slot."""

    def __init__(self, edges, biases, seed, betas, nchains, replica_offset=0, basic=True, rule="right"):
        assert rule in RULES
        self.betas = np.asarray(betas, dtype=np.float64)
        self.T, self.C, self.seed, self.rule, self.basic = len(self.betas), int(nchains), int(seed), rule, basic
        self.R = self.T * self.C
        assert replica_offset % self.T == 0
        self.chain = np.arange(self.C, dtype=np.uint64) + np.uint64(replica_offset // self.T)
        self.batch = CR.BatchRef(edges, biases, seed, self.R, replica_offset)
        self.reps = None if basic else [CR.RefGraphState(edges, biases, seed, replica_offset + r) for r in range(self.R)]
        self.temp_of = np.tile(np.arange(self.T, dtype=np.int64), (self.C, 1))  # [C][i]
        self.slot_at = self.temp_of.copy()                                       # [C][t]
        self.pt_step = 0
        self.attempts = np.zeros((self.C, self.T - 1), dtype=np.uint64)
        self.accepts = np.zeros((self.C, self.T - 1), dtype=np.uint64)

    def states(self):
        return self.batch.state.astype(np.uint8) if self.basic else np.stack([g.state_bytes() for g in self.reps])

    def epochs(self):
        return np.full(self.R, self.batch.epoch, dtype=np.uint64) if self.basic else np.array([g.epoch for g in self.reps], dtype=np.uint64)

    def counters(self):
        return np.array([g.counters for g in self.reps], dtype=np.uint64)

    def states_by_temperature(self):
        return np.take_along_axis(self.states().reshape(self.C, self.T, -1), self.slot_at[:, :, None], axis=1)

    def _tempering_step(self, energy):
        """energy [C][i] by slot"""
        rows = np.arange(self.C)
        by_position = np.take_along_axis(energy, self.slot_at, axis=1)  # [C][t] before the round's swaps
        a_first = (CR.philox_np(self.seed, 0, self.pt_step, self.chain, TAG_PT)[:, 0] >> np.uint64(31)).astype(bool)
        for phase in (0, 1):
            first = a_first if phase == 0 else ~a_first
            for parity in (0, 1):  # the pairs of a phase are disjoint: all the even (odd) t of the chains whose phase holds them, at once
                ch = rows[first if parity == 0 else ~first][:, None]
                t = np.arange(parity, self.T - 1, 2)[None, :]
                if not ch.size or not t.size:
                    continue
                u = CR.philox_np(self.seed, 1 + t, self.pt_step, self.chain[ch], TAG_PT)[..., 0].astype(np.float64) * (1.0 / 4294967296.0)
                a, b = self.slot_at[ch, t], self.slot_at[ch, t + 1]
                if self.rule == "position":
                    ea, eb = by_position[ch, t], by_position[ch, t + 1]
                else:
                    ea, eb = energy[ch, a], energy[ch, b]
                x = (self.betas[t] - self.betas[t + 1]) * (ea - eb)
                with np.errstate(over="ignore"):
                    acc = np.exp(-x if self.rule == "reversed" else x) > u
                if self.rule == "always":
                    acc = np.ones(acc.shape, dtype=bool)
                self.attempts[ch, t] += np.uint64(1)
                cs, ts = np.broadcast_to(ch, acc.shape)[acc], np.broadcast_to(t, acc.shape)[acc]
                self.slot_at[cs, ts], self.slot_at[cs, ts + 1] = b[acc], a[acc]
                self.temp_of[cs, a[acc]], self.temp_of[cs, b[acc]] = ts + 1, ts
                self.accepts[cs, ts] += np.uint64(1)

    def round(self, steps):
        """One round; returns (energy [C][T], magnetization [C][T]) by temperature, before the round's swaps."""
        beta = self.betas[self.temp_of.reshape(-1)]
        if self.basic:
            self.batch.timesteps(steps, beta)
        else:
            for g, b in zip(self.reps, beta):
                g.timesteps(steps, float(b), kinds=CR.KINDS_ALL)
        st = self.states()
        energy = slot_energies(self.batch, st).reshape(self.C, self.T)
        mag = magnetizations(st).reshape(self.C, self.T)
        e_row, m_row = np.take_along_axis(energy, self.slot_at, axis=1), np.take_along_axis(mag, self.slot_at, axis=1)
        self._tempering_step(energy)
        self.pt_step += 1
        return e_row, m_row

    def run(self, rounds, steps):
        rows = [self.round(steps) for _ in range(rounds)]
        return np.stack([e for e, _ in rows]), np.stack([m for _, m in rows])


# ---- the parity cases: 6 rounds of 2 KINDS_ALL steps each (so that worms occur) ----
PT_ROUNDS, PT_STEPS = 6, 2


def _ladder(t, lo=0.1, hi=3.0):
    return [float(b) for b in np.linspace(lo, hi, t)]


def _pt_case(graph, betas, chains):
    return dict(edges=graph[0], biases=graph[1], betas=[float(b) for b in betas], chains=chains)


def _pt_cases():
    ring300 = cc.LAYOUT_CASES["ring300_distinct"]
    c = {}
    c["k8_T2"] = _pt_case(cc.CASES["k8"], [0.3, 1.0], 1)                      # the smallest batch
    c["ring65_T3"] = _pt_case(cc.CASES["ring65"], [0.2, 0.7, 1.5], 3)         # odd T; R = 9 leaves empty waves in the last steps workgroup
    c["lattice4x4_T8"] = _pt_case(cc.CASES["lattice4x4"], _ladder(8, 0.1, 1.0), 4)
    c["ring33_T64"] = _pt_case(cc.CASES["ring33"], _ladder(64), 1)
    c["ring33_T65"] = _pt_case(cc.CASES["ring33"], _ladder(65), 2)            # one more than a wave has lanes; more than 32 pairs a phase
    c["ring33_T300"] = _pt_case(cc.CASES["ring33"], _ladder(300), 1)          # many more slots than the workgroup has waves
    c["k8_T2100"] = _pt_case(cc.CASES["k8"], _ladder(2100), 1)                # T beyond the workgroup's 1024 threads, and more pairs a phase
    c["star71_biased"] = _pt_case(cc.CASES["star71"], [0.2, 0.5, 1.0, 2.0], 2)
    c["ring300_distinct"] = _pt_case((ring300["edges"], ring300["biases"]), [0.3, 1.0, 4.0, 40.0], 2)  # non-dyadic sums: the energy order
    c["ring33_zero_and_equal"] = _pt_case(cc.CASES["ring33"], [0.0, 0.5, 0.5, 1.0, 2.0], 2)  # exponent 0: always accepted
    c["ring33_nonmonotone"] = _pt_case(cc.CASES["ring33"], [1.0, 0.2, 2.0, 0.5], 2)
    # random multigraphs: rows of 0 .. 16 entries, multi-edges, variables without an edge; 129 = two full lane passes and one variable
    for name in ("random33x1", "random129x4"):
        rc = cc.RANDOM_CASES[name]
        c[name + "_T4"] = _pt_case((rc["edges"], rc["biases"]), [0.2, 0.5, 1.0, 2.0], 2)
    return c


PT_CASES = _pt_cases()
PT_VARIANTS = ["batched", "serial", "global"]  # every case has N <= 5476


def pt_offset(name):
    """The replica offset of a parity case: one chain's worth, so that the global chain indices start at 1."""
    return len(PT_CASES[name]["betas"])


def initial_states(seed, nreplicas, nvars, replica_offset=0):
    """make_random_spin_state of every replica, as the library draws it."""
    idx = np.arange(nvars, dtype=np.uint64)
    rep = np.arange(nreplicas, dtype=np.uint64) + np.uint64(replica_offset)
    return (CR.philox_np(seed, idx[None, :], 0, rep[:, None], CR.TAG_INIT)[..., 0] >> np.uint64(31)).astype(np.uint8)


def host_run(cl, edges, biases, betas, chains, rounds, steps, replica_offset=0, **kw):
    """host_tempering_run from the random initial states."""
    nrep = chains * len(betas)
    init = initial_states(cc.SEED, nrep, len(biases), replica_offset)
    return cl.host_tempering_run(edges, biases, cc.SEED, init, 0, betas, rounds, steps, replica_offset=replica_offset, **kw)


@functools.lru_cache(maxsize=None)
def host_parity_reference(name):
    """The parity run of a case through isingmc_classical_host_pt_run.  Cached; callers do not write into it."""
    import isingmontecarlo_amd.classical as cl
    c = PT_CASES[name]
    return host_run(cl, c["edges"], c["biases"], c["betas"], c["chains"], PT_ROUNDS, PT_STEPS, replica_offset=pt_offset(name), kinds=cl.KINDS_ALL)


# ---- exact enumeration under tempering: C = 2048 chains of T = 4, 48 rounds of one only_basic_moves step ----
ENUM_PT_BETAJ = [0.2, 0.2 + 0.8 / 3.0, 0.2 + 1.6 / 3.0, 1.0]
ENUM_PT_CHAINS, ENUM_PT_ROUNDS = cc.ENUM_R // 4, 48
ENUM_PT_SKIP = 24  # rounds left out of the series mean (the equilibration the batch tests allow is 48 steps; see the CPU test)


def enum_pt_betas(name):
    return [cc.enum_beta(name, bj) for bj in ENUM_PT_BETAJ]


def enum_pt_violations(name, by_temperature):
    """enum_violations of states [C][T][N] at every temperature of the ladder: [(t, observable, mean, exact, sigma)]."""
    return [(t,) + v for t, bj in enumerate(ENUM_PT_BETAJ) for v in cc.enum_violations(name, bj, by_temperature[:, t, :])]


def enum_pt_series_sigmas(name, energy, skip=ENUM_PT_SKIP):
    """The mean of the recorded E series [rounds][C][T] over the rounds from `skip` on, in units of the exact standard deviation over
    sqrt(the number of samples), per temperature."""
    edges, biases = cc.ENUM_SYSTEMS[name]
    out = []
    for t, bj in enumerate(ENUM_PT_BETAJ):
        mean, sd = CR.exact_moments(edges, biases, cc.enum_beta(name, bj))["E"]
        x = energy[skip:, :, t]
        out.append(float(abs(x.mean() - mean) / (sd / np.sqrt(x.size))))
    return out
