"""The graph-swapping reference of parallel tempering that every tempering test compares against: oracle replicas live at
(chain, temperature) slots and whole graphs change places (TemperingContainer::tempering_step, tempering_container.rs:121-149,
241-302), with GraphWeights::relative_weight (tempering_traits.rs:126-155) when the slots carry different Hamiltonians.
Test infrastructure only."""
import ctypes as C
from collections import namedtuple

import numpy as np

import _oracle as O

TAG_PT = 6
PtReference = namedtuple("PtReference", "by_slot ids swaps pair_accepts acc attempts")
PtReference.__doc__ = """by_slot[k][t]: the oracle replica at chain k, temperature t; ids[t*K + k]: the configuration (global id it was
created with) now at that slot; swaps: all accepted swaps; pair_accepts[t]: accepted swaps of the pair (t, t + 1) over all chains;
acc[t*K + k][8]: what the replicas accumulated while they sat at that slot; attempts: decisions taken (pairs * chains * steps)."""


def powi(x, n):
    """f64::powi as the library and the oracle evaluate it: squaring sequence, reciprocal for negative exponents."""
    m, r = abs(int(n)), 1.0
    while m:
        if m & 1:
            r *= x
        x *= x
        m >>= 1
    return 1.0 / r if n < 0 else r


def philox(seed, idx, step, chain):
    """First word of the decision stream: counter (idx, step_lo, chain, TAG_PT << 24 | step_hi), key = seed."""
    ctr = (C.c_uint32 * 4)(idx, step & 0xFFFFFFFF, chain, (TAG_PT << 24) | ((step >> 32) & 0xFFFFFF))
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = (C.c_uint32 * 4)()
    O.lib().ora_philox4x32_10(ctr, key, out)
    return out[0]


class SlotHamiltonians:
    """Per-slot Hamiltonians on one graph: J[T*K][E], gamma[T*K], h[T*K], row t*K + k."""

    def __init__(self, nvars, edges, J, gamma, h):
        self.N, self.edges = int(nvars), [list(e) for e in edges]
        self.E = len(self.edges)
        self.J = np.asarray(J, dtype=np.float64)
        self.gamma = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (len(self.J),)).copy()
        self.h = np.broadcast_to(np.asarray(0.0 if h is None else h, dtype=np.float64), (len(self.J),)).copy()
        self.has_long = bool(np.any(self.h != 0.0))
        self.models = [O.Model(self.N, self.edges, list(self.J[s]), float(self.gamma[s]), float(self.h[s])) for s in range(len(self.J))]

    def relative_weight(self, rep, s_from, s_to):
        """The weight of rep's configuration under slot s_to's Hamiltonian relative to the one it lives in (s_from): edges in
        order, then the transverse field, then the longitudinal one when s_from has any."""
        E, N, w = self.E, self.N, 1.0
        for b in range(E):
            w *= powi(self.J[s_to][b] / self.J[s_from][b], rep.bond_count(b))
        w *= powi(self.gamma[s_to] / self.gamma[s_from], sum(rep.bond_count(E + v) for v in range(N)))
        if self.has_long and abs(self.h[s_from]) > np.finfo(float).eps:
            w *= powi(self.h[s_to] / self.h[s_from], sum(rep.bond_count(E + N + v) for v in range(N)))
        return w

    def offset(self, s):
        return np.abs(self.J[s]).sum() + self.N * (self.gamma[s] + abs(self.h[s]))


def reference_pt(model, betas, nchains, seed, cap, cutoff, nsteps, sweeps_per_step, flags=0, step0=0, hams=None):
    """`nsteps` times: `sweeps_per_step` sweeps of every replica at its slot's beta with the update rule `flags`, then one tempering
    step (numbered step0, step0 + 1, ...).  `model` is the common oracle model; with `hams` (SlotHamiltonians) every slot has its
    own, swaps weigh both Hamiltonians and an accepted swap rebuilds the two replicas on the slots' models."""
    betas = np.asarray(betas, dtype=np.float64)
    T, K = len(betas), int(nchains)
    mdl = (lambda t, k: hams.models[t * K + k]) if hams is not None else (lambda t, k: model)
    by_slot = [[O.Replica(mdl(t, k), cap, cutoff, seed, t * K + k) for t in range(T)] for k in range(K)]
    ids = np.arange(T * K, dtype=np.int64)
    acc = np.zeros((T * K, 8), dtype=np.uint64)
    pair_accepts = np.zeros(max(T - 1, 0), dtype=np.int64)
    swaps = attempts = 0
    for i in range(nsteps):
        step = step0 + i
        for k in range(K):
            for t in range(T):
                rep = by_slot[k][t]
                before = rep.accumulators()
                rep.timesteps(sweeps_per_step, float(betas[t]), 1, flags)
                acc[t * K + k] += rep.accumulators() - before
        if T <= 1:
            continue
        for k in range(K):
            chain = by_slot[k]
            maxcut = max(r.cutoff for r in chain)
            check = None
            if hams is None:  # the oracle's own step on the same graphs: must agree with the decisions below
                check = list(chain)
                check_swaps = O.pt_step(check, betas, seed, k, step)
            for r in chain:
                assert r.set_cutoff(maxcut) == 0
            a_first = (philox(seed, 0, step, k) >> 31) != 0
            took = 0
            for phase in range(2):
                set_a = a_first if phase == 0 else not a_first
                for t in range(0 if set_a else 1, T - 1, 2):
                    u = philox(seed, 1 + t, step, k) / 4294967296.0
                    ga, gb = chain[t], chain[t + 1]
                    sa, sb = t * K + k, (t + 1) * K + k
                    p = powi(betas[t] / betas[t + 1], gb.n - ga.n)
                    if hams is not None:
                        p = p * (hams.relative_weight(ga, sa, sb) * hams.relative_weight(gb, sb, sa))
                    attempts += 1
                    if not p > u:
                        continue
                    took += 1
                    pair_accepts[t] += 1
                    if hams is None:
                        chain[t], chain[t + 1] = gb, ga
                    else:
                        na = O.Replica(hams.models[sa], cap, maxcut, seed, int(ids[sb]), gb.state()); na.set_ops(gb.ops()); na.set_epoch(gb.epoch)
                        nb = O.Replica(hams.models[sb], cap, maxcut, seed, int(ids[sa]), ga.state()); nb.set_ops(ga.ops()); nb.set_epoch(ga.epoch)
                        chain[t], chain[t + 1] = na, nb
                    ids[sa], ids[sb] = ids[sb], ids[sa]
            if check is not None:
                assert check_swaps == took and [r.ptr for r in check] == [r.ptr for r in chain], "the oracle's pt_step decided differently"
            swaps += took
    return PtReference(by_slot, ids, swaps, pair_accepts, acc, attempts)
