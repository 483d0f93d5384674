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
    """f64::powi as the library and the oracle evaluate it: squaring sequence, reciprocal for negative exponents.  With an array
    for either argument the same sequence runs element by element (the same bits as the scalar form)."""
    if np.ndim(x) == 0 and np.ndim(n) == 0:
        m, r = abs(int(n)), 1.0
        while m:
            if m & 1:
                r *= x
            x *= x
            m >>= 1
        return 1.0 / r if n < 0 else r
    n = np.asarray(n, dtype=np.int64)
    x = np.broadcast_to(np.asarray(x, dtype=np.float64), np.broadcast(x, n).shape).copy()
    n = np.broadcast_to(n, x.shape)
    m, r = np.abs(n), np.ones(x.shape)
    with np.errstate(all="ignore"):
        while m.any():
            r = np.where((m & 1) != 0, r * x, r)
            x = x * x
            m = m >> 1
        return np.where(n < 0, 1.0 / r, r)


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
        self.nbonds = self.E + self.N * (2 if self.has_long else 1)

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

    def relative_weights(self, counts, s_from, s_to):
        """relative_weight for many configurations at once: counts[m][nbonds] (bond_count of every bond), slots s_from[m], s_to[m].
        The same factors multiplied in the same order, so the same bits."""
        E, N = self.E, self.N
        counts = np.asarray(counts, dtype=np.int64)
        w = np.ones(len(counts))
        for b in range(E):
            w = w * powi(self.J[s_to, b] / self.J[s_from, b], counts[:, b])
        w = w * powi(self.gamma[s_to] / self.gamma[s_from], counts[:, E:E + N].sum(axis=1))
        if self.has_long:
            on = np.abs(self.h[s_from]) > np.finfo(float).eps
            lw = powi(self.h[s_to] / np.where(on, self.h[s_from], 1.0), counts[:, E + N:E + 2 * N].sum(axis=1))
            w = np.where(on, w * lw, w)
        return w

    def offset(self, s):
        return np.abs(self.J[s]).sum() + self.N * (self.gamma[s] + abs(self.h[s]))


def reference_pt(model, betas, nchains, seed, cap, cutoff, nsteps, sweeps_per_step, flags=0, step0=0, hams=None, accept=None, warmup=0):
    """`nsteps` times: `sweeps_per_step` sweeps of every replica at its slot's beta with the update rule `flags`, then one tempering
    step (numbered step0, step0 + 1, ...).  `model` is the common oracle model; with `hams` (SlotHamiltonians) every slot has its
    own, swaps weigh both Hamiltonians and an accepted swap moves the two configurations onto each other's model.

    `accept(beta_t, beta_t1, n_a, n_b, rel) -> p` replaces the rule p = powi(beta_t / beta_t1, n_b - n_a) * rel (tests of the tests:
    a wrong rule must be seen).  It is called once per pair of slots with arrays over the chains that decide that pair (n_a, n_b
    int64; rel the product of the two relative weights, the float 1.0 without `hams`); a hook with an attribute `sides = True` gets
    the pair (rel_a, rel_b) instead of the product.  With a hook the cross-check against the oracle's own pt_step is skipped.
    `warmup`: the first so many steps add nothing to acc, swaps, attempts and pair_accepts.

    All replicas sweep in one threaded batch call and the decisions of a pair of slots are taken for all chains at once; the
    arithmetic per decision is the one spelled out in `powi` and `relative_weight`."""
    betas = np.asarray(betas, dtype=np.float64)
    T, K = len(betas), int(nchains)
    S = T * K
    mdl = (lambda s: hams.models[s]) if hams is not None else (lambda s: model)
    objs = [O.Replica(mdl(s), cap, cutoff, seed, s) for s in range(S)]  # replica objects; who[s]: the one now at slot s = t*K + k
    who = np.arange(S)
    optr = O.pointers(objs)
    bslot = np.repeat(betas, K)
    ids = np.arange(S, dtype=np.int64)
    acc = np.zeros((S, 8), dtype=np.uint64)
    pair_accepts = np.zeros(max(T - 1, 0), dtype=np.int64)
    swaps = attempts = 0
    sides = bool(getattr(accept, "sides", False))
    for i in range(nsteps):
        step, measured = step0 + i, i >= warmup
        ptrs = optr[who]
        before = O.batch_get(ptrs)[2]
        O.batch_run(ptrs, sweeps_per_step, bslot, 1, flags)
        n, cut, after = O.batch_get(ptrs)
        if measured:
            acc += after - before
        if T <= 1:
            continue
        check = None
        if hams is None and accept is None:  # the oracle's own step on the same graphs: must agree with the decisions below
            check, check_swaps = O.batch_pt_step(ptrs, betas, K, seed, step)
        maxcut = cut.reshape(T, K).max(axis=0)
        for s in np.flatnonzero(cut != np.tile(maxcut, T)):
            assert objs[who[s]].set_cutoff(int(maxcut[s % K])) == 0
        words = O.pt_words(seed, step, T, K)
        a_first = (words[0] >> 31) != 0
        u = words[1:] / 4294967296.0
        n = n.astype(np.int64).reshape(T, K)
        counts = O.batch_bond_counts(ptrs, hams.nbonds).reshape(T, K, -1) if hams is not None else None
        took = np.zeros(K, dtype=np.int64)
        for phase in range(2):
            set_a = a_first if phase == 0 else ~a_first
            for t in range(T - 1):
                ks = np.flatnonzero(set_a if t % 2 == 0 else ~set_a)
                if ks.size == 0:
                    continue
                sa, sb = t * K + ks, (t + 1) * K + ks
                na, nb = n[t, ks], n[t + 1, ks]
                rel = 1.0
                if hams is not None:
                    ra, rb = hams.relative_weights(counts[t, ks], sa, sb), hams.relative_weights(counts[t + 1, ks], sb, sa)
                    rel = ra * rb
                if accept is None:
                    p = powi(betas[t] / betas[t + 1], nb - na)
                    if hams is not None:
                        p = p * rel
                else:
                    p = np.broadcast_to(np.asarray(accept(betas[t], betas[t + 1], na, nb, (ra, rb) if sides and hams is not None else rel),
                                                   dtype=np.float64), ks.shape)
                yes = p > u[t, ks]
                ka, sa, sb = ks[yes], sa[yes], sb[yes]
                if measured:
                    attempts += int(ks.size)
                    pair_accepts[t] += int(ka.size)
                    swaps += int(ka.size)
                took[ka] += 1
                n[t, ka], n[t + 1, ka] = n[t + 1, ka], n[t, ka]
                if hams is None:
                    who[sa], who[sb] = who[sb], who[sa]
                elif ka.size:
                    counts[t, ka], counts[t + 1, ka] = counts[t + 1, ka], counts[t, ka]
                    # the configurations change Hamiltonians: each lands on the other slot's model with its op-string, state, update
                    # counter and Philox identity (cutoffs are equal by now), which is the two replica objects exchanging models
                    O.swap_models([objs[j] for j in who[sa]], [objs[j] for j in who[sb]])
                    who[sa], who[sb] = who[sb], who[sa]
                ids[sa], ids[sb] = ids[sb], ids[sa]
        if check is not None:
            assert np.array_equal(check_swaps, took) and np.array_equal(check, optr[who]), "the oracle's pt_step decided differently"
    by_slot = [[objs[who[t * K + k]] for t in range(T)] for k in range(K)]
    return PtReference(by_slot, ids, swaps, pair_accepts, acc, attempts)
