"""isingmc_pt_plan_phase — the decisions of one phase of isingmc_pt_step's host leg as one rank sees them, from plain data — with the
ranks simulated in one process: every rank gets its neighbours' wire, a returned item moves an operator count and a configuration
id across the boundary, and after both phases the ladder must be what isingmc_pt_decide makes of it.  This is the only place where
a rank talks to a lower and an upper neighbour in one phase, and where a rank owns a single temperature (its first and last walker
coincide).  Relative weights other than 1 are not covered here (per-slot Hamiltonians run on the GPU, one and two ranks)."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O

SEED = 99
STEPS = list(range(20)) + [2 ** 32 - 1]
LAYOUTS = [(3, 1, 3), (6, 3, 3), (9, 2, 3), (6, 3, 2), (5, 3, 1)]  # (T, K, world)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Rank:
    def __init__(self, im, rank, world, tper, K, betas, n_of_config):
        self.im, self.rank, self.world, self.tper, self.K, self.betas = im, rank, world, tper, K, betas
        R = tper * K
        self.slot_of = np.arange(rank * R, (rank + 1) * R, dtype=np.uint32)  # replica r starts at local slot r
        self.at = np.arange(R, dtype=np.uint32)
        self.ids = self.slot_of.copy()  # configuration id of replica r
        self.n = np.ascontiguousarray(n_of_config[self.ids], dtype=np.uint32)
        self.cutoff = np.arange(50, 50 + K, dtype=np.uint32)
        self.got = [(self.im._PtWire * K)(), (self.im._PtWire * K)()]
        self.items = [np.zeros(3 * K, dtype=np.uint32), np.zeros(3 * K, dtype=np.uint32)]

    def wire(self, side):
        """what this rank sends to its lower (0) / upper (1) neighbour: its first / last temperature's walkers"""
        base = (self.tper - 1) * self.K if side else 0
        return [(int(self.n[self.at[base + k]]), 1.0) for k in range(self.K)]

    def receive(self, side, wire):
        for k, (n, rel) in enumerate(wire):
            self.got[side][k].n, self.got[side][k].pad, self.got[side][k].rel = n, 0, rel

    def plan(self, step, phase):
        v = self.im._PtPhase(struct_size=C.sizeof(self.im._PtPhase), rank=self.rank, world=self.world, tper=self.tper, nchains=self.K,
                             phase=phase, betas=_p(self.betas, C.c_double), seed=SEED, step=step, n=_p(self.n, C.c_uint32), rel=None,
                             cutoff=_p(self.cutoff, C.c_uint32), fixed_words=7, slot_of=_p(self.slot_of, C.c_uint32),
                             at=_p(self.at, C.c_uint32))
        for s in range(2):
            if 0 <= self.rank + (1 if s else -1) < self.world:
                v.from_[s] = C.cast(self.got[s], C.POINTER(self.im._PtWire))
                v.items[s] = _p(self.items[s], C.c_uint32)
        assert self.im.load_library().isingmc_pt_plan_phase(C.byref(v)) == 0
        out = []
        for s in range(2):
            it = self.items[s][:3 * v.nitems[s]].reshape(-1, 3)
            # message layout: items in chain order, each fixed_words + its chain's cutoff long
            chains = [int(self.slot_of[r]) % self.K for r in it[:, 0]]
            assert chains == sorted(set(chains)) and [int(c) for c in it[:, 2]] == [50 + k for k in chains]
            assert [int(o) for o in it[:, 1]] == [int(x) for x in np.cumsum([0] + [7 + 50 + k for k in chains])[:-1]]
            assert v.words[s] == sum(7 + 50 + k for k in chains)
            out.append([int(r) for r in it[:, 0]])
        return out, int(v.nswaps)


def reference(im, T, K):
    """isingmc_pt_decide over the trials (one step each, on a fresh ladder with fresh operator counts): the counts, config_at after
    the step, its swaps, and (decoded from the permutation and the oracle's coin word) how often every pair of neighbouring
    temperatures was accepted and refused."""
    rng = np.random.default_rng(11)
    betas = np.linspace(1.0, 2.0, T)
    ns, after, swaps, acc, coins = [], [], [], np.zeros(max(T - 1, 0), dtype=int), set()
    for step in STEPS:
        ns.append(rng.integers(0, 40, size=T * K).astype(np.uint32))
        before = np.arange(T * K, dtype=np.uint32)
        config_at = before.copy()
        swaps.append(im.pt_decide(SEED, step, K, T, betas, ns[-1], config_at))
        after.append(config_at)
        for k in range(K):
            a_first = bool(int(O.pt_words(SEED, step, 1, K)[0, k]) >> 31)
            coins.add(a_first)
            cur, fin = list(before[k::K]), list(config_at[k::K])
            first = 0 if a_first else 1
            for t in range(first, T - 1, 2):  # first phase: an accepted walker ends at t + 1 or above, a refused one at t or below
                if fin.index(cur[t]) >= t + 1:
                    cur[t], cur[t + 1] = cur[t + 1], cur[t]
                    acc[t] += 1
            for t in range(1 - first, T - 1, 2):  # second phase: nothing moves afterwards
                if fin[t] != cur[t]:
                    cur[t], cur[t + 1] = cur[t + 1], cur[t]
                    acc[t] += 1
            assert cur == fin
        assert sum(acc) == sum(swaps)
    return betas, ns, after, swaps, acc, len(STEPS) * K - acc, coins


@pytest.mark.parametrize("T,K,world", LAYOUTS, ids=[f"T{t}_K{k}_ranks{w}" for t, k, w in LAYOUTS])
def test_simulated_ranks_match_pt_decide(T, K, world):
    import isingmontecarlo_amd as im
    betas, ns, after, swaps, accepted, refused, coins = reference(im, T, K)
    # the reference alone: every pair, each rank boundary included, is accepted and refused, and both phase orders occur
    assert accepted.min() >= 3 and refused.min() >= 3 and coins == {False, True}, (accepted, refused, coins)
    tper = T // world
    for i, step in enumerate(STEPS):
        ranks = [Rank(im, g, world, tper, K, betas, ns[i]) for g in range(world)]
        total = 0
        for phase in range(2):
            for g in range(world - 1):  # the exchange of the boundary walkers' counts
                up, down = ranks[g].wire(1), ranks[g + 1].wire(0)
                ranks[g].receive(1, down)
                ranks[g + 1].receive(0, up)
            planned = [r.plan(step, phase) for r in ranks]
            total += sum(sw for _, sw in planned)
            for g in range(world - 1):  # the accepted boundary swaps: the configurations change ranks
                lo, hi = ranks[g], ranks[g + 1]
                mine, theirs = planned[g][0][1], planned[g + 1][0][0]
                assert len(mine) == len(theirs)
                for ra, rb in zip(mine, theirs):
                    assert lo.slot_of[ra] + K == hi.slot_of[rb]
                    lo.n[ra], hi.n[rb] = hi.n[rb], lo.n[ra]
                    lo.ids[ra], hi.ids[rb] = hi.ids[rb], lo.ids[ra]
        assert total == swaps[i], step
        for r in ranks:
            assert np.array_equal(r.at[r.slot_of - r.rank * tper * K], np.arange(tper * K))
            assert np.array_equal(r.ids, after[i][r.slot_of]) and np.array_equal(r.n, ns[i][after[i][r.slot_of]]), (step, r.rank)
