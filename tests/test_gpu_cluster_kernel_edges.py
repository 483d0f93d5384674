"""The dedicated cluster kernel (csrc/sse_cluster.hip.h) on the paths its instruction trimming touched, bit-exact against the
CPU oracle: the branch-free predicated stores of the row scan (rows without a cut, rows full of cuts, two cuts on one variable),
the union block's parent stores and its serial routine (many lanes hooking one root), the per-wave table fill and the ballot-based
state / free-spin tail at variable counts that are no multiple of 32 or 64, and the largest model the kernel takes.

Every case proves that the dedicated kernel did the work and not the general kernel behind it: launch_info()["lean_cluster"]
is set after every call, and every replica's id count S = 16 N + C (C = transverse ops, counted from the oracle's op words after
every timestep) passes the kernel's gate as isingmc_plan_cluster_lds reports it.  The gate is evaluated at a lower bound of the
launch's union-find capacity: plan_lean() sizes it from the largest C the host has seen (plus a sixteenth and 384 ids of headroom),
which it refreshes at the end of every call.  A string that starts empty grows by up to half its length per timestep, which
outruns that headroom within a few timesteps of one call (the kernel then flags the replica for the general kernel, by design), so
every call here is one timestep long and the bound is taken from the counts in front of it."""
import ctypes as C

import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import make_pair, assert_same

pytestmark = pytest.mark.gpu

CAP = 1 << 16


def cuts_of(rep, E, N):
    w = rep.ops()
    bond = (w >> 4).astype(np.int64) - 1
    return int(((w != 0) & (bond >= E) & (bond < E + N)).sum())


def gate_ok(N, Nb, has_long, ufcap, S):
    import isingmontecarlo_amd as im
    out = (C.c_uint32 * 13)()
    assert im.load_library().isingmc_plan_cluster_lds(N, (N + 31) // 32, Nb, has_long, ufcap, S, out) == 0
    return bool(out[11])


class Pair:
    """A batch and its oracle replicas, advanced together; the oracle one timestep at a time so that the cut counts of every
    cluster update are known."""

    def __init__(self, oracle, edges, gamma, h, cutoff, cap, seed, R, k=0, cfg_flags=0, nvars=None):
        self.oracle = oracle
        self.g, self.m, self.reps = make_pair(oracle, edges, gamma, h, cutoff, cap, seed, R, k=k, cfg_flags=cfg_flags, nvars=nvars)
        self.E, self.N, self.cap, self.has_long = len(edges), self.g.nvars, cap, 1 if h != 0.0 else 0
        self.Nb = self.E + self.N * (2 if self.has_long else 1)
        self.seen = 0  # largest C at the end of any call so far: the host knows at least this much

    def ufcap_bound(self):
        c0 = max(self.seen, max(cuts_of(rep, self.E, self.N) for rep in self.reps))
        return 16 * self.N + min(self.cap, c0 + c0 // 16 + 384)

    def check_gate(self, ufcap, what):
        for r, rep in enumerate(self.reps):
            c = cuts_of(rep, self.E, self.N)
            assert gate_ok(self.N, self.Nb, self.has_long, ufcap, 16 * self.N + c), f"{what}: replica {r} with {c} cuts is outside the gate (ufcap >= {ufcap})"
            self.seen = max(self.seen, c)

    def run(self, t, beta, flags, what):
        """t timesteps, one per call, the gate asserted for the cluster update of every one of them"""
        for s in range(t):
            ufcap = self.ufcap_bound()
            self.g.run(1, beta, flags=flags)
            self.oracle.batch_timesteps(self.reps, 1, [beta] * len(self.reps), 1, flags)
            self.check_gate(ufcap, f"{what} step {s}")
            assert self.g.launch_info()["lean_cluster"], what
        assert_same(self.g, self.reps, what)

    def check_acc(self, what):
        acc = self.g.accumulators()
        for r, rep in enumerate(self.reps):
            assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), what
        assert self.g.verify().all(), what


# Both predicated stores of a row all-dummy (beta = 0.25: most rows hold no cut and no union) and all-real (beta = 8), both
# HAS_LONG instantiations, both tile shapes, deferred flips and the in-place apply pass, with and without the directed loop
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("inplace", [False, True], ids=["deferred", "inplace"])
@pytest.mark.parametrize("beta", [0.25, 8.0])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("h", [0.0, 0.3])
@pytest.mark.parametrize("l", [4, 8])
def test_scan_and_union_stores(oracle, l, h, k, beta, inplace, flags):
    import isingmontecarlo_amd as im
    R = 8
    p = Pair(oracle, lat.two_d_ferro(l), 1.0, h, 16, 1 << 20, 8642, R, k=k, cfg_flags=im.CFG_NO_DEFERRED_FLIPS if inplace else 0)
    assert p.g.launch_info()["slots_per_lane"] == k
    what = f"{l}x{l} h={h} k={k} beta={beta} inplace={inplace} flags={flags}"
    p.run(30, beta, flags, what)
    p.check_acc(what)


# Rows full of cuts, two cuts on one variable in most rows (the lane-order path of the scan), inside the gate: beta * Gamma ~ 100
@pytest.mark.parametrize("name,edges", [("ring4", lat.one_d_periodic(4, -1.0)), ("bond", [((0, 1), -1.0)])])
def test_rows_full_of_cuts(oracle, name, edges):
    N = max(max(e) for e, _ in edges) + 1
    p = Pair(oracle, edges, 1.0, 0.0, N, CAP, 4711, 2)
    p.run(20, 100.0, 0, name)
    # most occupied rows hold two cuts on one variable
    rows = two = 0
    for rep in p.reps:
        w = rep.ops()
        w = np.pad(w, (0, -len(w) % 64)).reshape(-1, 64)
        bond = (w >> 4).astype(np.int64) - 1
        cut = (w != 0) & (bond >= p.E) & (bond < p.E + N)
        cnt = np.stack([(cut & (bond == p.E + v)).sum(axis=1) for v in range(N)], axis=1)
        rows += int((w != 0).any(axis=1).sum())
        two += int((cnt >= 2).any(axis=1).sum())
    assert two >= 0.5 * rows, (name, two, rows)
    ufcap = p.ufcap_bound()
    nc = p.g.single_cluster_step(flip_free=False)
    for r, rep in enumerate(p.reps):
        assert nc[r] == rep.cluster_update(0.5), f"{name}: cluster count differs r={r}"
    assert p.g.launch_info()["lean_cluster"]
    p.check_gate(ufcap, name + " cluster step")
    assert_same(p.g, p.reps, name + " cluster step")
    p.check_acc(name)


# Many lanes hooking one root in one row: link conflicts, the serial union routine
@pytest.mark.parametrize("name,edges", [("complete8", lat.complete(8, -1.0)), ("star9", lat.star(9, -1.0))])
def test_many_lanes_hook_one_root(oracle, name, edges):
    N = max(max(e) for e, _ in edges) + 1
    p = Pair(oracle, edges, 1.0, 0.0, N, CAP, 1357, 4)
    p.run(30, 8.0, 0, name)
    p.check_acc(name)


# Variable counts that are no multiple of 32 or 64: table fill, state and free-spin ballots.  A starting cutoff of 8 leaves most
# variables untouched in the first sweeps, so free spins are drawn; the state is compared after each of the first 5 timesteps
@pytest.mark.parametrize("n", [31, 33, 65, 97])
def test_odd_variable_counts(oracle, n):
    R, beta = 3, 2.0
    p = Pair(oracle, lat.one_d_periodic(n, -1.0), 1.0, 0.0, 8, CAP, 2468 + n, R)
    free_drawn = False
    for s in range(5):
        ufcap = p.ufcap_bound()
        p.g.run(1, beta, flags=0)
        oracle.batch_timesteps(p.reps, 1, [beta] * R, 1, 0)
        st = p.g.state_ref()
        for r, rep in enumerate(p.reps):
            assert np.array_equal(st[r], rep.state()), f"n={n}: state differs after timestep {s}, replica {r}"
            w = rep.ops()
            bond = (w[w != 0] >> 4).astype(np.int64) - 1
            touched = set(bond[bond >= n] - n) | {a for b in bond[bond < n] for a in (int(b), (int(b) + 1) % n)}
            free_drawn |= len(touched) < n and cuts_of(rep, p.E, n) > 0  # (a replica without a cut is the general kernel's)
        p.check_gate(ufcap, f"n={n} step {s}")
        assert p.g.launch_info()["lean_cluster"]
        assert_same(p.g, p.reps, f"n={n} step {s}")
    assert free_drawn, f"n={n}: no sweep of the dedicated kernel left a variable untouched"
    p.run(25, beta, 0, f"n={n} steps 5-29")
    p.check_acc(f"n={n}")


def largest_lean_ring(oracle, steps, beta, cutoff, seed):
    """Largest ring whose every one of `steps` one-timestep calls the dedicated kernel takes on this device, from the plan
    exports: the batch's plan keeps the kernel, and the LDS of every launch fits.  A launch's union-find is sized as plan_lean()
    sizes it, from the largest cut count m the host has seen at the end of the calls before it (16 N + m + m / 16 + 384 ids), so
    the first cuts already push the largest ring of a fresh batch out: the oracle gives the counts of every candidate."""
    import torch
    import isingmontecarlo_amd as im
    import _plan_cases as pc
    lds_bytes = torch.cuda.get_device_properties(0).shared_memory_per_block
    lib = im.load_library()
    out = (C.c_uint32 * 13)()

    def fits(n, ufcap):
        assert lib.isingmc_plan_cluster_lds(n, (n + 31) // 32, 2 * n, 0, ufcap, ufcap - 1, out) == 0
        return bool(out[11]) and 4 * out[10] <= lds_bytes

    for n in range(2048, 2, -1):
        if not fits(n, 16 * n + 384):
            continue
        edges = lat.one_d_periodic(n, -1.0)
        cfg, keep = pc.config_of(im, dict(nreplicas=1, capacity=CAP, cutoff=cutoff), dict(edges=edges, nvars=n, transverse=1.0, longitudinal=0.0))
        rc, slots = pc.plan_batch(im, cfg, lds_bytes)
        if rc != 0 or not dict(zip(pc.SLOTS, slots))["lean_cluster"]:
            continue
        e, j = lat.split(edges)
        rep = oracle.Replica(oracle.Model(n, e, j, 1.0, 0.0), CAP, cutoff, seed, 0, None)
        m, ok = 0, True
        for s in range(steps):
            ok = ok and fits(n, 16 * n + min(CAP, m + m // 16 + 384))
            rep.timesteps(1, beta, 1, 0)
            m = max(m, cuts_of(rep, n, n))
        if ok:
            return n
    raise AssertionError("no ring fits the dedicated cluster kernel")


def test_largest_model_the_kernel_takes(oracle):
    """The table fill at the top of its range: the largest ring that stays the dedicated kernel's through 5 timesteps from a
    starting cutoff of 64."""
    steps, beta, cutoff, seed = 5, 0.5, 64, 97531
    n = largest_lean_ring(oracle, steps, beta, cutoff, seed)
    assert n >= 1024, n  # (the benchmark's 32 x 32 lattice runs through this kernel)
    p = Pair(oracle, lat.one_d_periodic(n, -1.0), 1.0, 0.0, cutoff, CAP, seed, 1)
    p.run(steps, beta, 0, f"ring of {n}")
    p.check_acc(f"ring of {n}")
