"""The dedicated cluster kernel (csrc/sse_cluster.hip.h) behind its row scan, bit-exact against the CPU oracle: the row masks of
the deferred flips (collected in one register per tile and stored by lanes 0 .. 4 K - 1), the root list written by the flatten
pass (both branches: the list holds every root / more roots than it holds), the bond table at its smallest and largest, and the
range joins on strings with empty ranges, untouched variables, one giant cluster and many small ones.

As in test_gpu_cluster_kernel_edges every call is one timestep long, launch_info()["lean_cluster"] is asserted after every call
and every replica's id count passes the kernel's gate (Pair.run), so the dedicated kernel did the work and not the general one."""
import ctypes as C

import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import assert_same
from test_gpu_cluster_kernel_edges import Pair, cuts_of, largest_lean_ring, CAP

pytestmark = pytest.mark.gpu


def chunk_size(cap, k):
    import isingmontecarlo_amd as im
    out = (C.c_uint32 * 4)()
    assert im.load_library().isingmc_plan_geometry(cap, 4, k, 16, out) == 0
    return int(out[0])


def list_cap(N, Nb, has_long, S):
    """entries of the root list for a replica with S ids (isingmc_plan_cluster_lds out[12]; independent of the launch's capacity)"""
    import isingmontecarlo_amd as im
    out = (C.c_uint32 * 13)()
    assert im.load_library().isingmc_plan_cluster_lds(N, (N + 31) // 32, Nb, has_long, 65535, S, out) == 0
    return int(out[12])


# Row masks.  "one_chunk": a capacity of 2^20 makes one chunk of 8192 slots, so wave 0 scans the whole string and the ranges of the
# other 15 waves are empty (no tile, no mask store); the string's length is no multiple of a tile, so the only range ends in a
# partial tile.  "few_chunks": a capacity of 2^14 makes chunks of 256 slots, the string fills several of them and the last wave
# that has a range ends in a partial tile.  20 timesteps: the flip bytes made from every mask a cluster update stores are consumed
# by the diagonal launch of the next one.  h = 0.3: the second pair of mask dwords of a row (the two-site mask) is a ballot that
# the lane write reads right behind the compare that makes it; a build that hides that dependency from the compiler (inline
# assembly) reads a stale mask on gfx950 and fails every h = 0.3 case here at its first timestep.
@pytest.mark.parametrize("layout", ["one_chunk", "few_chunks"])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("h", [0.0, 0.3])
@pytest.mark.parametrize("l", [4, 8])
def test_row_masks(oracle, l, h, k, layout):
    cap, beta = ((1 << 20), 2.0) if layout == "one_chunk" else ((1 << 14), 8.0)
    p = Pair(oracle, lat.two_d_ferro(l), 1.0, h, 16, cap, 97 + l, 4, k=k)
    assert p.g.launch_info()["slots_per_lane"] == k
    ch, what = chunk_size(cap, k), f"{l}x{l} h={h} k={k} {layout}"
    partial = several = False
    for s in range(20):
        p.run(1, beta, 0, f"{what} step {s}")
        for rep in p.reps:
            used = (rep.cutoff + ch - 1) // ch
            assert used == 1 if layout == "one_chunk" else used <= 128, what
            several |= used >= 2
            partial |= rep.cutoff % (64 * k) != 0
    assert partial, what
    assert several or layout == "one_chunk", what
    p.check_acc(what)


# Root list, both branches.  The flatten pass lists at most (clusters + N) roots: every placeholder id is joined to a smaller id,
# every cut id that is a root is a cluster, and the N initial ids are clusters or untouched.  So a cluster count with
# count + N <= cl_list_cap takes the list branch for certain, and a count above cl_list_cap the branch in which every id draws
# its root's coin.  The counts are the oracle's (the return value of its cluster update, taken at the string that 20 timesteps
# at this beta produce), the capacity is the kernel's own for that string's S = 16 N + C.
@pytest.mark.parametrize("name,edges,beta,overflow", [
    ("chain3", [((0, 1), -1.0), ((1, 2), -1.0)], 4.0, False),
    ("8x8", lat.two_d_ferro(8), 8.0, False),
    ("bond", [((0, 1), -1.0)], 100.0, True),
    ("ring4", lat.one_d_periodic(4, -1.0), 100.0, True),
])
def test_root_list_branches(oracle, name, edges, beta, overflow):
    N = max(max(e) for e, _ in edges) + 1
    p = Pair(oracle, edges, 1.0, 0.0, N, CAP, 4711, 2)
    p.run(20, beta, 0, name)
    caps = [list_cap(N, p.Nb, 0, 16 * N + cuts_of(rep, p.E, N)) for rep in p.reps]
    ufcap = p.ufcap_bound()
    nc = p.g.single_cluster_step(flip_free=False)
    for r, rep in enumerate(p.reps):
        want = rep.cluster_update(0.5)
        print(f"{name}: replica {r}: {want} clusters, list holds {caps[r]}")
        assert nc[r] == want, f"{name}: cluster count differs r={r}"
        if overflow:
            assert want > caps[r], (name, want, caps[r])
        else:
            assert want + N <= caps[r], (name, want, N, caps[r])
    assert p.g.launch_info()["lean_cluster"]
    p.check_gate(ufcap, name + " cluster step")
    assert_same(p.g, p.reps, name + " cluster step")
    p.check_acc(name)


# Bond table: two entries besides the empty slot's (open 3-site chain, E = 2), Nb = E + N and E + 2 N at 8 x 8
@pytest.mark.parametrize("name,edges,h", [
    ("chain3", [((0, 1), -1.0), ((1, 2), -1.0)], 0.0),
    ("chain3_long", [((0, 1), -1.0), ((1, 2), -1.0)], 0.3),
    ("8x8", lat.two_d_ferro(8), 0.0),
    ("8x8_long", lat.two_d_ferro(8), 0.3),
])
def test_bond_table_sizes(oracle, name, edges, h):
    N = max(max(e) for e, _ in edges) + 1
    p = Pair(oracle, edges, 1.0, h, 16, CAP, 1234, 3)
    assert p.Nb == len(edges) + N * (2 if h else 1)
    p.run(20, 4.0, 0, name)
    p.check_acc(name)


def test_bond_table_largest_model(oracle):
    """the largest ring the dedicated kernel takes (as test_gpu_cluster_kernel_edges finds it), now for 20 timesteps from an
    almost empty string"""
    steps, beta, cutoff, seed = 20, 0.05, 64, 86420
    n = largest_lean_ring(oracle, steps, beta, cutoff, seed)
    assert n >= 1024, n
    p = Pair(oracle, lat.one_d_periodic(n, -1.0), 1.0, 0.0, cutoff, CAP, seed, 1)
    p.run(steps, beta, 0, f"ring of {n}")
    p.check_acc(f"ring of {n}")


def test_two_graphs_stepped_alternately(oracle):
    """two batches of different graphs (and different table sizes) alive in one process: nothing of one launch's set-up leaks
    into the other's"""
    a = Pair(oracle, lat.two_d_ferro(8), 1.0, 0.0, 16, CAP, 11, 3)
    b = Pair(oracle, lat.one_d_periodic(33, -1.0), 1.0, 0.3, 16, CAP, 12, 2)
    for s in range(20):
        a.run(1, 4.0, 0, f"8x8 step {s}")
        b.run(1, 2.0, 0, f"ring33 step {s}")
    a.check_acc("8x8")
    b.check_acc("ring33")


# Range joins
JOIN_CASES = [
    # variables that no op ever touches: nvars above the largest index of an edge (their 16 ids are joined into one untouched tree)
    ("ring6_of_10", lat.one_d_periodic(6, -1.0), 10, 2.0, CAP),
    # strings with empty ranges: one chunk, so 15 of the 16 boundaries chain a placeholder to a placeholder
    ("8x8_one_chunk", lat.two_d_ferro(8), None, 0.25, 1 << 20),
    # one giant cluster: many threads link one root
    ("8x8_giant", lat.two_d_ferro(8), None, 8.0, 1 << 14),
    # many small clusters: many distinct links
    ("8x8_weak", [(e, -0.05) for e, _ in lat.two_d_ferro(8)], None, 8.0, 1 << 14),
]


@pytest.mark.parametrize("name,edges,nvars,beta,cap", JOIN_CASES, ids=[c[0] for c in JOIN_CASES])
def test_range_joins(oracle, name, edges, nvars, beta, cap):
    p = Pair(oracle, edges, 1.0, 0.0, 16, cap, 1357, 4, nvars=nvars)
    if nvars is not None:
        assert p.N == nvars
    p.run(25, beta, 0, name)
    p.check_acc(name)
