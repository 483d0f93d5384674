"""The range joins and the flatten pass of the dedicated cluster kernel (csrc/sse_cluster.hip.h), bit-exact against the CPU oracle.

A thread joins the 16 range boundaries of its variable: the segment the worldline is in when range w ends continues into the
placeholder of range w + 1.  Wave wv takes the boundaries in the order (k + wv) & 15, so that the waves do not meet at one pair of
roots.  The flatten pass behind the joins walks four ids per thread to their roots together and appends a batch's roots to the
root list at once.  (One link per wave, boundary and pair of roots, the "dedup" of this file's name, was measured and is not in
the kernel: DESIGN.md section 7, r17.)  The cases are the strings on which the joins of a wave coincide most and least, and the
shapes of the variable loop:
  * giant: 8 x 8 ferromagnet at beta = 8: almost every lane of a wave finds the same pair of roots at a boundary;
  * interleaved: two disjoint, strongly coupled rings on the even and on the odd variables of N = 128: neighbouring lanes
    alternate between two pairs of roots.  The test rebuilds the clusters of the string from the oracle's op words, checks its
    count against the oracle's, and asserts that each ring holds a cluster of at least 64 ids (as many as it has variables);
  * distinct: N = 70 with couplings of 0.01 at beta = 2: almost no two-site op, so every lane links a pair of its own, and the
    second wave of the variable loop is partial;
  * one_chunk: a capacity of 2^20 makes one chunk of 8192 slots: 15 ranges are empty and every join of their boundaries is a
    real link between untouched placeholders;
  * chain3 and ring1100: fewer variables than a wave; two passes of the variable loop, the second one partial with 14 waves idle.
The kernel keeps no counter of its joins outside diagnostic builds (-DSSE_CL_JOIN_COUNTERS, tools/attribute.py), so this file pins
results only.

As in test_gpu_cluster_kernel_edges every call is one timestep long, launch_info()["lean_cluster"] is asserted after every call and
every replica's id count passes the kernel's gate (Pair.run): the dedicated kernel did the work and not the general one."""
import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import assert_same
from test_gpu_cluster_kernel_edges import Pair, CAP
from test_gpu_cluster_postscan_edges import chunk_size

pytestmark = pytest.mark.gpu


def two_rings(n, j):
    """ring 0 -> 2 -> 4 ... on the even variables and ring 1 -> 3 -> 5 ... on the odd ones"""
    return [((i, (i + 2) % n), j) for i in range(n)]


def clusters_of(words, edges, N):
    """The clusters of an op-string at h = 0 or not (cluster.rs:193-271): a transverse op opens a new segment of its variable, a
    two-site op joins the segments its variables are in, a longitudinal op joins nothing, the last segment of a variable continues
    into its first.  Returns {root: [variable of every id in the cluster]} over the cut segments and the touched initial ones."""
    E = len(edges)
    parent, var_of = list(range(N)), list(range(N))
    cur, touched = list(range(N)), [False] * N

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(a, b):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)

    for w in words:
        if w == 0:
            continue
        b = (int(w) >> 4) - 1
        if b < E:
            a, c = edges[b][0]
            touched[a] = touched[c] = True
            union(cur[a], cur[c])
        elif b < E + N:
            touched[b - E] = True
            parent.append(len(parent))
            var_of.append(b - E)
            cur[b - E] = len(parent) - 1
        else:
            touched[b - E - N] = True
    for v in range(N):
        union(cur[v], v)
    out = {}
    for i in range(len(parent)):
        if i >= N or touched[i]:
            out.setdefault(find(i), []).append(var_of[i])
    return out


def cluster_step(p, what):
    """one cluster update on both sides: counts, strings, gate"""
    ufcap = p.ufcap_bound()
    nc = p.g.single_cluster_step(flip_free=False)
    for r, rep in enumerate(p.reps):
        assert nc[r] == rep.cluster_update(0.5), f"{what}: cluster count differs r={r}"
    assert p.g.launch_info()["lean_cluster"], what
    p.check_gate(ufcap, what + " cluster step")
    assert_same(p.g, p.reps, what + " cluster step")


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("h", [0.0, 0.3])
def test_one_giant_cluster(oracle, h, k):
    edges = lat.two_d_ferro(8)
    p = Pair(oracle, edges, 1.0, h, 16, 1 << 14, 1357, 2, k=k)
    assert p.g.launch_info()["slots_per_lane"] == k
    what = f"giant h={h} k={k}"
    p.run(20, 8.0, 0, what)
    ch = chunk_size(1 << 14, k)
    assert all(rep.cutoff > 4 * ch for rep in p.reps), what  # several ranges hold ops
    for rep in p.reps:  # one cluster holds most ids of the string
        sizes = sorted((len(c) for c in clusters_of(rep.ops(), edges, 64).values()), reverse=True)
        assert sizes[0] >= 0.5 * sum(sizes), (what, sizes[:4], sum(sizes))
    cluster_step(p, what)
    p.check_acc(what)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("h", [0.0, 0.3])
def test_two_interleaved_clusters(oracle, h, k):
    N, edges = 128, two_rings(128, -4.0)
    p = Pair(oracle, edges, 1.0, h, 16, 1 << 14, 2468, 2, k=k)
    assert p.g.launch_info()["slots_per_lane"] == k
    what = f"interleaved h={h} k={k}"
    p.run(20, 4.0, 0, what)
    mine = [clusters_of(rep.ops(), edges, N) for rep in p.reps]
    ufcap = p.ufcap_bound()
    nc = p.g.single_cluster_step(flip_free=False)
    for r, rep in enumerate(p.reps):
        want = rep.cluster_update(0.5)
        assert nc[r] == want, f"{what}: cluster count differs r={r}"
        # the rebuilt partition has the oracle's count, no cluster spans both rings, and each ring holds a large one
        assert len(mine[r]) == want, (what, r, len(mine[r]), want)
        assert all(len({v % 2 for v in c}) == 1 for c in mine[r].values()), what
        big = [max(len(c) for c in mine[r].values() if c[0] % 2 == par) for par in (0, 1)]
        print(f"{what}: replica {r}: {want} clusters, largest of the even ring {big[0]} ids, of the odd ring {big[1]}")
        assert min(big) >= N // 2, (what, r, big)
    assert p.g.launch_info()["lean_cluster"], what
    p.check_gate(ufcap, what + " cluster step")
    assert_same(p.g, p.reps, what + " cluster step")
    p.check_acc(what)


@pytest.mark.parametrize("k", [2, 4])
def test_all_pairs_distinct(oracle, k):
    N, edges = 70, lat.one_d_periodic(70, -0.01)
    p = Pair(oracle, edges, 1.0, 0.0, 16, CAP, 97531, 2, k=k)
    assert p.g.launch_info()["slots_per_lane"] == k
    what = f"distinct k={k}"
    p.run(20, 2.0, 0, what)
    for rep in p.reps:  # almost no two-site op: a segment is joined to its variable's wrap-around partner and to nothing else
        w = rep.ops()
        two = int(((w != 0) & ((w >> 4) <= len(edges))).sum())
        assert rep.n >= 100 and two <= 0.05 * rep.n, (what, two, rep.n)
        c = clusters_of(w, edges, N)
        assert len(c) >= sum(len(x) for x in c.values()) - N - two, what
    cluster_step(p, what)
    p.check_acc(what)


@pytest.mark.parametrize("k", [2, 4])
def test_one_chunk(oracle, k):
    cap = 1 << 20
    p = Pair(oracle, lat.two_d_ferro(8), 1.0, 0.0, 16, cap, 8642, 2, k=k)
    assert p.g.launch_info()["slots_per_lane"] == k
    what, ch = f"one chunk k={k}", chunk_size(cap, k)
    for s in range(20):
        p.run(1, 2.0, 0, f"{what} step {s}")
        assert all(0 < rep.cutoff <= ch for rep in p.reps), what  # wave 0 scans the whole string, 15 ranges are empty
    cluster_step(p, what)
    p.check_acc(what)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name,edges,beta,cutoff,steps", [
    ("chain3", [((0, 1), -1.0), ((1, 2), -1.0)], 4.0, 16, 20),
    ("ring1100", lat.one_d_periodic(1100, -1.0), 0.5, 64, 8),
])
def test_variable_loop_shapes(oracle, name, edges, beta, cutoff, steps, k):
    N = max(max(e) for e, _ in edges) + 1
    p = Pair(oracle, edges, 1.0, 0.0, cutoff, CAP, 4711, 1 if N > 1000 else 2, k=k)
    assert p.g.launch_info()["slots_per_lane"] == k
    what = f"{name} k={k}"
    p.run(steps, beta, 0, what)
    cluster_step(p, what)
    p.check_acc(what)
