"""The touched flag of the dedicated cluster kernel (csrc/sse_cluster.hip.h), bit-exact against the CPU oracle.

Without a longitudinal field the scan stores no touched byte: a variable counts as touched in a wave's range iff its table entry
carries the flag behind the scan, and only a cut's whole-word store or the union block's compare-and-store set it.  A variable
wrongly taken as untouched gets its p = 0 spin redrawn by the free-spin step (and is not flipped with its cluster), one wrongly
taken as touched keeps a spin it should draw: either shows in the states, and from the next sweep on in the op-strings.  The
cases are the ways a variable can be touched or not; each asserts from the oracle's strings that its situation really occurs
for the committed seed, so that a change of the update rules cannot quietly empty it:
  * untouched: 4x4 ferromagnet at beta = 0.2, most sweeps leave variables without any op (their free-spin draws must match);
  * root0: ring of 4, Gamma = 0.05: variable 0 carries two-site ops and no cut while the replica has a cut elsewhere, so wave 0
    touches it only through unions in which its own id 0, the smallest of all, survives as the root;
  * later_range: capacity 2^13 (chunks of 256 slots) with cutoffs above 512: ranges of later waves, whose initial ids are
    placeholders, hold variables with two-site ops and no cut;
  * two_cuts: two variables, Gamma = 4: 64-slot rows with two transverse ops on one variable (the scan's rare path, which
    stores the surviving cut's id with a 16-bit store and the flag next to it);
  * long: h != 0, where an op can act on a variable without cutting or linking: the kernel's other instantiation, which keeps
    its touched stores.
Every case runs with deferred flips and with the in-place apply pass, with four and with two slots per lane, 12 whole
timesteps, and ends by reading the strings back (export_ops)."""
import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import assert_same, make_pair
from test_gpu_trim_paths import CLUSTER_WAVES, chunk_size

pytestmark = pytest.mark.gpu

STEPS, SEED = 12, 4711

# name: edges, Gamma, h, beta, starting cutoff, capacity, replicas
CASES = {
    "untouched": (lat.two_d_ferro(4), 1.0, 0.0, 0.2, 16, 1 << 12, 8),
    "root0": (lat.one_d_periodic(4), 0.05, 0.0, 2.0, 16, 1 << 12, 8),
    "later_range": (lat.two_d_ferro(4), 0.2, 0.0, 8.0, 600, 1 << 13, 4),
    "two_cuts": (lat.chain(2, lambda i: 1.0), 4.0, 0.0, 8.0, 64, 1 << 12, 4),
    "long": (lat.two_d_ferro(4), 1.0, 0.25, 3.0, 64, 1 << 12, 4),
}


def acts_on(words, edges, nvars):
    """Of one stretch of an op-string: (variables with any op, variables with a transverse op, transverse ops, longitudinal ops).
    Bonds [0, E) are the edges, [E, E + N) the transverse field, the rest the longitudinal field (word = (bond + 1) << 4 | bits)."""
    E = len(edges)
    ea, ec = np.array([e[0][0] for e in edges]), np.array([e[0][1] for e in edges])
    b = (words.astype(np.int64) >> 4) - 1
    occ = words != 0
    two, cut, lng = occ & (b < E), occ & (b >= E) & (b < E + nvars), occ & (b >= E + nvars)
    touched, cutv = np.zeros(nvars, bool), np.zeros(nvars, bool)
    touched[ea[b[two]]] = True
    touched[ec[b[two]]] = True
    touched[b[cut] - E] = True
    touched[b[lng] - E - nvars] = True
    cutv[b[cut] - E] = True
    return touched, cutv, int(cut.sum()), int(lng.sum())


@pytest.fixture(scope="module")
def references():
    """name -> (replicas at the end, history): emptied when the module is done, while the oracle library is still loaded"""
    cache = {}
    yield cache
    cache.clear()


def reference(oracle, cache, name, reps, edges, nvars, beta):
    """The oracle's 12 timesteps, run once per case and shared by its four variants: the replicas at the end and, sweep by
    sweep, every replica's (string, cutoff, n)."""
    if name not in cache:
        hist = []
        for _ in range(STEPS):
            oracle.batch_timesteps(reps, 1, [beta] * len(reps), 1, 0)
            hist.append([(rep.ops(), rep.cutoff, rep.n) for rep in reps])
        cache[name] = (reps, hist)
    return cache[name]


def check_precondition(name, hist, edges, nvars, ch):
    """What the case is about occurs in the oracle's run (a sweep's string is what its cluster update saw: the update only
    flips bits).  Replica-sweeps without a cut or without an op are not counted: the kernel leaves those to the general one."""
    E = len(edges)
    sweeps = [[acts_on(w, edges, nvars) + (w, M, n) for w, M, n in sw] for sw in hist]
    if name == "untouched":
        some_free = [any(C > 0 and not t.all() for t, c, C, _, w, M, n in sw) for sw in sweeps]
        assert sum(some_free) >= STEPS // 2, some_free
    elif name == "root0":
        hits = sum(1 for sw in sweeps for t, c, C, _, w, M, n in sw if C > 0 and t[0] and not c[0])
        assert hits >= 4, hits
        assert all(M < ch for sw in sweeps for *_, M, n in sw)  # one range: wave 0, where variable 0's initial id is 0
    elif name == "later_range":
        assert all(M > 512 for *_, M, n in sweeps[-1]), [M for *_, M, n in sweeps[-1]]
        hits = ranges = 0
        for sw in sweeps:
            for t, c, C, _, w, M, n in sw:
                used = -(-M // ch)
                q = -(-used // CLUSTER_WAVES)
                for wave in range(1, CLUSTER_WAVES):
                    c0 = min(wave * q, used)
                    c1 = min(c0 + q, used)
                    if c1 > c0:
                        tr, cr, _, _ = acts_on(w[c0 * ch:min(c1 * ch, M)], edges, nvars)
                        ranges += 1
                        hits += bool(C > 0 and (tr & ~cr).any())
        assert ranges >= 2 * STEPS and hits >= ranges // 2, (hits, ranges)  # at least three waves have a range, most hold such a variable
    elif name == "two_cuts":
        rows = 0
        assert all(n >= 64 for *_, n in sweeps[-1]), [n for *_, n in sweeps[-1]]
        for sw in sweeps:
            for t, c, C, _, w, M, n in sw:
                for p in range(0, M, 64):
                    b = (w[p:p + 64].astype(np.int64) >> 4) - 1
                    cv = b[(w[p:p + 64] != 0) & (b >= E) & (b < E + nvars)] - E
                    rows += bool(len(cv) and np.bincount(cv).max() >= 2)
        assert rows >= 16, rows
    else:
        assert all(nl > 0 for sw in sweeps for t, c, C, nl, w, M, n in sw)  # longitudinal ops in every string


@pytest.mark.parametrize("k", [0, 2], ids=["k4", "k2"])
@pytest.mark.parametrize("inplace", [False, True], ids=["deferred", "inplace"])
@pytest.mark.parametrize("name", list(CASES))
def test_touched_flag(oracle, references, name, inplace, k):
    import isingmontecarlo_amd as im
    edges, gamma, h, beta, cut0, cap, R = CASES[name]
    g, m, fresh = make_pair(oracle, edges, gamma, h, cut0, cap, SEED, R, k=k, cfg_flags=im.CFG_NO_DEFERRED_FLIPS if inplace else 0)
    reps, hist = reference(oracle, references, name, fresh, edges, g.nvars, beta)
    ch = chunk_size(cap, k or 4)
    assert ch == 256  # (both capacities: with 2^13 a cutoff above 512 spreads over three waves and more)
    check_precondition(name, hist, edges, g.nvars, ch)
    g.run(STEPS, beta)
    info = g.launch_info()
    assert info["lean_cluster"] and info["slots_per_lane"] == (k or 4), info
    assert_same(g, reps, name)  # states (the free-spin draws), epochs, counts, and the strings through export_ops
    acc = g.accumulators()
    for r, rep in enumerate(reps):
        assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), f"{name}: accumulators differ r={r}"
    assert g.verify().all()
