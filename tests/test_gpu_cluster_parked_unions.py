"""Parked unions of the dedicated cluster kernel's build scan (csrc/sse_cluster.hip.h), bit-exact against the CPU oracle.

A lane of the scan's union block whose find does not end inside the straight-line hops (SSE_CL_FIND_LEVELS = 4: a leg whose
representative lies four or more parents below its root), or whose link lost against another lane's, appends its pair of
ancestors to its wave's queue (64 entries).  A full queue is served at the top of the next tile of the range (an "early drain"),
a lane that finds the queue full before that runs the serial routine in its row as every such lane used to, and what is left is
served behind the scan.  The kernel counts, per replica, the pairs it served from the queues (word 11 of debug_phase_ticks) and
the early drains (word 15); every case asserts from them that the path it is about was taken.

Hand-built strings (import_ops, then cluster_update on both sides).  The model is a set of open ferromagnetic chains of n
variables side by side (variable c n + i, edge c (n - 1) + i joins i and i + 1 of chain c), all spins 0, every op a diagonal
two-site op, plus one variable without an edge that carries the one transverse op of the string (the kernel leaves strings without
a cut to the general kernel).  Capacity 2^16 makes chunks of 512 slots; the cutoff is 112 chunks, so that each of the 16 waves
scans seven chunks = 56 rows of 64 slots.  A tile's rows are all looked up before the first of them is linked (the compare-and-store
of a row that met a stale entry fails), so every row with ops below starts a tile of its own: "row j" is row 4 j of the wave's range
for either tile size (four rows at four slots per lane, two at two).  Chains have n = 11 variables.  Row j holds op
(n - 2 - j, n - 1 - j) of every chain, j = 0 .. 9: behind these "descending" rows variable i's table entry names the id of i - 1,
which lies i - 1 parents below the root (the id of variable 0).  A later op (i, i + 1) then starts from ids at depths i - 1 and i:
it is parked iff one of them is 4 or more, i.e. for i >= 4.  (The issue draws six descending rows for a chain of 12 inside one
chunk; with one row per tile that needs more rows than a chunk has, so a wave's range is seven chunks here and the chains are built
down to variable 0, which makes the depths the plain ones above.)
  * deep: one chain in wave 0's range, then a row with the ops (i, i + 1), i = 5 .. 9: five lanes parked, no early drain;
  * later_range: the same rows in wave 1's range, where the ids are placeholders;
  * overflow: 32 chains; row 10 holds (i, i + 1), i = 6 .. 9, of chains 0 - 15: 64 lanes, the queue is full; row 11 (the next
    tile) holds (9, 10) of chains 16 - 31: 16 more (serving the queue flattens the chains it touches, so the second dense row
    takes chains of its own).  One early drain, 80 parked, both dense rows in one wave's range;
  * full_queue: the same two rows in ONE tile (rows 40 and 41 of the range): the 16 lanes find the queue full and are served in
    their row.  64 parked, one early drain at the top of the tile behind;
  * revisit: the deep row (5,6), (7,8), (9,10), then three rows on the same variables: (6,7), (8,9); the deep row's ops again;
    (6,7), (8,9) again.  Three replicas hold the string up to the deep row, up to the second and up to the third of these rows:
    the last row parks fewer lanes than the deep row did: a parked lane rewrites both legs' entries with the smaller of the
    ancestors it reached, so later ops start closer to the root.  (The kernel does not re-point the start nodes in the parent
    table as well: that was timed and is slower at the headline size.  With it the middle rows would park nothing; without it
    they park one lane each, and the last row none either way);
  * conflict: a star of 40 leaves 0 .. 39 around variable 40, all 40 ops in one row: every lane hooks the root 40 under its own
    leaf, one wins, the others find another parent on reading back.  There is no straight-line second attempt for a lost link
    in the kernel (it did not earn its place), so they are parked: at least one.
Every case runs with four and two slots per lane, with deferred and in-place apply, and once with a longitudinal field of 0.25
(the kernel's other instantiation); three cluster updates each, compared after every one.

One equilibrated case ties the counters to real strings: 8x8 ferromagnet, Gamma = 1, beta = 8, capacity 2^14, 4 replicas, 12 whole
timesteps.  Only the counters' consistency is asserted (an early drain serves a whole queue); their level is printed."""
import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import assert_same, make_pair
from test_gpu_trim_paths import CLUSTER_WAVES, chunk_size

pytestmark = pytest.mark.gpu

CAP, CH, CHUNKS, SEED, N = 1 << 16, 512, 112, 90125, 11
ROWS = CHUNKS * CH // 64 // CLUSTER_WAVES  # rows of a wave's range
QCAP = 64


def chains(nchains, n):
    """edges of the chains and the number of variables, the last one without an edge"""
    return [((c * n + i, c * n + i + 1), -1.0) for c in range(nchains) for i in range(n - 1)], nchains * n + 1


def string(nchains, n, rows, wave=0, same_tile=False):
    """rows: per tile of the wave's range the list of i whose op (i, i + 1) every chain gets in the tile's first row (same_tile: the
    last list goes into the second row of the tile in front of it); the cut sits in the string's last slot"""
    words = np.zeros(CHUNKS * CH, dtype=np.uint32)
    at = [4 * j for j in range(len(rows))]
    if same_tile:
        at[-1] = at[-2] + 1
    assert at[-1] < ROWS
    for j, ops in zip(at, rows):
        ops, which = ops if isinstance(ops, tuple) else (ops, range(nchains))  # (ops, chains) or ops for every chain
        lanes = [c * (n - 1) + i for i in ops for c in which]
        assert len(lanes) <= 64 and len(set(lanes)) == len(lanes)
        p = (wave * ROWS + j) * 64
        words[p:p + len(lanes)] = [(b + 1) << 4 for b in lanes]
    words[-1] = (nchains * (n - 1) + nchains * n + 1) << 4  # bond E + (last variable), in = out = 0
    return words


def descending(n):
    return [[n - 2 - j] for j in range(n - 1)]


def star_case():
    leaves = 40
    edges = [((l, leaves), -1.0) for l in range(leaves)]
    words = np.zeros(CHUNKS * CH, dtype=np.uint32)
    words[:leaves] = [(b + 1) << 4 for b in range(leaves)]
    words[-1] = (leaves + (leaves + 1) + 1) << 4  # the cut on the edge-less variable leaves + 1
    return edges, leaves + 2, [words]


def build(name):
    """edges, variables, one string per replica"""
    if name == "deep":
        e, nv = chains(1, N)
        return e, nv, [string(1, N, descending(N) + [[5, 6, 7, 8, 9]])] * 2
    if name == "later_range":
        e, nv = chains(1, N)
        return e, nv, [string(1, N, descending(N) + [[5, 6, 7, 8, 9]], wave=1)] * 2
    if name in ("overflow", "full_queue"):
        e, nv = chains(32, N)
        dense = [([6, 7, 8, 9], range(16)), ([9], range(16, 32))]
        return e, nv, [string(32, N, descending(N) + dense, same_tile=name == "full_queue")] * 2
    if name == "revisit":
        e, nv = chains(1, N)
        deep, odd = [5, 7, 9], [6, 8]
        return e, nv, [string(1, N, descending(N) + tail) for tail in ([deep], [deep, odd, deep], [deep, odd, deep, odd])]
    assert name == "conflict"
    e, nv, w = star_case()
    return e, nv, w * 2


def check_counters(name, k, parked, drains):
    """the path the case is about was taken (parked, drains: per replica, after the first update)"""
    assert (drains * QCAP <= parked).all(), (parked, drains)
    if name in ("deep", "later_range"):
        assert (parked >= 1).all() and (drains == 0).all(), (parked, drains)
        assert (parked == 5).all(), parked  # the five lanes of the deep row, nothing else
    elif name == "overflow":
        assert (drains >= 1).all() and (parked > QCAP).all(), (parked, drains)
        assert (parked == 80).all() and (drains == 1).all(), (parked, drains)
    elif name == "full_queue":
        assert (drains == 1).all() and (parked == QCAP).all(), (parked, drains)
    elif name == "revisit":
        first, last = int(parked[0]), int(parked[2]) - int(parked[1])
        assert first >= 1 and 0 <= last < first, parked
    else:
        assert (parked >= 1).all(), parked


VARIANTS = [(0, False, 0.0), (0, True, 0.0), (2, False, 0.0), (2, True, 0.0), (0, False, 0.25)]


@pytest.mark.parametrize("k,inplace,h", VARIANTS, ids=["k4-deferred", "k4-inplace", "k2-deferred", "k2-inplace", "k4-deferred-long"])
@pytest.mark.parametrize("name", ["deep", "later_range", "overflow", "full_queue", "revisit", "conflict"])
def test_parked_unions(oracle, name, k, inplace, h):
    import isingmontecarlo_amd as im
    edges, nvars, strings = build(name)
    R, M = len(strings), CHUNKS * CH
    assert chunk_size(CAP, k or 4) == CH and -(-M // CH) == CHUNKS >= 2  # seven chunks per wave: the rows where string() puts them
    g, m, reps = make_pair(oracle, edges, 1.0, h, M, CAP, SEED, R, state=[0] * nvars, k=k, nvars=nvars,
                           cfg_flags=im.CFG_NO_DEFERRED_FLIPS if inplace else 0)
    for r, words in enumerate(strings):
        g.import_ops(words, r)
        reps[r].set_ops(words)
    assert g.verify().all() and all(rep.verify() for rep in reps)
    g.debug_phase_ticks(reset=True)
    for call in range(3):
        nc = g.single_cluster_step(flip_free=False)
        info = g.launch_info()
        assert info["lean_cluster"] and info["slots_per_lane"] == (k or 4), info
        if call == 0:
            tk = g.debug_phase_ticks(reset=True)
            parked, drains = tk[:, 11].astype(np.int64), tk[:, 15].astype(np.int64)
            print(f"{name}: parked {parked.tolist()} early drains {drains.tolist()}")
            check_counters(name, k or 4, parked, drains)
        for r, rep in enumerate(reps):
            assert nc[r] == rep.cluster_update(0.5), f"{name}: cluster count differs call={call} r={r}"
        assert_same(g, reps, f"{name} call {call}")
    acc = g.accumulators()
    for r, rep in enumerate(reps):
        assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), f"{name}: accumulators differ r={r}"
    assert g.verify().all()


def test_counters_on_equilibrated_strings(oracle):
    edges, beta, steps, R = lat.two_d_ferro(8), 8.0, 12, 4
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 64, 1 << 14, 4711, R)
    for _ in range(steps):
        oracle.batch_timesteps(reps, 1, [beta] * R, 1, 0)
    g.debug_phase_ticks(reset=True)
    g.run(steps, beta)
    assert g.launch_info()["lean_cluster"]
    tk = g.debug_phase_ticks(reset=False)
    parked, drains = tk[:, 11].astype(np.int64), tk[:, 15].astype(np.int64)
    print(f"8x8, beta 8, {steps} timesteps: parked per replica {parked.tolist()}, early drains {drains.tolist()}, cutoffs {g.get_cutoff().tolist()}")
    assert (drains * QCAP <= parked).all(), (parked, drains)
    assert_same(g, reps, "equilibrated")
    acc = g.accumulators()
    for r, rep in enumerate(reps):
        assert np.array_equal(acc[r, :7], rep.accumulators()[:7])
    assert g.verify().all()
