"""The cases that the tests of per-replica couplings share (CPU: the host entries, GPU: the kernels): the realisations of every case by
a fixed numpy rule, and the oracle: replica r of a per-replica batch is a shared-coupling one-replica run with J = couplings[r] at
replica_offset + r, through isingmc_classical_host_steps (the path that existed before the flag) and through the numpy restatement
RefGraphState.  Test infrastructure only."""
import functools

import numpy as np

import _classical_cases as cc
import _classical_pt_cases as pc
import _classical_reference as CR
import _lattices as lat

R = 5
PARITY = ["one_edge", "triangle", "k8", "star71", "duplicate_edge", "ring33", "ring65"]
IMPORTANCE = ["k8_positive", "ring33_positive"]
ZERO_ROWS_CASE = "ring33"  # this case keeps a zero coupling in its odd rows


def with_couplings(edges, row):
    """The same endpoints with the couplings of one realisation."""
    return [(ab, float(j)) for (ab, _), j in zip(edges, row)]


def realisations(name, nreplicas=R):
    """[nreplicas][E]: row r is a permutation of the case's own (dyadic) couplings, for the cases with signs under random sign flips, so
    every sum stays exact; row 0 is the case's own list.  The importance cases keep their positive values."""
    edges, _ = cc.CASES[name]
    js = np.array([j for _, j in edges], dtype=np.float64)
    rng = np.random.default_rng(1000 + len(name) * 31 + len(js))
    rows = [js.copy()]
    for r in range(1, nreplicas):
        row = js[rng.permutation(len(js))]
        if name not in IMPORTANCE:
            row = row * rng.choice([-1.0, 1.0], len(js))
        if name == ZERO_ROWS_CASE and r % 2:
            row[(3 * r) % len(js)] = 0.0
        rows.append(row)
    return np.ascontiguousarray(np.stack(rows))


def rotate_rows(couplings):
    """The rows moved on by one replica (what indexing the tables by the wrong replica reads)."""
    return np.ascontiguousarray(np.roll(couplings, 1, axis=0))


def rotate_entries(edges, couplings):
    """Every row with its couplings moved on by one edge (cc.rotate_couplings per row: a wrong entry index reads rows like these)."""
    return np.ascontiguousarray(np.array([[j for _, j in cc.rotate_couplings(with_couplings(edges, row))] for row in couplings]))


# ---- more than a dictionary, and sums that depend on their order ----
def _signed_value(i):
    return (-(i + 1) if i % 3 == 0 else (i + 1)) / 256.0


def dictionary_case(distinct):
    """A ring of 200 with biases: every replica alone has at most 200 distinct couplings, the batch exactly 256 (R = 2: the dictionary's
    last size) or 257 (R = 3: one value too many, doubles)."""
    assert distinct in (256, 257)
    rows = [[_signed_value(i) for i in range(200)], [_signed_value(i) for i in range(56, 256)]]
    if distinct == 257:
        rows.append([_signed_value(256)] + rows[0][1:])
    cj = np.array(rows, dtype=np.float64)
    assert len(np.unique(cj)) == distinct and all(len(np.unique(r)) <= 200 for r in cj)
    edges = [((i, (i + 1) % 200), float(j)) for i, j in enumerate(rows[0])]
    return edges, [0.125 * ((v % 5) - 2) for v in range(200)], cj


def order_case():
    """ring300_distinct-style, with values that are not dyadic: 300 couplings +-(i + 1) / 300 and biases in tenths, row r the values moved
    on by 7 r edges.  The energies and energy differences depend on the order of the additions; 300 distinct values: doubles."""
    vals = np.array([(-(i + 1) if i % 3 == 0 else (i + 1)) / 300.0 for i in range(300)])
    cj = np.ascontiguousarray(np.stack([np.roll(vals, 7 * r) for r in range(R)]))
    edges = [((i, (i + 1) % 300), float(j)) for i, j in enumerate(cj[0])]
    return edges, [0.1 * ((v % 5) - 2) for v in range(300)], cj


def case(name):
    """(edges, biases, couplings [R'][E], betas [R'], importance)"""
    if name in ("dict256", "dict257"):
        e, b, cj = dictionary_case(int(name[4:]))
        return e, b, cj, cc.LAYOUT_BETAS_SMALL_J[1:1 + len(cj)], False
    if name == "order300":
        e, b, cj = order_case()
        return e, b, cj, cc.LAYOUT_BETAS_SMALL_J, False
    e, b = cc.CASES[name]
    return e, b, realisations(name), cc.betas(R), name in IMPORTANCE


def initial_states(nreplicas, nvars):
    """make_random_spin_state of the replicas OFFSET .. OFFSET + R - 1 as the library draws it."""
    return pc.initial_states(cc.SEED, nreplicas, nvars, cc.OFFSET)


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


def host_chain(edges, biases, couplings, betas, runs, importance=False, states=None, per_replica=True, flags=0):
    """`runs` one after the other through isingmc_classical_host_steps from the random initial states (or `states`): [(states, counters,
    epochs)] after each run, counters summed from the start.  per_replica: one call with the couplings argument; otherwise the oracle:
    one shared-coupling one-replica call per row, J = couplings[r], replica_offset = OFFSET + r."""
    cl = _cl()
    nrep, n = len(couplings), len(biases)
    flags |= cl.CFG_EDGE_IMPORTANCE if importance else 0
    st = initial_states(nrep, n) if states is None else np.array(states, dtype=np.uint8)
    ep, total, out = np.zeros(nrep, dtype=np.uint64), np.zeros((nrep, 8), dtype=np.uint64), []
    for kinds, t, nspin, nedge, nworm in runs:
        if per_replica:
            st, ep, ctr = cl.host_steps(edges, biases, cc.SEED, st, ep, t, betas, nspin, nedge, nworm, kinds=kinds, replica_offset=cc.OFFSET, flags=flags,
                                        couplings=couplings)
        else:
            rows = [cl.host_steps(with_couplings(edges, couplings[r]), biases, cc.SEED, st[r:r + 1], ep[r:r + 1], t, betas[r:r + 1], nspin, nedge, nworm,
                                  kinds=kinds, replica_offset=cc.OFFSET + r, flags=flags) for r in range(nrep)]
            st, ep, ctr = (np.concatenate([row[i] for row in rows]) for i in range(3))
        total = total + ctr
        out.append((st.copy(), total.copy(), ep.copy()))
    return out


@functools.lru_cache(maxsize=None)
def oracle_chain(name, runs=None):
    """cc.RUNS of a case by the oracle.  Cached; callers do not write into it."""
    e, b, cj, betas, imp = case(name)
    return host_chain(e, b, cj, betas, cc.RUNS if runs is None else runs, imp, per_replica=False)


@functools.lru_cache(maxsize=None)
def host_per_replica_chain(name, runs=None, flags=0):
    """cc.RUNS of a case through the per-replica host entry (what the device is compared with).  Cached."""
    e, b, cj, betas, imp = case(name)
    return host_chain(e, b, cj, betas, cc.RUNS if runs is None else runs, imp, flags=flags)


@functools.lru_cache(maxsize=None)
def restatement_chain(name):
    """cc.RUNS of a case on the numpy restatement, one RefGraphState per replica on its own realisation."""
    e, b, cj, betas, imp = case(name)
    reps = [CR.RefGraphState(with_couplings(e, cj[r]), b, cc.SEED, cc.OFFSET + r, importance=imp) for r in range(len(cj))]
    out = []
    for kinds, t, nspin, nedge, nworm in cc.RUNS:
        for g, beta in zip(reps, betas):
            g.timesteps(t, beta, nspin=nspin, nedge=nedge, nworm=nworm, kinds=kinds)
        out.append((np.stack([g.state_bytes() for g in reps]), np.array([g.counters for g in reps], dtype=np.uint64),
                    np.array([g.epoch for g in reps], dtype=np.uint64)))
    return out


# ---- the plan cases: +-J realisations on the l x l periodic lattice at 40960 LDS words ----
# in_lds / tables bits: row starts 1, row entries 2, dictionary 4, biases 8, edge list 16, cumulative weights 32, per-replica couplings 64
def lattice_pmj(l, nreplicas=R):
    """(edges, biases, couplings): independent random signs on every bond of every replica."""
    edges = lat.two_d_periodic(l)
    cj = np.random.default_rng(l).choice([-1.0, 1.0], (nreplicas, len(edges)))
    return edges, [0.0] * (l * l), np.ascontiguousarray(cj)


def carve_words(l, waves, codes_in_lds, edges_in_lds=True):
    """The LDS words of a launch of the l x l lattice with a dictionary of two values, by arithmetic: `waves` areas of state bits and
    stamp bytes, the row starts, the row entries, the waves' code bytes, the dictionary on an even word, the packed edge list."""
    n, e = l * l, 2 * l * l
    o = waves * ((n + 31) // 32 + (n + 3) // 4) + (n + 1) + 2 * e
    if codes_in_lds:
        o += waves * ((2 * e + 3) // 4)
    o = (o + 1) // 2 * 2 + 2 * 2
    return o + (e if edges_in_lds else 0)


def wave_words(l, codes_in_lds):
    n, e = l * l, 2 * l * l
    return (n + 31) // 32 + (n + 3) // 4 + ((2 * e + 3) // 4 if codes_in_lds else 0)


PLAN_CASES = {
    # 4 waves with everything in LDS: 2592 + 2305 + 9216 + 4 * 2304 -> 23329, the dictionary at 23330 .. 23333, the edge list 4608
    "pmj48": dict(l=48, flags=0, plan=dict(waves=4, in_lds=87, tables=87, lds_words=27942, wave_words=2952, coupling_format=1, compact_couplings=True)),
    # 4 waves would need 49670 words; 2 waves: 2304 + 4097 + 16384 + 2 * 4096 -> 30977, 30978 .. 30981, 8192
    "pmj64": dict(l=64, flags=0, plan=dict(waves=2, in_lds=87, tables=87, lds_words=39174, wave_words=5248, coupling_format=1, compact_couplings=True)),
    # one wave with everything needs 42936 words: the fall-back, 4 waves, 5832 + 5185 + 20736 = 31753; the codes (4 * 5184) and the edge
    # list (10368) do not fit behind, the dictionary does
    "pmj72": dict(l=72, flags=0, plan=dict(waves=4, in_lds=7, tables=87, lds_words=31758, wave_words=1458, coupling_format=1, compact_couplings=True)),
    # tables forced to global memory: only the waves' areas
    "pmj48_global": dict(l=48, flags=2, plan=dict(waves=4, in_lds=0, tables=87, lds_words=2592, wave_words=648, coupling_format=1, compact_couplings=True)),
    # the codes alone kept in global memory (CFG_GLOBAL_CODES, for A-B timing): the shared-coupling launch of this lattice, 33286 words
    "pmj64_global_codes": dict(l=64, flags=16, plan=dict(waves=4, in_lds=23, tables=87, lds_words=33286, wave_words=1152, coupling_format=1, compact_couplings=True)),
}
LDS_WORDS = 40960


def layout_states(nvars):
    return np.random.default_rng(nvars + 1).integers(0, 2, (R, nvars), dtype=np.uint8)


# ---- tempering: C realisations x T temperatures ----
PT_CASES = {"k8_T2": ("k8", [0.3, 1.0], 3), "ring65_T3": ("ring65", [0.2, 0.7, 1.5], 3), "lattice4x4_T8": ("lattice4x4", pc._ladder(8, 0.1, 1.0), 4)}
PT_KEYS = ("states", "epochs", "counters", "temp_of", "attempts", "accepts", "energy", "magnetization")


def pt_case(name):
    """(edges, biases, betas, chains, couplings [C T][E]: realisation c in the T rows of chain c)"""
    graph, betas, chains = PT_CASES[name]
    edges, biases = cc.CASES[graph]
    js = np.array([j for _, j in edges], dtype=np.float64)
    rng = np.random.default_rng(77 + len(js))
    real = np.stack([js] + [js[rng.permutation(len(js))] * rng.choice([-1.0, 1.0], len(js)) for _ in range(chains - 1)])
    return edges, biases, betas, chains, np.ascontiguousarray(np.repeat(real, len(betas), axis=0))


@functools.lru_cache(maxsize=None)
def pt_host_reference(name, record=True, steps=pc.PT_STEPS):
    """The per-replica host run of a tempering case from the random initial states, replica_offset = T.  Cached."""
    edges, biases, betas, chains, cj = pt_case(name)
    return pc.host_run(_cl(), edges, biases, betas, chains, pc.PT_ROUNDS, steps, replica_offset=len(betas), kinds=CR.KINDS_ALL, couplings=cj, record=record)


def pt_oracle_chain(name, c):
    """Chain c by the oracle: a shared-coupling run of T slots on realisation c at replica_offset = T + c T."""
    edges, biases, betas, chains, cj = pt_case(name)
    t = len(betas)
    return pc.host_run(_cl(), with_couplings(edges, cj[c * t]), biases, betas, 1, pc.PT_ROUNDS, pc.PT_STEPS, replica_offset=t + c * t, kinds=CR.KINDS_ALL)
