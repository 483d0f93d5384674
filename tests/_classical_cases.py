"""The graphs and runs that the classical Monte Carlo tests share (CPU: isingmc_classical_host_steps, GPU: the kernels), and the
restatement's results for them, computed once per run and cached.  Test infrastructure only."""
import functools

import numpy as np

import _classical_reference as CR
import _lattices as lat


def _dyadic(rng, n, lo=-16, hi=16, nonzero=True):
    x = rng.integers(lo, hi + 1, n).astype(np.float64)
    if nonzero:
        x[x == 0] = 1.0
    return x / 8.0


def _ring(n, seed):
    rng = np.random.default_rng(seed)
    return [((i, (i + 1) % n), float(j)) for i, j in enumerate(_dyadic(rng, n))], [float(h) for h in _dyadic(rng, n, -4, 4, nonzero=False)]


def bathroom_unit_cells(l):
    """graph.rs:605-625"""
    edges = []
    for x in range(l):
        for y in range(l):
            for i in range(4):
                va, vb = y * l * 4 + x * 4 + i, y * l * 4 + x * 4 + (i + 1) % 4
                edges.append(((min(va, vb), max(va, vb)), 1.0 if i == 0 else -1.0))
            va, vb = y * l * 4 + x * 4 + 1, y * l * 4 + ((x + 1) % l) * 4 + 3
            edges.append(((min(va, vb), max(va, vb)), -1.0))
            va, vb = y * l * 4 + x * 4, ((y + 1) % l) * l * 4 + x * 4 + 2
            edges.append(((min(va, vb), max(va, vb)), -1.0))
    return edges


def _cases():
    rng = np.random.default_rng(20)
    c = {}
    c["one_edge"] = ([((0, 1), 1.0)], [0.25, -0.5])
    c["triangle"] = ([((0, 1), 1.0), ((1, 2), 1.0), ((2, 0), 1.0)], [0.0, 0.0, 0.0])
    c["chain20"] = ([((x, x + 1), 1.0) for x in range(19)], [0.5] + [0.0] * 18 + [-0.25])
    c["lattice4x4"] = (lat.two_d_periodic(4), [0.0] * 16)  # two_d_periodic of the reference's test module (graph.rs:461-479)
    k8 = lat.complete(8)
    c["k8"] = ([(ab, float(j)) for (ab, _), j in zip(k8, _dyadic(rng, len(k8)))], [float(h) for h in _dyadic(rng, 8, -4, 4, nonzero=False)])
    c["star71"] = ([((0, v), 0.5 if v % 3 else -1.0) for v in range(1, 71)], [0.125 * ((v % 5) - 2) for v in range(71)])  # centre of degree 70
    c["duplicate_edge"] = ([((0, 1), 1.0), ((1, 2), -0.5), ((0, 1), 0.75), ((2, 0), 1.0), ((1, 0), 1.0)], [0.0, 0.25, 0.0])
    for n in (33, 64, 65):
        c[f"ring{n}"] = _ring(n, n)
    # non-uniform positive couplings: edge importance sampling
    c["k8_positive"] = ([(ab, abs(j)) for ab, j in c["k8"][0]], c["k8"][1])
    c["ring33_positive"] = ([(ab, abs(j)) for ab, j in c["ring33"][0]], c["ring33"][1])
    return c


CASES = _cases()
PARITY = ["one_edge", "triangle", "chain20", "lattice4x4", "k8", "star71", "duplicate_edge", "ring33", "ring64", "ring65"]
IMPORTANCE = ["k8_positive", "ring33_positive"]
BETAS5 = [0.0, 0.3, 1.0, 2.5, 1000.0]
SEED, OFFSET = 0x5EED0C1A551CA1, 3
# (kinds, t, nspin, nedge, nworm): every kind, only_basic, the reference's default counts, and the batch sizes of the kernel
RUNS = [(CR.KINDS_ALL, 6, None, None, None), (CR.KINDS_BASIC, 6, None, None, None), (CR.KINDS_SPIN, 2, 1, None, None),
        (CR.KINDS_SPIN, 2, 63, None, None), (CR.KINDS_SPIN, 2, 64, None, None), (CR.KINDS_SPIN, 2, 65, None, None),
        (CR.KINDS_SPIN, 2, 200, None, None), (CR.KINDS_EDGE, 2, None, 1, None), (CR.KINDS_EDGE, 2, None, 65, None),
        (CR.KINDS_EDGE, 2, None, 200, None), (CR.KINDS_WORM, 3, None, None, 2), (CR.KINDS_WORM_NO_DOUBLES, 3, None, None, 2)]


def betas(nreplicas):
    return (BETAS5 * ((nreplicas + 4) // 5))[:nreplicas]


@functools.lru_cache(maxsize=None)
def reference_chain(name, nreplicas, importance=False, replica_offset=OFFSET, runs=None):
    """The runs of RUNS one after the other from the random initial states, on the restatement: [(states [R][N], counters [R][8],
    epochs [R])] after each run (counters summed from the start)."""
    edges, biases = CASES[name]
    reps = [CR.RefGraphState(edges, biases, SEED, replica_offset + r, importance=importance) for r in range(nreplicas)]
    out = []
    for kinds, t, nspin, nedge, nworm in (RUNS if runs is None else runs):
        for g, beta in zip(reps, betas(nreplicas)):
            g.timesteps(t, beta, nspin=nspin, nedge=nedge, nworm=nworm, kinds=kinds)
        out.append((np.stack([g.state_bytes() for g in reps]), np.array([g.counters for g in reps], dtype=np.uint64),
                    np.array([g.epoch for g in reps], dtype=np.uint64)))
    return out


# ---- the layout cases: every table format, table placement and wave count of the launch plan ----
# in_lds / tables bits of classical.plan(): row starts 1, row entries 2, couplings 4, biases 8, edge list 16, cumulative weights 32
LAYOUT_R = 5
LAYOUT_BETAS = [0.0, 0.3, 1.0, 2.5, float("inf")]
LAYOUT_BETAS_SMALL_J = [0.0, 0.3, 4.0, 40.0, float("inf")]  # the non-compact cases: their couplings are small
# 130 moves: two full batches of 64 and a batch of 2; 70: a full batch and a batch of 6
LAYOUT_RUNS = [(CR.KINDS_SPIN, 2, 130, None, None), (CR.KINDS_EDGE, 2, None, 130, None),
               (CR.KINDS_WORM, 1, None, None, 2), (CR.KINDS_ALL, 3, 70, 70, 1)]
LAYOUT_MAX_VARS = 145632  # the most variables whose state bits and stamps fit the 40960 LDS words of one workgroup


def _signed(i, x):
    return -x if i % 3 == 0 else x


def distinct_ring(n, biased):
    """n distinct couplings +-(i + 1) / 256."""
    return [((i, (i + 1) % n), _signed(i, (i + 1) / 256.0)) for i in range(n)], [0.125 * ((v % 5) - 2) if biased else 0.0 for v in range(n)]


def distinct_lattice(l):
    """2 l^2 distinct couplings +-(i + 1) / 8192 on the l x l periodic lattice, three bias values."""
    return ([(ab, _signed(i, (i + 1) / 8192.0)) for i, (ab, _) in enumerate(lat.two_d_periodic(l))], [0.25 * ((v % 3) - 1) for v in range(l * l)])


def hightail(n, top=80):
    """n variables of which only the last `top` (and the first eight) have edges: a signed ring over them, chords, and eight edges
    down to the variables 0 .. 7.  The edge list is short, so the edge moves keep drawing endpoints near n."""
    lo = n - top
    edges = [((lo + i, lo + (i + 1) % top), _signed(i, ((i % 7) + 1) / 8.0)) for i in range(top)]
    edges += [((lo + i, lo + (i + 17) % top), 0.5) for i in range(0, top, 3)]
    edges += [((i, lo + i), -0.75) for i in range(8)]
    return edges, [0.0] * n


def random_graph(n, density):
    """min(density n, 600) edges (at least one) with random endpoints: multi-edges kept, self-loops redrawn."""
    rng = np.random.default_rng(1000 * n + density)
    pairs = []
    while len(pairs) < max(1, min(density * n, 600)):
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            pairs.append((a, b))
    return [(ab, float(j)) for ab, j in zip(pairs, _dyadic(rng, len(pairs)))], [float(h) for h in _dyadic(rng, n, -4, 4, nonzero=False)]


def _layout(graph, waves, in_lds, tables, compact=True, packed=True, betas=None, importance=False, lds_words=None):
    plan = dict(waves=waves, in_lds=in_lds, tables=tables, compact_couplings=compact, packed_edges=packed)
    if lds_words is not None:
        plan["lds_words"] = lds_words
    return dict(edges=graph[0], biases=graph[1], plan=plan, betas=LAYOUT_BETAS if betas is None else betas, importance=importance)


def _layout_cases():
    small = LAYOUT_BETAS_SMALL_J
    c = {}
    c["ring300_distinct"] = _layout(distinct_ring(300, True), 4, 31, 31, compact=False, betas=small)
    c["ring256_distinct"] = _layout(distinct_ring(256, False), 4, 23, 23)  # the dictionary's last size
    c["ring257_distinct"] = _layout(distinct_ring(257, False), 4, 23, 23, compact=False, betas=small)
    c["lat48_noncompact"] = _layout(distinct_lattice(48), 2, 31, 31, compact=False, betas=small, lds_words=40466)
    c["lat64_noncompact"] = _layout(distinct_lattice(64), 4, 11, 31, compact=False, betas=small)  # jv global, the biases in LDS behind it
    c["lat72"] = _layout((lat.two_d_periodic(72, lambda i, j, d: 1.0), [0.0] * 5184), 2, 23, 23)
    c["lat74"] = _layout((lat.two_d_periodic(74, lambda i, j, d: 1.0), [0.0] * 5476), 1, 23, 23)
    e64 = [(ab, 1.0 + 0.5 * (i % 2)) for i, (ab, _) in enumerate(lat.two_d_periodic(64))]
    c["lat64_bias_importance"] = _layout((e64, [0.25 * ((v % 3) - 1) for v in range(4096)]), 4, 15, 63, importance=True)  # edge list, cum global
    c["hightail65600"] = _layout(hightail(65600), 2, 22, 23, packed=False)  # two-word edges, the row starts global
    c["hightail100000"] = _layout(hightail(100000), 1, 22, 23, packed=False)
    c["hightail145632"] = _layout(hightail(LAYOUT_MAX_VARS), 1, 0, 23, packed=False, lds_words=40959)  # LDS filled to the last word but one
    return c


LAYOUT_CASES = _layout_cases()
LAYOUT_NONCOMPACT = [k for k, c in LAYOUT_CASES.items() if not c["plan"]["compact_couplings"]]
LAYOUT_HIGHTAIL = [k for k in LAYOUT_CASES if k.startswith("hightail")]
LAYOUT_SMALL = [k for k, c in LAYOUT_CASES.items() if len(c["biases"]) <= 5476]  # these also run serial and with the tables forced global
RANDOM_SIZES = (2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)  # around the 32 state bits and 4 stamp bytes of a word
RANDOM_CASES = {f"random{n}x{d}": dict(edges=g[0], biases=g[1], plan=None, betas=LAYOUT_BETAS, importance=False)
                for n in RANDOM_SIZES for d in (1, 4) for g in [random_graph(n, d)]}


def layout_case(name):
    return LAYOUT_CASES[name] if name in LAYOUT_CASES else RANDOM_CASES[name]


def layout_states(nvars):
    """The explicit initial states of a layout case, [LAYOUT_R][nvars]."""
    return np.random.default_rng(nvars).integers(0, 2, (LAYOUT_R, nvars), dtype=np.uint8)


def rotate_couplings(edges):
    """The same endpoints with every coupling moved on by one edge (a wrong coupling index reads a graph like this one)."""
    js = [j for _, j in edges]
    return [(ab, j) for (ab, _), j in zip(edges, js[-1:] + js[:-1])]


def truncate_endpoints(edges):
    """The endpoints cut to 16 bits (what a packed edge word would hold), the self-loops this makes dropped."""
    cut = [((a & 0xFFFF, b & 0xFFFF), j) for (a, b), j in edges]
    return [(ab, j) for ab, j in cut if ab[0] != ab[1]]


def run_reference(edges, biases, states, betas, runs, importance=False, epoch=0):
    """`runs` one after the other on the restatement, replica r with states[r], betas[r] and stream OFFSET + r:
    [(states [R][N], counters [R][8], epochs [R])] after each run, and the replicas."""
    reps = [CR.RefGraphState(edges, biases, SEED, OFFSET + r, state=None if states is None else states[r], importance=importance, epoch=epoch)
            for r in range(len(betas))]
    out = []
    for kinds, t, nspin, nedge, nworm in runs:
        for g, beta in zip(reps, betas):
            g.timesteps(t, beta, nspin=nspin, nedge=nedge, nworm=nworm, kinds=kinds)
        out.append((np.stack([g.state_bytes() for g in reps]), np.array([g.counters for g in reps], dtype=np.uint64),
                    np.array([g.epoch for g in reps], dtype=np.uint64)))
    return out, reps


@functools.lru_cache(maxsize=None)
def _layout_reference(name):
    c = layout_case(name)
    out, reps = run_reference(c["edges"], c["biases"], layout_states(len(c["biases"])), c["betas"], LAYOUT_RUNS, c["importance"])
    return out, np.array([g.get_energy() for g in reps])


def layout_reference_chain(name):
    """LAYOUT_RUNS from layout_states on the restatement, R = LAYOUT_R (replicas are independent: the first R' rows are the chain of a
    batch of R' replicas).  Cached; callers do not write into it."""
    return _layout_reference(name)[0]


def layout_reference_energies(name):
    """get_energy of the restatement's final states, [LAYOUT_R]."""
    return _layout_reference(name)[1]


EPOCH_STARTS = [2 ** 32 - 2, 2 ** 56 - 2]  # four steps from each cross 2^32 (epoch_hi24 becomes 1) and 2^56 (it wraps to 0)


@functools.lru_cache(maxsize=None)
def epoch_reference(start):
    """Four KINDS_ALL steps of ring33 with the default move counts from the random initial states, the epochs starting at `start`."""
    return run_reference(*CASES["ring33"], None, betas(5), [(CR.KINDS_ALL, 4, None, None, None)], epoch=start)[0][0]


# ---- exact enumeration (N <= 9) ----
def _enumeration_systems():
    rng = np.random.default_rng(7)
    ring = ([((i, (i + 1) % 9), 1.0 if i % 3 else -0.5) for i in range(9)], [0.5, -0.25, 0.0, 0.25, 0.0, -0.5, 0.25, 0.0, 0.25])
    f = lambda i, j: j * 2 + i  # 2 x 4 open ladder, antiferromagnetic rungs and legs with ferromagnetic diagonals: frustrated
    frus = []
    for j in range(4):
        frus.append(((f(0, j), f(1, j)), 1.0))
        if j < 3:
            frus += [((f(0, j), f(0, j + 1)), 1.0), ((f(1, j), f(1, j + 1)), 1.0), ((f(0, j), f(1, j + 1)), 0.5)]
    k5 = [(ab, float(j)) for (ab, _), j in zip(lat.complete(5), _dyadic(rng, 10))]
    return {"ring9_biased": ring, "frustrated2x4": (frus, [0.0] * 8), "k5_random": (k5, [0.0] * 5)}


ENUM_SYSTEMS = _enumeration_systems()
ENUM_BETAJ = [0.2, 0.6, 1.0]
ENUM_R, ENUM_STEPS, ENUM_SIGMAS = 8192, 48, 4.5


def enum_beta(name, betaj):
    return betaj / max(abs(j) for _, j in ENUM_SYSTEMS[name][0])


def enum_violations(name, betaj, states):
    """The observables of `states` [R][N] that miss the Boltzmann value by more than 4.5 sigma, sigma = the exact standard deviation
    over sqrt(R): [(observable, sampled mean, exact mean, sigma of the mean)]."""
    edges, biases = ENUM_SYSTEMS[name]
    exact = CR.exact_moments(edges, biases, enum_beta(name, betaj))
    got = CR.sample_moments(edges, biases, states)
    bad = []
    for obs, (mean, sd) in exact.items():
        sigma = sd / np.sqrt(len(states))
        if abs(got[obs].mean() - mean) > ENUM_SIGMAS * sigma:
            bad.append((obs, float(got[obs].mean()), mean, sigma))
    return bad


@functools.lru_cache(maxsize=None)
def enum_reference_states(name, betaj, bias_sign=1.0, edge_omit=True):
    edges, biases = ENUM_SYSTEMS[name]
    b = CR.BatchRef(edges, biases, SEED, ENUM_R, bias_sign=bias_sign, edge_omit=edge_omit)
    b.timesteps(ENUM_STEPS, enum_beta(name, betaj))
    return b.state.astype(np.uint8)
