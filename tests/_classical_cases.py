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
