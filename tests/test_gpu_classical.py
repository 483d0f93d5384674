"""Classical Monte Carlo on the device (isingmontecarlo_amd.GraphState, csrc/sse_classical.hip.h) against the Python restatement of
graph.rs (tests/_classical_reference.py): the batched kernel, its one-move-at-a-time variant and the tables forced to global memory.

The comparisons are exact although the device's exp may differ from libm's in the last place: a disagreement needs a 32-bit uniform
inside one ulp of the acceptance threshold (probability about 2^-32 * 2^-20 per move with a positive energy change), far below 1e-9
over all the moves made here."""
import numpy as np
import pytest

import _classical_cases as cc
import _classical_reference as CR
import _lattices as lat

pytestmark = pytest.mark.gpu

VARIANTS = ["batched", "serial", "global"]


def _flags(variant, importance=False):
    import isingmontecarlo_amd.classical as cl
    return {"batched": 0, "serial": cl.CFG_SERIAL_MOVES, "global": cl.CFG_GLOBAL_TABLES}[variant] | (cl.CFG_EDGE_IMPORTANCE if importance else 0)


def _graph(name, nreplicas, variant="batched", importance=False, replica_offset=cc.OFFSET, state=None, cases=cc.CASES):
    import isingmontecarlo_amd as im
    edges, biases = cases[name]
    return im.GraphState(edges, biases, cc.SEED, state=state, nreplicas=nreplicas, replica_offset=replica_offset, cfg_flags=_flags(variant, importance))


def _assert_chain(g, want, runs, nreplicas, what):
    for (kinds, t, nspin, nedge, nworm), (ws, wc, we) in zip(runs, want):
        g.timesteps(t, cc.betas(nreplicas), nspin, nedge, nworm, kinds=kinds)
        run = (what, kinds, t, nspin, nedge, nworm)
        assert np.array_equal(g.state_ref(), ws), (run, "states")
        assert np.array_equal(g.counters(), wc), (run, g.counters().tolist(), wc.tolist())
        assert np.array_equal(g.get_epoch(), we), (run, "epochs")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", cc.PARITY + cc.IMPORTANCE)
def test_device_matches_the_restatement(oracle, name, variant):
    """R = 5 at four replicas per workgroup (the last workgroup is partly empty): random initial states, then every run of cc.RUNS:
    states, counters and epochs after each.  k8: almost every batch is disturbed; star71: rows longer than a wave."""
    imp = name in cc.IMPORTANCE
    g = _graph(name, 5, variant, imp)
    assert np.array_equal(g.state_ref(), np.stack([CR.random_state(cc.SEED, cc.OFFSET + r, g.nvars) for r in range(5)]))
    _assert_chain(g, cc.reference_chain(name, 5, imp), cc.RUNS, 5, (name, variant))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["k8", "star71", "ring65"])
def test_a_single_replica(oracle, name, variant):
    _assert_chain(_graph(name, 1, variant), cc.reference_chain(name, 1), cc.RUNS, 1, (name, variant))


LATTICE_RUNS = ((CR.KINDS_BASIC, 3, None, None, None), (CR.KINDS_WORM, 1, None, None, 1))


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_64x64_lattice(oracle, variant):
    """Real table sizes: N = 4096, E = 8192, the reference's default move counts (2048 spin or 4096 edge moves a step), R = 4."""
    import isingmontecarlo_amd.classical as cl
    cases = {"lattice64x64": (lat.two_d_periodic(64), [0.0] * 4096)}
    p = cl.plan(*cases["lattice64x64"], flags=_flags(variant))
    assert (p["in_lds"] == 0) == (variant == "global")
    want = _reference_lattice()
    _assert_chain(_graph("lattice64x64", 4, variant, cases=cases), want, LATTICE_RUNS, 4, ("lattice64x64", variant))


_LATTICE = []


def _reference_lattice():
    if not _LATTICE:
        edges, biases = lat.two_d_periodic(64), [0.0] * 4096
        reps = [CR.RefGraphState(edges, biases, cc.SEED, cc.OFFSET + r) for r in range(4)]
        for kinds, t, nspin, nedge, nworm in LATTICE_RUNS:
            for g, beta in zip(reps, cc.betas(4)):
                g.timesteps(t, beta, nspin=nspin, nedge=nedge, nworm=nworm, kinds=kinds)
            _LATTICE.append((np.stack([g.state_bytes() for g in reps]), np.array([g.counters for g in reps], dtype=np.uint64),
                             np.array([g.epoch for g in reps], dtype=np.uint64)))
    return _LATTICE


def test_tables_partly_in_lds(oracle):
    """A 128 x 128 lattice: the row starts and the coupling dictionary fit in LDS next to four waves' areas, the row entries and the
    edge list do not and are read from global memory (the plan says so); spin and edge moves, R = 5."""
    import isingmontecarlo_amd.classical as cl
    cases = {"lattice128x128": (lat.two_d_periodic(128), [0.0] * 16384)}
    p = cl.plan(*cases["lattice128x128"])
    assert p["in_lds"] == 1 | 4 and p["tables"] == 1 | 2 | 4 | 16 and p["waves"] == 4
    runs = ((CR.KINDS_SPIN, 1, 300, None, None), (CR.KINDS_EDGE, 1, None, 300, None))
    reps = [CR.RefGraphState(*cases["lattice128x128"], cc.SEED, cc.OFFSET + r, state=np.zeros(16384, dtype=np.uint8)) for r in range(5)]
    want = []
    for kinds, t, nspin, nedge, nworm in runs:
        for g, beta in zip(reps, cc.betas(5)):
            g.timesteps(t, beta, nspin=nspin, nedge=nedge, nworm=nworm, kinds=kinds)
        want.append((np.stack([g.state_bytes() for g in reps]), np.array([g.counters for g in reps], dtype=np.uint64), np.array([g.epoch for g in reps], dtype=np.uint64)))
    g = _graph("lattice128x128", 5, state=np.zeros(16384, dtype=np.uint8), cases=cases)
    _assert_chain(g, want, runs, 5, "lattice128x128")
    assert want[-1][0].any()


@pytest.mark.parametrize("name", ["k8", "lattice4x4"])
def test_calls_compose(name):
    """t = 10 in one call = ten calls of t = 1 = 3 + 7 with the states and epochs carried into a fresh handle."""
    beta = cc.betas(5)
    a, b, c = _graph(name, 5), _graph(name, 5), _graph(name, 5)
    a.timesteps(10, beta)
    for _ in range(10):
        b.do_time_step(beta)
    c.timesteps(3, beta)
    d = _graph(name, 5, state=c.state_ref())
    d.set_epoch(c.get_epoch())
    d.timesteps(7, beta)
    assert (a.get_epoch() == 10).all()
    for other in (b, d):
        assert np.array_equal(a.state_ref(), other.state_ref()) and np.array_equal(a.get_epoch(), other.get_epoch())
    assert np.array_equal(a.counters(), b.counters()) and np.array_equal(a.counters(), c.counters() + d.counters())


def test_replica_offsets_shard_a_batch():
    """Replicas 0-7 in one handle = two handles of four with replica_offset 0 and 4."""
    beta = np.array(cc.betas(8))
    whole = _graph("ring33", 8, replica_offset=0)
    lo, hi = _graph("ring33", 4, replica_offset=0), _graph("ring33", 4, replica_offset=4)
    assert np.array_equal(whole.state_ref(), np.concatenate([lo.state_ref(), hi.state_ref()]))
    for g, b in ((whole, beta), (lo, beta[:4]), (hi, beta[4:])):
        g.timesteps(5, b)
    assert np.array_equal(whole.state_ref(), np.concatenate([lo.state_ref(), hi.state_ref()]))
    assert np.array_equal(whole.counters(), np.concatenate([lo.counters(), hi.counters()]))


@pytest.mark.parametrize("name", ["k8", "star71", "ring65", "duplicate_edge"])
def test_energies(name):
    """get_energy against the restatement's, within (2E + N) 2^-52 (sum |J| + sum |h|): the bound of any summation order (0 for
    dyadic couplings, which these are)."""
    edges, biases = cc.CASES[name]
    g = _graph(name, 5)
    g.timesteps(3, cc.betas(5))
    want = np.array([CR.get_energy(edges, biases, s) for s in g.state_ref()])
    bound = (2 * len(edges) + len(biases)) * 2.0 ** -52 * (sum(abs(j) for _, j in edges) + sum(abs(h) for h in biases))
    got = g.get_energy()
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)


@pytest.mark.parametrize("variant", ["batched", "serial"])
@pytest.mark.parametrize("name,betaj", [(name, bj) for name in cc.ENUM_SYSTEMS for bj in cc.ENUM_BETAJ])
def test_device_samples_the_boltzmann_distribution(name, betaj, variant):
    """The enumeration statistics of tests/test_classical_cpu.py on the device: R = 8192, 48 only_basic_moves steps, 4.5 sigma."""
    import isingmontecarlo_amd as im
    edges, biases = cc.ENUM_SYSTEMS[name]
    g = im.GraphState(edges, biases, cc.SEED, nreplicas=cc.ENUM_R, cfg_flags=_flags(variant))
    g.timesteps(cc.ENUM_STEPS, cc.enum_beta(name, betaj), only_basic_moves=True)
    assert cc.enum_violations(name, betaj, g.state_ref()) == []


def test_counters_count_the_attempts():
    g = _graph("ring64", 5)
    n, e = 64, 64
    g.timesteps(4, 1.0, kinds=CR.KINDS_SPIN)
    g.timesteps(3, 1.0, nedgeupdates=70, kinds=CR.KINDS_EDGE)
    g.timesteps(2, 1.0, nwormupdates=5, kinds=CR.KINDS_WORM)
    c = g.counters()
    assert (c[:, CR.C_SPIN] == 4 * (n // 2)).all() and (c[:, CR.C_EDGE] == 3 * 70).all() and (c[:, CR.C_WORM] == 2 * 5).all()
    assert (c[:, CR.C_SPIN_ACC] <= c[:, CR.C_SPIN]).all() and (c[:, CR.C_EDGE_ACC] <= c[:, CR.C_EDGE]).all()
    assert (c[:, CR.C_WORM_ACC] + c[:, CR.C_WORM_FAIL] <= c[:, CR.C_WORM]).all() and (c[:, CR.C_WORM_PATH] >= 2 * c[:, CR.C_WORM]).all()
    g.timesteps(6, 1.0, only_basic_moves=True)
    d = g.counters() - c
    assert ((d[:, CR.C_SPIN] // (n // 2)) + (d[:, CR.C_EDGE] // (e // 2)) == 6).all() and (d[:, CR.C_WORM] == 0).all()


def test_checkpoint_resumes_bit_exactly(tmp_path):
    beta = cc.betas(5)
    a = _graph("k8_positive", 5)
    a.enable_edge_importance_sampling(True)
    a.timesteps(4, beta)
    a.save_checkpoint(str(tmp_path / "c.npz"))
    a.timesteps(5, beta)
    b = _graph("k8_positive", 5)
    b.load_checkpoint(str(tmp_path / "c.npz"))
    b.timesteps(5, beta)
    assert np.array_equal(a.state_ref(), b.state_ref()) and np.array_equal(a.get_epoch(), b.get_epoch()) and np.array_equal(a.counters(), b.counters())
    want = cc.reference_chain("k8_positive", 5, True, runs=((CR.KINDS_ALL, 9, None, None, None),))[0]
    assert np.array_equal(a.state_ref(), want[0]) and np.array_equal(a.counters(), want[1])


def test_new_from_graph_hands_the_states_to_the_quantum_sampler(oracle):
    """QmcIsingGraph::new_from_graph (qmc_ising.rs:151-166): the quantum batch starts from the classical states, and 20 SSE
    timesteps from there are the oracle's from the same states."""
    import isingmontecarlo_amd as im
    edges = lat.two_d_periodic(4)
    cg = im.GraphState(edges, [0.0] * 16, cc.SEED, nreplicas=3)
    cg.timesteps(20, [0.5, 1.0, 2.0])
    states = cg.state_ref()
    q = im.new_qmc_from_graph(cg, 1.0, 0.0, 16, 4242, capacity=4096)
    assert np.array_equal(q.state_ref(), states) and q.nreplicas == 3
    e, j = lat.split(edges)
    m = oracle.Model(16, e, j, 1.0, 0.0)
    reps = [oracle.Replica(m, 4096, 16, 4242, r, states[r]) for r in range(3)]
    q.run(20, 1.5)
    for r, rep in enumerate(reps):
        rep.timesteps(20, 1.5)
        assert np.array_equal(q.state_ref()[r], rep.state()) and np.array_equal(q.export_ops(r), rep.ops()) and q.get_n()[r] == rep.n
