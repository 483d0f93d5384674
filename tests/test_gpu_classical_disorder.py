"""Per-replica couplings on the device (GraphState(couplings=...), classical_steps_per_replica_kernel and the per-slot views of the
energies and tempering kernels) against the per-replica host entries, which tests/test_classical_disorder_cpu.py holds to the
shared-coupling path and to the numpy restatement.

The comparisons are exact although the device's exp may differ from libm's in the last place: a disagreement needs a 32-bit uniform
inside one ulp of an acceptance threshold (see tests/test_gpu_classical.py)."""
import numpy as np
import pytest

import _classical_cases as cc
import _classical_disorder_cases as dc
import _classical_pt_cases as pc
import _classical_reference as CR

pytestmark = pytest.mark.gpu

VARIANTS = ["batched", "serial", "global"]


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


def _flags(variant, importance=False):
    cl = _cl()
    return {"batched": 0, "serial": cl.CFG_SERIAL_MOVES, "global": cl.CFG_GLOBAL_TABLES}[variant] | (cl.CFG_EDGE_IMPORTANCE if importance else 0)


def _graph(edges, biases, couplings, variant="batched", importance=False, state=None, replica_offset=cc.OFFSET, flags=0):
    import isingmontecarlo_amd as im
    return im.GraphState(edges, biases, cc.SEED, state=state, nreplicas=len(couplings), replica_offset=replica_offset,
                         cfg_flags=_flags(variant, importance) | flags, couplings=couplings)


def _assert_chain(g, want, runs, betas, what):
    for (kinds, t, nspin, nedge, nworm), (ws, wc, we) in zip(runs, want):
        g.timesteps(t, betas, nspin, nedge, nworm, kinds=kinds)
        run = (what, kinds, t, nspin, nedge, nworm)
        assert np.array_equal(g.state_ref(), ws), (run, "states")
        assert np.array_equal(g.counters(), wc), (run, g.counters().tolist(), wc.tolist())
        assert np.array_equal(g.get_epoch(), we), (run, "epochs")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", dc.PARITY + dc.IMPORTANCE + ["dict256", "dict257", "order300"])
def test_device_matches_the_host_rows(name, variant):
    """R = 5 (dictionary cases: 2 and 3) at replica_offset = cc.OFFSET: the second workgroup holds one live wave, every wave of the first
    another realisation; the tables are indexed by the local replica, the Philox stream by the global one.  Random initial states,
    then every run of cc.RUNS.  dict256 / dict257: the dictionary's last size and the doubles; order300: sums that depend on their
    order; the two positive cases run with edge importance sampling."""
    e, b, cj, betas, imp = dc.case(name)
    g = _graph(e, b, cj, variant, imp)
    fmt = g.launch_plan()["coupling_format"]
    assert fmt == (2 if name in ("dict257", "order300") else 1)
    assert bool(g.launch_plan()["in_lds"] & 64) == (fmt == 1 and variant != "global")
    assert np.array_equal(g.state_ref(), dc.initial_states(len(cj), len(b)))
    _assert_chain(g, dc.host_per_replica_chain(name), cc.RUNS, betas, (name, variant))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["k8", "star71", "ring65"])
def test_a_single_replica(name, variant):
    """R = 1: the batch is row 0, the case's own couplings: the shared-coupling restatement chain of cc."""
    e, b, cj, betas, imp = dc.case(name)
    g = _graph(e, b, cj[:1], variant)
    _assert_chain(g, cc.reference_chain(name, 1), cc.RUNS, betas[:1], (name, variant))


@pytest.mark.parametrize("name", ["pmj48", "pmj64", "pmj72", "pmj64_global_codes"])
def test_layouts(name):
    """+-J realisations on the 48 x 48 (4 waves, codes in LDS), 64 x 64 (2 waves, codes in LDS; 4 waves with CFG_GLOBAL_CODES) and 72 x 72
    lattice (4 waves, codes and edge list in global memory): the plan first, then 130 spin moves, 130 edge moves, a worm step and
    mixed steps at R = 5."""
    c = dc.PLAN_CASES[name]
    e, b, cj = dc.lattice_pmj(c["l"])
    st = dc.layout_states(len(b))
    g = _graph(e, b, cj, state=st, flags=c["flags"])
    got = g.launch_plan()
    for k, v in c["plan"].items():
        assert got[k] == v, (name, k, got)
    want = dc.host_chain(e, b, cj, cc.LAYOUT_BETAS, cc.LAYOUT_RUNS, states=st)
    _assert_chain(g, want, cc.LAYOUT_RUNS, cc.LAYOUT_BETAS, name)
    assert (want[-1][0] != st).any(axis=1).all()


@pytest.mark.parametrize("name", ["k8", "ring65", "order300", "dict256"])
def test_energies(name):
    """get_energy of the batch = get_energy of R shared-coupling one-replica handles on couplings[r] with the same states, bit for bit."""
    import isingmontecarlo_amd as im
    e, b, cj, betas, imp = dc.case(name)
    g = _graph(e, b, cj)
    g.timesteps(3, betas)
    st = g.state_ref()
    want = np.array([im.GraphState(dc.with_couplings(e, cj[r]), b, cc.SEED, state=st[r], nreplicas=1, replica_offset=cc.OFFSET + r).get_energy()[0]
                     for r in range(len(cj))])
    got = g.get_energy()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert len(set(got.tolist())) > 1


def _assert_equals_host(g, want, what, series=None):
    assert np.array_equal(g.state_ref(), want["states"]), (what, "states")
    assert np.array_equal(g.get_epoch(), want["epochs"]), (what, "epochs")
    assert np.array_equal(g.counters(), want["counters"]), (what, "counters")
    assert np.array_equal(g.temperature_of(), want["temp_of"]), (what, g.temperature_of().tolist(), want["temp_of"].tolist())
    assert g.tempering_step_number() == want["pt_step"], (what, "pt_step")
    att, acc = g.swap_counts()
    assert np.array_equal(att, want["attempts"]) and np.array_equal(acc, want["accepts"]), (what, acc.tolist(), want["accepts"].tolist())
    if series is not None:
        assert np.array_equal(series["energy"], want["energy"]), (what, "energy series")
        assert np.array_equal(series["magnetization"], want["magnetization"]), (what, "magnetization series")


@pytest.mark.parametrize("mode", ["record", "no_record", "swaps_only"])
@pytest.mark.parametrize("name", list(dc.PT_CASES))
def test_tempering_matches_the_host_run(name, mode):
    """C realisations x T temperatures, 6 rounds of 2 KINDS_ALL steps: every output against host_tempering_run; also without the
    series, and with steps = 0 (swaps only)."""
    cl = _cl()
    e, b, betas, chains, cj = dc.pt_case(name)
    g = _graph(e, b, cj, replica_offset=len(betas))
    g.attach_tempering(betas)
    steps = 0 if mode == "swaps_only" else pc.PT_STEPS
    series = g.tempering_run(pc.PT_ROUNDS, steps, kinds=cl.KINDS_ALL, record=mode != "no_record")
    assert (series is None) == (mode == "no_record")
    _assert_equals_host(g, dc.pt_host_reference(name, True, steps), (name, mode), series)


def test_attach_refuses_rows_that_differ_inside_a_chain():
    import isingmontecarlo_amd as im
    e, b, betas, chains, cj = dc.pt_case("k8_T2")
    bad = cj.copy(); bad[3, 2] = -bad[3, 2]
    g = _graph(e, b, bad, replica_offset=2)
    with pytest.raises(im.IsingMcError) as ei:
        g.attach_tempering(betas)
    assert "chain 1" in str(ei.value) and "differ" in str(ei.value)
    g.timesteps(1, 1.0)  # the batch itself is fine
    _graph(e, b, cj, replica_offset=2).attach_tempering(betas)


# ---- composition ----
def test_checkpoint_format_3(tmp_path):
    """t = 10 equals 3 + 7 across save_checkpoint into a fresh handle; a handle with other couplings, or none, refuses the file."""
    import isingmontecarlo_amd as im
    e, b, cj, betas, _ = dc.case("k8")
    a, c = _graph(e, b, cj), _graph(e, b, cj)
    a.timesteps(10, betas)
    c.timesteps(3, betas)
    path = str(tmp_path / "c.npz")
    c.save_checkpoint(path)
    z = np.load(path)
    assert int(z["format"][0]) == 3 and np.array_equal(z["couplings"], cj) and "ladder" not in z.files
    d = _graph(e, b, cj)
    d.load_checkpoint(path)
    d.timesteps(7, betas)
    assert np.array_equal(a.state_ref(), d.state_ref()) and np.array_equal(a.get_epoch(), d.get_epoch()) and np.array_equal(a.counters(), d.counters())
    assert np.array_equal(a.state_ref(), dc.host_per_replica_chain("k8", ((CR.KINDS_ALL, 10, None, None, None),))[0][0])
    for other in (_graph(e, b, dc.rotate_rows(cj)), im.GraphState(e, b, cc.SEED, nreplicas=dc.R, replica_offset=cc.OFFSET)):
        with pytest.raises(im.IsingMcError):
            other.load_checkpoint(path)


def test_checkpoint_format_3_with_tempering(tmp_path):
    cl = _cl()
    e, b, betas, chains, cj = dc.pt_case("ring65_T3")
    a = _graph(e, b, cj, replica_offset=3)
    a.attach_tempering(betas)
    a.tempering_run(2, pc.PT_STEPS, kinds=cl.KINDS_ALL)
    path = str(tmp_path / "pt.npz")
    a.save_checkpoint(path)
    assert int(np.load(path)["format"][0]) == 3 and "ladder" in np.load(path).files
    d = _graph(e, b, cj, replica_offset=3)
    d.load_checkpoint(path)
    d.tempering_run(pc.PT_ROUNDS - 2, pc.PT_STEPS, kinds=cl.KINDS_ALL)
    _assert_equals_host(d, dc.pt_host_reference("ring65_T3"), "resumed")


def test_a_format_1_file_still_loads_into_a_shared_batch(tmp_path):
    import isingmontecarlo_amd as im
    e, b = cc.CASES["k8"]
    mk = lambda: im.GraphState(e, b, cc.SEED, nreplicas=5, replica_offset=cc.OFFSET)
    a, d = mk(), mk()
    a.timesteps(3, cc.betas(5))
    path = str(tmp_path / "one.npz")
    a.save_checkpoint(path)
    z = np.load(path)
    assert int(z["format"][0]) == 1 and "couplings" not in z.files and a.couplings is None
    d.load_checkpoint(path)
    a.timesteps(4, cc.betas(5)); d.timesteps(4, cc.betas(5))
    assert np.array_equal(a.state_ref(), d.state_ref()) and np.array_equal(a.counters(), d.counters())
    assert np.array_equal(a.state_ref(), cc.reference_chain("k8", 5, runs=((CR.KINDS_ALL, 7, None, None, None),))[0][0])
    with pytest.raises(im.IsingMcError):  # ... and not into a batch with couplings
        _graph(e, b, dc.realisations("k8")).load_checkpoint(path)


def test_importance_sampling_rebuild_keeps_the_couplings():
    """enable_edge_importance_sampling(True) then (False): couplings, states and epochs stay; the steps in between are those of the
    host entry with and without the flag."""
    cl = _cl()
    e, b, cj, betas, _ = dc.case("k8_positive")
    g = _graph(e, b, cj)
    g.timesteps(2, betas)
    st, ep = g.state_ref(), g.get_epoch()
    g.enable_edge_importance_sampling(True)
    assert np.array_equal(g.couplings, cj) and np.array_equal(g.state_ref(), st) and np.array_equal(g.get_epoch(), ep)
    assert g.launch_plan()["tables"] & 32 and g.launch_plan()["coupling_format"] == 1
    g.timesteps(3, betas)
    g.enable_edge_importance_sampling(False)
    assert np.array_equal(g.couplings, cj) and not g.launch_plan()["tables"] & 32
    g.timesteps(2, betas)
    h = cl.host_steps(e, b, cc.SEED, dc.initial_states(dc.R, 8), 0, 2, betas, replica_offset=cc.OFFSET, couplings=cj)
    h = cl.host_steps(e, b, cc.SEED, h[0], h[1], 3, betas, replica_offset=cc.OFFSET, couplings=cj, flags=cl.CFG_EDGE_IMPORTANCE)
    h = cl.host_steps(e, b, cc.SEED, h[0], h[1], 2, betas, replica_offset=cc.OFFSET, couplings=cj)
    assert np.array_equal(g.state_ref(), h[0]) and np.array_equal(g.get_epoch(), h[1]) and (h[1] == 7).all()


def test_new_from_graph_hands_over_the_realisations():
    """QmcIsingGraph.new_from_graph from a per-replica GraphState: the quantum batch has the same realisation per replica and starts
    from the classical states; a few timesteps later verify() holds for every replica."""
    import isingmontecarlo_amd as im
    import _lattices as lat
    edges = lat.two_d_periodic(4)
    cj = np.ascontiguousarray(np.random.default_rng(4).choice([-1.0, 1.0], (3, len(edges))))
    g = im.GraphState(edges, [0.0] * 16, cc.SEED, nreplicas=3, couplings=cj)
    g.timesteps(20, [0.5, 1.0, 2.0])
    assert g.edge_list() == [((a, b), j) for (a, b), j in edges] and [j for _, j in g.edge_list(2)] == cj[2].tolist()
    q = im.QmcIsingGraph.new_from_graph(g, 1.0, 0.0, 16, 4242, capacity=4096)
    assert q.nreplicas == 3 and np.array_equal(np.asarray(q.J).reshape(3, -1), g.couplings) and np.array_equal(g.couplings, cj)
    assert np.array_equal(q.state_ref(), g.state_ref())
    q.timesteps(10, 1.5)
    assert q.verify().all()
