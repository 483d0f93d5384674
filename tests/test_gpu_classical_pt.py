"""Classical parallel tempering on the device (GraphState.attach_tempering / tempering_run, csrc/sse_classical_pt.hip.h) against
isingmc_classical_host_pt_run, the same rounds by the sequential rule on the CPU, which tests/test_classical_pt_cpu.py holds to the
numpy restatement and to exact enumeration.

The comparisons are exact although the device's exp may differ from libm's in the last place: a disagreement needs a 32-bit uniform
inside one ulp of an acceptance threshold (see tests/test_gpu_classical.py), in a swap as in a move."""
import ctypes as C

import numpy as np
import pytest

import _classical_cases as cc
import _classical_pt_cases as pc
import _classical_reference as CR

pytestmark = pytest.mark.gpu


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


def _flags(variant):
    cl = _cl()
    return {"batched": 0, "serial": cl.CFG_SERIAL_MOVES, "global": cl.CFG_GLOBAL_TABLES}[variant]


def _graph(edges, biases, betas, chains, replica_offset=0, cfg_flags=0, attach=True):
    import isingmontecarlo_amd as im
    g = im.GraphState(edges, biases, cc.SEED, nreplicas=chains * len(betas), replica_offset=replica_offset, cfg_flags=cfg_flags)
    if attach:
        g.attach_tempering(betas)
    return g


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


@pytest.mark.parametrize("variant", pc.PT_VARIANTS)
@pytest.mark.parametrize("name", list(pc.PT_CASES))
def test_device_matches_the_host_run(name, variant):
    """6 rounds of 2 KINDS_ALL steps in one call: states, epochs, move counters, temp_of, swap counts and the E and M series, for the
    batched kernel, the one-move-at-a-time variant and the tables forced to global memory."""
    cl = _cl()
    c = pc.PT_CASES[name]
    g = _graph(c["edges"], c["biases"], c["betas"], c["chains"], pc.pt_offset(name), _flags(variant))
    series = g.tempering_run(pc.PT_ROUNDS, pc.PT_STEPS, kinds=cl.KINDS_ALL)
    _assert_equals_host(g, pc.host_parity_reference(name), (name, variant), series)
    slot_at = g.slot_at()
    assert np.array_equal(np.take_along_axis(g.temperature_of().reshape(slot_at.shape), slot_at.astype(np.int64), axis=1),
                          np.broadcast_to(np.arange(slot_at.shape[1]), slot_at.shape))
    by_t = g.states_by_temperature()
    st = g.state_ref().reshape(slot_at.shape + (-1,))
    assert all(np.array_equal(by_t[k, t], st[k, slot_at[k, t]]) for k in range(slot_at.shape[0]) for t in range(0, slot_at.shape[1], 7))


RING = cc.CASES["ring33"]
LADDER4 = [0.2, 0.5, 1.0, 2.0]


def _host_ring(chains, rounds, steps=2, replica_offset=0, **kw):
    cl = _cl()
    return pc.host_run(cl, RING[0], RING[1], LADDER4, chains, rounds, steps, replica_offset=replica_offset, kinds=cl.KINDS_ALL, **kw)


def test_calls_compose():
    """10 rounds in one call = 3 + 7 in two calls = 3 + 7 across a checkpoint into a fresh handle."""
    cl = _cl()
    want = _host_ring(4, 10)
    a, b = _graph(*RING, LADDER4, 4), _graph(*RING, LADDER4, 4)
    sa = a.tempering_run(10, 2, kinds=cl.KINDS_ALL)
    _assert_equals_host(a, want, "one call", sa)
    s3, s7 = b.tempering_run(3, 2, kinds=cl.KINDS_ALL), b.tempering_run(7, 2, kinds=cl.KINDS_ALL)
    _assert_equals_host(b, want, "two calls", {k: np.concatenate([s3[k], s7[k]]) for k in s3})


def test_checkpoint_resumes_a_tempering_run(tmp_path):
    cl = _cl()
    want = _host_ring(4, 10)
    c = _graph(*RING, LADDER4, 4)
    c.tempering_run(3, 2, kinds=cl.KINDS_ALL)
    path = str(tmp_path / "pt.npz")
    c.save_checkpoint(path)
    z = np.load(path)
    assert int(z["format"][0]) == 2 and np.array_equal(z["ladder"], LADDER4) and int(z["pt_step"][0]) == 3
    assert np.array_equal(z["temp_of"], c.temperature_of()) and z["swap_attempts"].shape == (4, 3) and (z["swap_attempts"] == 3).all()
    d = _graph(*RING, LADDER4, 4, attach=False)  # the file brings the ladder
    d.load_checkpoint(path)
    s7 = d.tempering_run(7, 2, kinds=cl.KINDS_ALL)
    _assert_equals_host(d, want, "checkpoint")
    assert np.array_equal(s7["energy"], want["energy"][3:]) and np.array_equal(s7["magnetization"], want["magnetization"][3:])


def test_chains_shard_over_handles():
    """4 chains in one handle = two handles of 2 chains at replica_offset 0 and 2 T."""
    cl = _cl()
    whole = _graph(*RING, LADDER4, 4)
    lo, hi = _graph(*RING, LADDER4, 2, 0), _graph(*RING, LADDER4, 2, 8)
    sw, sl, sh = (g.tempering_run(5, 2, kinds=cl.KINDS_ALL) for g in (whole, lo, hi))
    assert np.array_equal(whole.state_ref(), np.concatenate([lo.state_ref(), hi.state_ref()]))
    assert np.array_equal(whole.temperature_of(), np.concatenate([lo.temperature_of(), hi.temperature_of()]))
    assert np.array_equal(whole.swap_counts()[1], np.concatenate([lo.swap_counts()[1], hi.swap_counts()[1]]))
    assert np.array_equal(sw["energy"], np.concatenate([sl["energy"], sh["energy"]], axis=1))
    assert whole.swap_counts()[1].sum() > 0


def test_series_is_optional_and_steps_may_be_zero():
    cl = _cl()
    a, b = _graph(*RING, LADDER4, 4), _graph(*RING, LADDER4, 4)
    assert a.tempering_run(10, 2, kinds=cl.KINDS_ALL, record=False) is None
    b.tempering_run(10, 2, kinds=cl.KINDS_ALL, record=True)
    assert np.array_equal(a.state_ref(), b.state_ref()) and np.array_equal(a.temperature_of(), b.temperature_of())
    c = _graph(*RING, LADDER4, 4)
    before = c.state_ref()
    s = c.tempering_run(0, 2)
    assert s["energy"].shape == (0, 4, 4) and c.tempering_step_number() == 0 and np.array_equal(c.state_ref(), before)
    s = c.tempering_run(5, 0)  # swaps only
    _assert_equals_host(c, _host_ring(4, 5, steps=0), "swaps only", s)
    assert np.array_equal(c.state_ref(), before) and c.swap_counts()[1].sum() > 0


def test_energy_series_is_get_energy_of_the_states():
    """k8 has dyadic couplings and biases: every order of additions gives the same sum, so the series equals the restatement's
    get_energy of the states exactly, round by round with steps = 1; the magnetisation is the sum of the spins."""
    cl = _cl()
    edges, biases = cc.CASES["k8"]
    g = _graph(edges, biases, [0.2, 0.6, 1.0], 2)
    for _ in range(4):
        before = g.temperature_of()
        s = g.tempering_run(1, 1, kinds=cl.KINDS_ALL)
        st = g.state_ref()
        for r in range(6):
            assert s["energy"][0, r // 3, before[r]] == CR.get_energy(edges, biases, st[r])
            assert s["magnetization"][0, r // 3, before[r]] == 2 * int(st[r].sum()) - 8
    assert np.array_equal(g.get_energy(), [CR.get_energy(edges, biases, x) for x in g.state_ref()])


@pytest.mark.parametrize("name", list(cc.ENUM_SYSTEMS))
def test_device_samples_the_boltzmann_distribution_at_every_temperature(name):
    """The inputs of the CPU enumeration test on the device: 2048 chains of T = 4, 48 rounds of one only_basic_moves step, the states
    at every temperature and the mean of the E series from round 24 on within 4.5 sigma of the enumerated values.  The device equals
    the host entry bit for bit (the parity tests above), so the CPU run predicts the outcome: at most 2.0 sigma in the states and 1.8
    in the series."""
    edges, biases = cc.ENUM_SYSTEMS[name]
    g = _graph(edges, biases, pc.enum_pt_betas(name), pc.ENUM_PT_CHAINS)
    s = g.tempering_run(pc.ENUM_PT_ROUNDS, 1, only_basic_moves=True)
    assert g.nreplicas == cc.ENUM_R and (g.get_epoch() == pc.ENUM_PT_ROUNDS).all()
    assert pc.enum_pt_violations(name, g.states_by_temperature()) == []
    sigmas = pc.enum_pt_series_sigmas(name, s["energy"])
    assert max(sigmas) <= cc.ENUM_SIGMAS, sigmas
    att, acc = g.swap_counts()
    assert (att == pc.ENUM_PT_ROUNDS).all() and (acc.sum(axis=0) / att.sum(axis=0) > 0.3).all()


def test_importance_sampling_rebuild_keeps_the_tempering_state():
    cl = _cl()
    edges, biases = cc.CASES["ring33_positive"]
    g = _graph(edges, biases, LADDER4, 2)
    g.tempering_run(4, 2, kinds=cl.KINDS_ALL)
    tof, step, (att, acc) = g.temperature_of(), g.tempering_step_number(), g.swap_counts()
    st, ep, ctr = g.state_ref(), g.get_epoch(), g.counters()
    g.enable_edge_importance_sampling(True)
    assert np.array_equal(g.temperature_of(), tof) and g.tempering_step_number() == step == 4
    assert np.array_equal(g.swap_counts()[0], att) and np.array_equal(g.swap_counts()[1], acc)
    s = g.tempering_run(3, 2, kinds=cl.KINDS_ALL)
    want = cl.host_tempering_run(edges, biases, cc.SEED, st, ep, LADDER4, 3, 2, kinds=cl.KINDS_ALL, temp_of=tof, pt_step=step, flags=cl.CFG_EDGE_IMPORTANCE)
    want["counters"] = want["counters"] + ctr
    want["attempts"], want["accepts"] = want["attempts"] + att, want["accepts"] + acc
    _assert_equals_host(g, want, "after the rebuild", s)


# ---- existing behaviour ----
def test_timesteps_on_an_attached_handle_are_those_of_a_plain_one():
    a, b = _graph(*RING, LADDER4, 2), _graph(*RING, LADDER4, 2, attach=False)
    cl = _cl()
    a.tempering_run(2, 1)  # the labels have moved
    tof, (att, acc) = a.temperature_of(), a.swap_counts()
    b.set_state(a.state_ref())
    b.set_epoch(a.get_epoch())
    beta = cc.betas(8)
    a.timesteps(5, beta)
    b.timesteps(5, beta)
    assert np.array_equal(a.state_ref(), b.state_ref()) and np.array_equal(a.get_epoch(), b.get_epoch())
    assert np.array_equal(a.temperature_of(), tof) and a.tempering_step_number() == 2  # the maps are left alone
    assert np.array_equal(a.swap_counts()[0], att) and np.array_equal(a.swap_counts()[1], acc)
    st, ep = a.state_ref(), a.get_epoch()
    s = a.tempering_run(2, 1, kinds=cl.KINDS_ALL)  # and the next round reads the ladder through the maps, not the betas of timesteps
    want = cl.host_tempering_run(RING[0], RING[1], cc.SEED, st, ep, LADDER4, 2, 1, kinds=cl.KINDS_ALL, temp_of=tof, pt_step=2)
    assert np.array_equal(a.state_ref(), want["states"]) and np.array_equal(a.temperature_of(), want["temp_of"])
    assert np.array_equal(s["energy"], want["energy"])


def test_a_checkpoint_without_tempering_is_the_format_1_file(tmp_path):
    """The same entries, values and dtypes as before tempering existed, and it loads into an attached handle without touching the maps."""
    plain = _graph(*RING, LADDER4, 2, attach=False)
    plain.timesteps(3, cc.betas(8))
    path = str(tmp_path / "plain.npz")
    plain.save_checkpoint(path)
    z = np.load(path)
    want = dict(format=np.array([1], dtype=np.uint32), edges=plain.edges, J=plain.J, biases=plain.biases, seed=np.array([cc.SEED], dtype=np.uint64),
                replica_offset=np.array([0], dtype=np.uint32), importance=np.array([False]), state=plain.state_ref(), epoch=plain.get_epoch(),
                counters=plain.counters())
    assert list(z.keys()) == list(want)
    for k, v in want.items():
        assert z[k].dtype == v.dtype and np.array_equal(z[k], v), k
    other = _graph(*RING, LADDER4, 2)
    other.tempering_run(2, 1)
    tof = other.temperature_of()
    other.load_checkpoint(path)  # format 1 still loads
    assert np.array_equal(other.state_ref(), plain.state_ref()) and np.array_equal(other.get_epoch(), plain.get_epoch())
    assert np.array_equal(other.temperature_of(), tof) and other.tempering_step_number() == 2


def test_maps_are_checked_and_attach_comes_first():
    cl = _cl()
    import isingmontecarlo_amd as im
    g = _graph(*RING, LADDER4, 2, attach=False)
    lib, h = g._lib, g._h
    buf32, buf64, step = np.zeros(8, dtype=np.uint32), np.zeros(6, dtype=np.uint64), C.c_uint64(0)
    for rc in (lib.isingmc_classical_pt_run(h, 1, 1, cl.NONE, cl.NONE, cl.NONE, 0, None, None),
               lib.isingmc_classical_pt_get(h, im._ptr(buf32, C.c_uint32), C.byref(step)),
               lib.isingmc_classical_pt_set(h, im._ptr(buf32, C.c_uint32), 0),
               lib.isingmc_classical_pt_swap_counts(h, im._ptr(buf64, C.c_uint64), im._ptr(buf64, C.c_uint64))):
        assert rc == -1 and b"isingmc_classical_pt_attach first" in lib.isingmc_classical_last_error(h)
    with pytest.raises(im.IsingMcError):
        g.tempering_run(1, 1)
    for betas, words in (([1.0], "ntemps >= 2"), ([0.1, 0.2, 0.3], "multiple of ntemps"), ([0.1, float("inf")], "finite")):
        with pytest.raises(im.IsingMcError) as ei:
            g.attach_tempering(betas)
        assert ei.value.code == -1 and words in str(ei.value)
    assert lib.isingmc_classical_pt_attach(h, 4, None) == -1 and b"non-null" in lib.isingmc_classical_last_error(h)
    with pytest.raises(im.IsingMcError) as ei:
        _graph(*RING, LADDER4, 2, replica_offset=2)
    assert "replica_offset must be a multiple" in str(ei.value)
    g.attach_tempering(LADDER4)
    for bad in ([0, 1, 2, 2, 0, 1, 2, 3], [0, 1, 2, 4, 0, 1, 2, 3], [0, 1, 2, 3, 3, 2, 1, 1]):
        with pytest.raises(im.IsingMcError) as ei:
            g.set_temperature_of(bad)
        assert ei.value.code == -1 and "permutation" in str(ei.value)
    assert np.array_equal(g.temperature_of(), np.arange(8) % 4)  # refused: nothing changed
    g.set_temperature_of([3, 2, 1, 0, 0, 1, 3, 2], pt_step=7)
    assert np.array_equal(g.slot_at(), [[3, 2, 1, 0], [0, 1, 3, 2]]) and g.tempering_step_number() == 7
    g.tempering_run(2, 1)
    g.attach_tempering(LADDER4)  # attaching again resets the maps, the counters and the step number
    assert np.array_equal(g.temperature_of(), np.arange(8) % 4) and g.tempering_step_number() == 0 and g.swap_counts()[0].sum() == 0
