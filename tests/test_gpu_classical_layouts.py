"""The classical Monte Carlo kernels (csrc/sse_classical.hip.h) on every table format, table placement and wave count of the launch
plan, against the Python restatement (tests/_classical_reference.py): couplings without the dictionary, the two-word
edge list, workgroups of 2 waves and of 1 wave, tables split between LDS and global memory, LDS filled to the last word, epochs
beyond 32 bits, beta = +inf, and random multigraphs around the word boundaries of the state bits and stamp bytes.

Each test first asserts that the handle's own launch (GraphState.launch_plan, chosen from the device's LDS size) is the one its case
is named for, so a device with another LDS size fails there and not by testing something else.  The comparisons are exact, as in
tests/test_gpu_classical.py (see its docstring); the couplings are dyadic, so the energies are exact as well."""
import numpy as np
import pytest

import _classical_cases as cc
import _classical_reference as CR

pytestmark = pytest.mark.gpu


def _flags(variant, c):
    import isingmontecarlo_amd.classical as cl
    return {"batched": 0, "serial": cl.CFG_SERIAL_MOVES, "global": cl.CFG_GLOBAL_TABLES}[variant] | (cl.CFG_EDGE_IMPORTANCE if c["importance"] else 0)


def _graph(name, variant="batched", nreplicas=cc.LAYOUT_R, state=True):
    import isingmontecarlo_amd as im
    c = cc.layout_case(name)
    init = cc.layout_states(len(c["biases"]))[:nreplicas] if state else None
    return im.GraphState(c["edges"], c["biases"], cc.SEED, state=init, nreplicas=nreplicas, replica_offset=cc.OFFSET, cfg_flags=_flags(variant, c))


def _assert_plan(g, name, variant):
    want = cc.LAYOUT_CASES[name]["plan"]
    if variant == "global":
        want = dict(want, in_lds=0, waves=4)
        want.pop("lds_words", None)
    p = g.launch_plan()
    assert {k: p[k] for k in want} == want, (name, variant, p)
    if variant == "global":
        assert p["lds_words"] == p["waves"] * p["wave_words"]


def _assert_layout_chain(g, name, variant, nreplicas=cc.LAYOUT_R):
    betas = cc.layout_case(name)["betas"][:nreplicas]
    for (kinds, t, nspin, nedge, nworm), (ws, wc, we) in zip(cc.LAYOUT_RUNS, cc.layout_reference_chain(name)):
        g.timesteps(t, betas, nspin, nedge, nworm, kinds=kinds)
        run = (name, variant, nreplicas, kinds, t, nspin, nedge, nworm)
        got = g.state_ref()
        assert np.array_equal(got, ws[:nreplicas]), (run, "states", np.argwhere(got != ws[:nreplicas])[:8].tolist())
        assert np.array_equal(g.counters(), wc[:nreplicas]), (run, g.counters().tolist(), wc[:nreplicas].tolist())
        assert np.array_equal(g.get_epoch(), we[:nreplicas]), (run, "epochs")
    got, want = g.get_energy(), cc.layout_reference_energies(name)[:nreplicas]
    assert np.array_equal(got, want), (name, variant, got.tolist(), want.tolist())


@pytest.mark.parametrize("variant,name", [("batched", n) for n in cc.LAYOUT_CASES] + [(v, n) for v in ("serial", "global") for n in cc.LAYOUT_SMALL])
def test_layout_cases_match_the_restatement(oracle, name, variant):
    """R = 5 from explicit states: the launch is the case's, then states, counters and epochs after each run of cc.LAYOUT_RUNS, then
    the energies kernel on the final states."""
    g = _graph(name, variant)
    _assert_plan(g, name, variant)
    _assert_layout_chain(g, name, variant)


@pytest.mark.parametrize("nreplicas", [1, 3])
def test_two_wave_workgroups_with_an_empty_wave(oracle, nreplicas):
    """lat72 runs two waves per workgroup: R = 1 and R = 3 leave the second wave of the last workgroup without a replica."""
    g = _graph("lat72", nreplicas=nreplicas)
    _assert_plan(g, "lat72", "batched")
    _assert_layout_chain(g, "lat72", "batched", nreplicas)


@pytest.mark.parametrize("variant", ["batched", "serial"])
@pytest.mark.parametrize("name", list(cc.RANDOM_CASES))
def test_random_multigraphs_match_the_restatement(oracle, name, variant):
    """Multi-edges, isolated variables and dense rows at N = 2 .. 257, around the 32 state bits and the 4 stamp bytes of an LDS word."""
    _assert_layout_chain(_graph(name, variant), name, variant)


def test_random_initial_states_beyond_65536_variables(oracle):
    g = _graph("hightail65600", state=False)
    idx = np.arange(65600, dtype=np.uint64)
    want = CR.philox_np(cc.SEED, idx[None, :], 0, (np.arange(cc.LAYOUT_R, dtype=np.uint64) + np.uint64(cc.OFFSET))[:, None], CR.TAG_INIT)[..., 0] >> np.uint64(31)
    assert np.array_equal(g.state_ref(), want.astype(np.uint8))


@pytest.mark.parametrize("start", cc.EPOCH_STARTS)
def test_epochs_beyond_32_bits(oracle, start):
    """epoch_hi24 of the Philox counter on the device: four steps of ring33 across 2^32 and across 2^56."""
    import isingmontecarlo_amd as im
    g = im.GraphState(*cc.CASES["ring33"], cc.SEED, nreplicas=5, replica_offset=cc.OFFSET)
    g.set_epoch(start)
    g.timesteps(4, cc.betas(5))
    ws, wc, we = cc.epoch_reference(start)
    assert np.array_equal(g.state_ref(), ws) and np.array_equal(g.counters(), wc), (g.counters().tolist(), wc.tolist())
    assert np.array_equal(g.get_epoch(), we) and (g.get_epoch() == np.uint64(start + 4)).all()
