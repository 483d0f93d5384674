"""Classical Monte Carlo without a device: the sequential rule of csrc/classical_rule.h (isingmc_classical_host_steps) against the
Python restatement of graph.rs (tests/_classical_reference.py), the reference's own worm known answers, exact enumeration, the launch
plan and the ABI of the new entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _classical_cases as cc
import _classical_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


def test_numpy_philox_is_the_oracles(oracle):
    idx = np.array([0, 1, 77, 2 ** 32 - 1], dtype=np.uint64)
    got = CR.philox_np(cc.SEED, idx[:, None], (1 << 40) + 5, np.array([0, 9], dtype=np.uint64)[None, :], CR.TAG_CLASSICAL)
    for i, ix in enumerate(idx):
        for j, rep in enumerate((0, 9)):
            assert [int(x) for x in got[i, j]] == CR.philox(cc.SEED, int(ix), (1 << 40) + 5, rep, CR.TAG_CLASSICAL)


def _host_chain(name, nreplicas, importance=False):
    """cc.RUNS one after the other through isingmc_classical_host_steps, from the restatement's random initial states."""
    cl = _cl()
    edges, biases = cc.CASES[name]
    st = np.stack([CR.random_state(cc.SEED, cc.OFFSET + r, len(biases)) for r in range(nreplicas)])
    ep = np.zeros(nreplicas, dtype=np.uint64)
    total = np.zeros((nreplicas, 8), dtype=np.uint64)
    out = []
    for kinds, t, nspin, nedge, nworm in cc.RUNS:
        st, ep, ctr = cl.host_steps(edges, biases, cc.SEED, st, ep, t, cc.betas(nreplicas), nspin, nedge, nworm, kinds=kinds, replica_offset=cc.OFFSET,
                                    flags=cl.CFG_EDGE_IMPORTANCE if importance else 0)
        total = total + ctr
        out.append((st.copy(), total.copy(), ep.copy()))
    return out


@pytest.mark.parametrize("name", cc.PARITY + cc.IMPORTANCE)
def test_host_steps_match_the_restatement(oracle, name):
    """States and counters bit for bit after every run of cc.RUNS (all three kinds drawn, only_basic, each forced kind, the batch
    sizes 1 / 63 / 64 / 65 / 200), betas 0 .. 1000; exp is libm on both sides.  The positive-J cases run with edge importance sampling."""
    imp = name in cc.IMPORTANCE
    want = cc.reference_chain(name, 5, imp)
    got = _host_chain(name, 5, imp)
    for i, ((ws, wc, we), (gs, gc, ge)) in enumerate(zip(want, got)):
        assert np.array_equal(ws, gs), (name, cc.RUNS[i], "states")
        assert np.array_equal(wc, gc), (name, cc.RUNS[i], wc.tolist(), gc.tolist())
        assert np.array_equal(we, ge), (name, cc.RUNS[i], "epochs")
    assert (want[-1][1][:, [CR.C_SPIN, CR.C_EDGE, CR.C_WORM]] > 0).all()  # every kind ran


TRIANGLE = [((0, 1), 1.0), ((1, 2), 1.0), ((2, 0), 1.0)]


def _one_worm(edges, biases, beta, doubles, seed, use_host=True):
    cl = _cl()
    kinds = CR.KINDS_WORM if doubles else CR.KINDS_WORM_NO_DOUBLES
    if use_host:
        st, _, ctr = cl.host_steps(edges, biases, seed, np.zeros(len(biases), dtype=np.uint8), 0, 1, beta, nwormupdates=1, kinds=kinds)
        return st[0], ctr[0]
    g = CR.RefGraphState(edges, biases, seed, 0, state=np.zeros(len(biases), dtype=np.uint8))
    g.do_time_step(beta, nworm=1, kinds=kinds)
    return g.state_bytes(), np.array(g.counters, dtype=np.uint64)


@pytest.mark.parametrize("use_host", [True, False], ids=["host_steps", "restatement"])
def test_worm_known_answers_of_the_reference(oracle, use_host):
    """graph.rs:481-603 for 64 seeds each (the restatement: 8), from the all-false state."""
    chain = [((x, x + 1), 1.0) for x in range(19)]
    bounce = [10.0] + [0.0] * 18 + [10.0]
    for seed in range(64 if use_host else 8):
        assert _one_worm(TRIANGLE, [0.0] * 3, 1.0, False, seed, use_host)[0].all()              # test_worm_flip
        assert _one_worm(TRIANGLE, [-1.0] * 3, 1.0, False, seed, use_host)[0].all()             # test_worm_flip_bias
        assert not _one_worm(TRIANGLE, [1.0] * 3, 1000.0, False, seed, use_host)[0].any()       # test_worm_flip_bias_not
        assert not _one_worm(chain, bounce, 1000.0, False, seed, use_host)[0].any()             # test_worm_flip_bounce
        assert len(set(_one_worm(TRIANGLE, [0.0] * 3, 1.0, True, seed, use_host)[0].tolist())) == 1  # test_worm_flip_doubles
        st, ctr = _one_worm(cc.CASES["lattice4x4"][0], [0.0] * 16, 1000.0, True, seed, use_host)  # test_worm_2d: terminates
        assert set(st.tolist()) <= {0, 1} and ctr[CR.C_WORM] == 1 and ctr[CR.C_WORM_FAIL] <= 1 and ctr[CR.C_WORM_PATH] <= 17


def test_worm_on_the_bathroom_lattice(oracle):
    """test_worm_2d_bathroom (graph.rs:627-647, N = 1024): terminates, leaves every variable 0 / 1, at most one failure per worm; and
    the sequential rule walks as the restatement does (three seeds)."""
    edges = cc.bathroom_unit_cells(16)
    for seed in range(64):
        st, ctr = _one_worm(edges, [0.0] * 1024, 1000.0, True, seed)
        assert set(st.tolist()) <= {0, 1} and ctr[CR.C_WORM] == 1 and ctr[CR.C_WORM_FAIL] <= 1 and 2 <= ctr[CR.C_WORM_PATH] <= 1025
        if seed < 3:
            rs, rc = _one_worm(edges, [0.0] * 1024, 1000.0, True, seed, use_host=False)
            assert np.array_equal(rs, st) and np.array_equal(rc, ctr)


ENUM = [(name, bj) for name in cc.ENUM_SYSTEMS for bj in cc.ENUM_BETAJ]


def test_enumeration_inputs_pass_on_the_restatement_and_catch_wrong_rules(oracle):
    """The statistics test below has sound inputs and power: the restatement alone passes it on every system and temperature, and
    two wrong rules fail it at the same inputs: the bias term's sign reversed, and the omit filter dropped from the edge move."""
    for name, bj in ENUM:
        assert cc.enum_violations(name, bj, cc.enum_reference_states(name, bj)) == [], (name, bj)
    wrong_sign = [v for name, bj in ENUM for v in cc.enum_violations(name, bj, cc.enum_reference_states(name, bj, bias_sign=-1.0))]
    no_omit = [v for name, bj in ENUM for v in cc.enum_violations(name, bj, cc.enum_reference_states(name, bj, edge_omit=False))]
    assert wrong_sign and no_omit, (wrong_sign, no_omit)


@pytest.mark.parametrize("name,betaj", ENUM)
def test_host_steps_sample_the_boltzmann_distribution(oracle, name, betaj):
    """8192 independent replicas, 48 only_basic_moves steps from random states, one sample each: <E>, <m>, <m^2> within 4.5 sigma of
    the enumerated values, sigma = the exact standard deviation / sqrt(R) (nothing measured on the code under test)."""
    cl = _cl()
    edges, biases = cc.ENUM_SYSTEMS[name]
    st = cc.enum_reference_states(name, betaj)  # (only for its shape: the initial states are drawn below)
    init = np.stack([CR.philox_np(cc.SEED, np.arange(len(biases), dtype=np.uint64), 0, np.uint64(r), CR.TAG_INIT)[:, 0] >> np.uint64(31)
                     for r in range(cc.ENUM_R)]).astype(np.uint8)
    assert init.shape == st.shape
    got, ep, _ = cl.host_steps(edges, biases, cc.SEED, init, 0, cc.ENUM_STEPS, cc.enum_beta(name, betaj), only_basic_moves=True)
    assert (ep == cc.ENUM_STEPS).all()
    assert cc.enum_violations(name, betaj, got) == []


def test_plan_places_the_tables():
    cl = _cl()
    import _lattices as lat
    edges = lat.two_d_periodic(64)
    csr = 1 | 2 | 4
    p = cl.plan(edges, [0.0] * 4096)
    assert p["waves"] >= 1 and p["in_lds"] == p["tables"] == (csr | 16) and p["lds_words"] * 4 <= 160 * 1024
    assert p["wave_words"] == 4096 // 32 + 4096 // 4 and p["compact_couplings"] and p["packed_edges"]
    p = cl.plan(edges, [0.25] * 4096)  # with biases everything still fits, with fewer waves if need be
    assert p["in_lds"] == p["tables"] == (csr | 8 | 16) and p["lds_words"] * 4 <= 160 * 1024
    p = cl.plan(edges, [0.0] * 4096, flags=cl.CFG_GLOBAL_TABLES)  # forced
    assert p["in_lds"] == 0 and p["tables"] == (csr | 16) and p["lds_words"] == p["waves"] * p["wave_words"]
    p = cl.plan(edges, [0.0] * 4096, lds_bytes=64 * 1024)  # does not fit: what fits stays, in the order of the carve
    assert p["in_lds"] not in (0, p["tables"]) and p["in_lds"] & 1 and p["lds_words"] * 4 <= 64 * 1024
    big = lat.two_d_periodic(256)
    p = cl.plan(big, [0.0] * 65536)
    assert p["in_lds"] != p["tables"] and p["lds_words"] * 4 <= 160 * 1024 and p["waves"] * p["wave_words"] <= p["lds_words"]
    n = 200000  # the state bits and stamps of one replica: 25000 + 200000 bytes
    with pytest.raises(cl.IsingMcError) as ei:
        cl.plan([((i, i + 1), 1.0) for i in range(n - 1)], [0.0] * n)
    assert ei.value.code == -5 and "exceed LDS" in str(ei.value) and "at most 145632 variables in 163840 bytes" in str(ei.value)
    assert (145632 + 31) // 32 + (145632 + 3) // 4 <= 40960 < (145633 + 31) // 32 + (145633 + 3) // 4


def _flags(c):
    return _cl().CFG_EDGE_IMPORTANCE if c["importance"] else 0


@pytest.mark.parametrize("name", list(cc.LAYOUT_CASES))
def test_layout_cases_plan_as_their_table_says(name):
    """The launch of every layout case at 160 KB of LDS is the one tests/test_gpu_classical_layouts.py means to run: waves, tables in
    LDS, table formats.  A change of the carve that moves a case to another launch fails here, without a device."""
    c = cc.LAYOUT_CASES[name]
    p = _cl().plan(c["edges"], c["biases"], flags=_flags(c))
    assert {k: p[k] for k in c["plan"]} == c["plan"], (name, p)
    assert p["lds_words"] <= 40960 and p["wave_words"] * p["waves"] <= p["lds_words"]


def test_one_variable_more_than_the_largest_is_refused():
    cl = _cl()
    assert len(cc.LAYOUT_CASES["hightail145632"]["biases"]) == cc.LAYOUT_MAX_VARS
    with pytest.raises(cl.IsingMcError) as ei:
        cl.plan(*cc.hightail(cc.LAYOUT_MAX_VARS + 1))
    assert ei.value.code == -5 and "at most 145632 variables" in str(ei.value)


def _host_layout_chain(name):
    cl = _cl()
    c = cc.layout_case(name)
    st, ep = cc.layout_states(len(c["biases"])), np.zeros(cc.LAYOUT_R, dtype=np.uint64)
    total = np.zeros((cc.LAYOUT_R, 8), dtype=np.uint64)
    out = []
    for kinds, t, nspin, nedge, nworm in cc.LAYOUT_RUNS:
        st, ep, ctr = cl.host_steps(c["edges"], c["biases"], cc.SEED, st, ep, t, c["betas"], nspin, nedge, nworm, kinds=kinds, replica_offset=cc.OFFSET,
                                    flags=_flags(c))
        total = total + ctr
        out.append((st.copy(), total.copy(), ep.copy()))
    return out


@pytest.mark.parametrize("name", list(cc.LAYOUT_CASES) + list(cc.RANDOM_CASES))
def test_host_steps_match_the_restatement_on_the_layout_cases(oracle, name):
    """The sequential rule over both coupling formats and both edge-list formats of build_tables, and over random multigraphs around
    the word boundaries of the state: states, counters and epochs bit for bit after every run of cc.LAYOUT_RUNS, beta up to +inf."""
    want, got = cc.layout_reference_chain(name), _host_layout_chain(name)
    for i, ((ws, wc, we), (gs, gc, ge)) in enumerate(zip(want, got)):
        assert np.array_equal(ws, gs), (name, cc.LAYOUT_RUNS[i], "states")
        assert np.array_equal(wc, gc), (name, cc.LAYOUT_RUNS[i], wc.tolist(), gc.tolist())
        assert np.array_equal(we, ge), (name, cc.LAYOUT_RUNS[i], "epochs")


def _final_states_of(name, edges):
    c = cc.LAYOUT_CASES[name]
    return cc.run_reference(edges, c["biases"], cc.layout_states(len(c["biases"])), c["betas"], cc.LAYOUT_RUNS, c["importance"])[0][-1][0]


@pytest.mark.parametrize("name", cc.LAYOUT_NONCOMPACT)
def test_noncompact_inputs_tell_a_wrong_coupling_index(oracle, name):
    """A condition on the restatement alone: with every coupling moved on by one edge the final states are different ones, so a kernel
    that reads jv one entry off cannot pass the parity test of this case."""
    c = cc.LAYOUT_CASES[name]
    assert not np.array_equal(cc.layout_reference_chain(name)[-1][0], _final_states_of(name, cc.rotate_couplings(c["edges"])))


@pytest.mark.parametrize("name", cc.LAYOUT_HIGHTAIL)
def test_hightail_inputs_tell_truncated_endpoints(oracle, name):
    """Conditions on the restatement alone: the final states differ from those of the graph with its endpoints cut to 16 bits, and a
    variable with index >= 65536 has changed, so the two-word edge list and the state words beyond 2048 matter to the parity test."""
    c = cc.LAYOUT_CASES[name]
    final = cc.layout_reference_chain(name)[-1][0]
    assert not np.array_equal(final, _final_states_of(name, cc.truncate_endpoints(c["edges"])))
    assert (final[:, 65536:] != cc.layout_states(len(c["biases"]))[:, 65536:]).any()


@pytest.mark.parametrize("start", cc.EPOCH_STARTS)
def test_host_steps_at_epochs_beyond_32_bits(oracle, start):
    """epoch_hi24 of the Philox counter: four steps across 2^32 and across 2^56."""
    cl = _cl()
    edges, biases = cc.CASES["ring33"]
    st = np.stack([CR.random_state(cc.SEED, cc.OFFSET + r, 33) for r in range(5)])
    st, ep, ctr = cl.host_steps(edges, biases, cc.SEED, st, start, 4, cc.betas(5), kinds=CR.KINDS_ALL, replica_offset=cc.OFFSET)
    ws, wc, we = cc.epoch_reference(start)
    assert np.array_equal(st, ws) and np.array_equal(ctr, wc) and np.array_equal(ep, we) and (ep == np.uint64(start + 4)).all()
    assert not np.array_equal(ws, cc.reference_chain("ring33", 5, runs=((CR.KINDS_ALL, 4, None, None, None),))[0][0])  # epoch 0 gives other states


def test_config_struct_and_null_handles(tmp_path):
    import isingmontecarlo_amd as im
    lib = im.load_library()
    src = tmp_path / "abi.c"
    src.write_text('#include "isingmc_hip.h"\n#include <stdio.h>\nint main(void){ printf("%zu\\n", sizeof(isingmc_classical_config)); return 0; }\n')
    exe = str(tmp_path / "abi")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert int(subprocess.check_output([exe], text=True)) == C.sizeof(im._ClassicalConfig) == 72
    assert lib.isingmc_classical_timesteps(None, 1, None, 1, 1, 1, 0) == -1
    for fn in (lib.isingmc_classical_get_epoch, lib.isingmc_classical_set_epoch, lib.isingmc_classical_energies, lib.isingmc_classical_counters):
        assert fn(None, None) == -1
    assert lib.isingmc_classical_get_state(None, 0, None) == -1 and lib.isingmc_classical_set_state(None, 0, None) == -1
    assert lib.isingmc_classical_set_stream(None, None) == -1 and lib.isingmc_classical_synchronize(None) == -1
    assert lib.isingmc_classical_last_kernel_ms(None, None) == -1 and lib.isingmc_classical_launch_plan(None, None) == -1
    assert lib.isingmc_classical_plan(None, 1024, None) == -1 and lib.isingmc_classical_host_steps(None, 1, None, 1, 1, 1, 0, None, None, None) == -1
    lib.isingmc_classical_destroy(None)
    assert lib.isingmc_classical_create(None, None) == -1


def test_config_errors_need_no_device():
    cl = _cl()
    ok = [((0, 1), 1.0), ((1, 2), 0.5)]
    assert cl.plan(ok, [0.0] * 3)["waves"] == 4
    for edges, biases, flags, words in [
        ([((0, 1), 1.0), ((1, 1), 1.0)], [0.0] * 3, 0, "self-loop"),
        ([((0, 3), 1.0)], [0.0] * 3, 0, "out of range"),
        ([], [0.0] * 3, 0, "at least one edge"),
        ([((0, 1), 1.0), ((1, 2), -0.5)], [0.0] * 3, cl.CFG_EDGE_IMPORTANCE, "every J > 0"),
        ([((0, 1), 1.0), ((1, 2), 0.0)], [0.0] * 3, cl.CFG_EDGE_IMPORTANCE, "every J > 0"),
        (ok, [0.0] * 3, 64, "unknown flag"),
    ]:
        with pytest.raises(cl.IsingMcError) as ei:
            cl.plan(edges, biases, flags=flags)
        assert ei.value.code == -1 and words in str(ei.value), (words, str(ei.value))
        with pytest.raises(cl.IsingMcError) as ei:
            cl.host_steps(edges, biases, 1, np.zeros((1, 3), dtype=np.uint8), 0, 1, 1.0, flags=flags)
        assert ei.value.code == -1 and words in str(ei.value)
    with pytest.raises(cl.IsingMcError):
        cl.host_steps(ok, [0.0] * 3, 1, np.zeros((1, 3), dtype=np.uint8), 0, 1, 1.0, kinds=6)


def test_no_device_is_a_loud_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import isingmontecarlo_amd as im
    with pytest.raises(im.IsingMcError) as ei:
        im.GraphState([((0, 1), 1.0)], [0.0, 0.0], 1)
    assert ei.value.code == -2 and "no CPU fallback" in str(ei.value)


def test_new_from_graph_refuses_biases():
    """qmc_ising.rs:157, checked before anything is built."""
    import isingmontecarlo_amd as im

    class Biased:  # what new_from_graph asks of a classical graph
        biases = np.array([0.0, 0.5])
        nreplicas, nvars = 1, 2
    with pytest.raises(AssertionError):
        im.QmcIsingGraph.new_from_graph(Biased(), 1.0, 0.0, 4, 1)
    with pytest.raises(AssertionError):
        im.new_qmc_from_graph(Biased(), 1.0, 0.0, 4, 1)
