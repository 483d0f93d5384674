"""Classical parallel tempering without a device: isingmc_classical_host_pt_run (csrc/classical_pt_rule.h by the sequential rule)
against the numpy restatement of a round (tests/_classical_pt_cases.py), against exact enumeration, and its argument checks."""
import os
import subprocess

import numpy as np
import pytest

import _classical_cases as cc
import _classical_pt_cases as pc
import _classical_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


def test_rule_header_is_plain_cpp(tmp_path):
    """classical_pt_rule.h compiles on its own under g++ -Wall -Wextra -Werror: no HIP header, no device code."""
    src = tmp_path / "rule.cpp"
    src.write_text('#include "classical_pt_rule.h"\nint main() { return cmc_pt_accept(1.0, 2.0, -1.0, 1.0, 0.5) ? 0 : 1; }\n')
    exe = str(tmp_path / "rule")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "isingmontecarlo_amd", "csrc"), str(src), "-o", exe])
    assert subprocess.call([exe]) == 0  # (beta_t - beta_t1) (e_t - e_t1) = 2 >= 0: accepted


@pytest.mark.parametrize("name", list(pc.PT_CASES))
def test_host_run_matches_the_restatement(oracle, name):
    """Every output bit for bit on every GPU parity case, 6 rounds of 2 KINDS_ALL steps: states, epochs, temp_of, move counters, swap
    counts, pt_step and both series.  exp is libm's in the host entry and numpy's in the restatement's swap test (see
    tests/test_gpu_classical.py on why the comparison is exact all the same)."""
    c = pc.PT_CASES[name]
    want = pc.host_parity_reference(name)
    ref = pc.TemperingRef(c["edges"], c["biases"], cc.SEED, c["betas"], c["chains"], pc.pt_offset(name), basic=False)
    energy, mag = ref.run(pc.PT_ROUNDS, pc.PT_STEPS)
    assert np.array_equal(ref.states(), want["states"]) and np.array_equal(ref.epochs(), want["epochs"])
    assert np.array_equal(ref.temp_of.reshape(-1), want["temp_of"]) and ref.pt_step == want["pt_step"] == pc.PT_ROUNDS
    assert np.array_equal(ref.counters(), want["counters"])
    assert np.array_equal(ref.attempts, want["attempts"]) and np.array_equal(ref.accepts, want["accepts"])
    assert np.array_equal(energy, want["energy"]) and np.array_equal(mag, want["magnetization"])
    assert want["counters"][:, CR.C_WORM].sum() > 0 and want["accepts"].sum() > 0 and want["attempts"].sum() > want["accepts"].sum()
    # each pair is attempted once a round
    assert (want["attempts"] == pc.PT_ROUNDS).all()


def test_host_energy_series_is_get_energy_of_the_states(oracle):
    """On a dyadic case every order of additions gives the same sum: the series equals the restatement's get_energy of the states
    round by round (steps = 1, one call per round), and the magnetisation is the sum of the spins."""
    cl = _cl()
    edges, biases = cc.CASES["k8"]
    betas, chains = [0.2, 0.6, 1.0], 2
    st, ep, tof, step = pc.initial_states(cc.SEED, 6, 8), 0, None, 0
    for _ in range(4):
        out = cl.host_tempering_run(edges, biases, cc.SEED, st, ep, betas, 1, 1, kinds=cl.KINDS_ALL, temp_of=tof, pt_step=step)
        before = tof if tof is not None else np.arange(6) % 3  # the series is laid out by the temperatures before the round's swaps
        st, ep, tof, step = out["states"], out["epochs"], out["temp_of"], out["pt_step"]
        for r in range(6):
            assert out["energy"][0, r // 3, before[r]] == CR.get_energy(edges, biases, st[r])
            assert out["magnetization"][0, r // 3, before[r]] == 2 * int(st[r].sum()) - 8
    assert step == 4


def test_calls_compose_and_chains_shard(oracle):
    """10 rounds = 3 + 7 with everything carried over; 4 chains = two batches of 2 chains at replica offsets 0 and 2 T; without the
    series the states are the same."""
    cl = _cl()
    edges, biases = cc.CASES["ring33"]
    betas = [0.2, 0.5, 1.0, 2.0]
    whole = pc.host_run(cl, edges, biases, betas, 4, 10, 2, kinds=cl.KINDS_ALL)
    a = pc.host_run(cl, edges, biases, betas, 4, 3, 2, kinds=cl.KINDS_ALL)
    b = cl.host_tempering_run(edges, biases, cc.SEED, a["states"], a["epochs"], betas, 7, 2, kinds=cl.KINDS_ALL, temp_of=a["temp_of"], pt_step=a["pt_step"])
    for k in ("states", "epochs", "temp_of", "pt_step"):
        assert np.array_equal(whole[k], b[k]), k
    for k in ("counters", "attempts", "accepts"):
        assert np.array_equal(whole[k], a[k] + b[k]), k
    assert np.array_equal(whole["energy"], np.concatenate([a["energy"], b["energy"]]))
    lo = pc.host_run(cl, edges, biases, betas, 2, 10, 2, replica_offset=0, kinds=cl.KINDS_ALL)
    hi = pc.host_run(cl, edges, biases, betas, 2, 10, 2, replica_offset=8, kinds=cl.KINDS_ALL)
    for k in ("states", "temp_of", "counters", "attempts", "accepts"):
        assert np.array_equal(whole[k], np.concatenate([lo[k], hi[k]])), k
    assert np.array_equal(whole["magnetization"], np.concatenate([lo["magnetization"], hi["magnetization"]], axis=1))
    quiet = pc.host_run(cl, edges, biases, betas, 4, 10, 2, kinds=cl.KINDS_ALL, record=False)
    assert "energy" not in quiet and np.array_equal(quiet["states"], whole["states"]) and np.array_equal(quiet["temp_of"], whole["temp_of"])
    swaps_only = pc.host_run(cl, edges, biases, betas, 4, 5, 0, kinds=cl.KINDS_ALL)  # steps = 0: the states stay, the labels move
    assert np.array_equal(swaps_only["states"], pc.initial_states(cc.SEED, 16, 33)) and (swaps_only["epochs"] == 0).all()
    assert swaps_only["accepts"].sum() > 0 and np.array_equal(np.sort(swaps_only["energy"][4], axis=1), np.sort(swaps_only["energy"][0], axis=1))
    none = pc.host_run(cl, edges, biases, betas, 4, 0, 2, kinds=cl.KINDS_ALL)  # rounds = 0: nothing happens
    assert none["pt_step"] == 0 and (none["epochs"] == 0).all() and none["energy"].shape == (0, 4, 4)


def _by_temperature(out, ntemps, nvars):
    slot_at = np.argsort(out["temp_of"].reshape(-1, ntemps), axis=1)
    return np.take_along_axis(out["states"].reshape(-1, ntemps, nvars), slot_at[:, :, None], axis=1)


@pytest.mark.parametrize("name", list(cc.ENUM_SYSTEMS))
def test_host_run_samples_the_boltzmann_distribution_at_every_temperature(oracle, name):
    """2048 chains of the ladder beta |J| = 0.2 .. 1.0 (T = 4), R = 8192, 48 rounds of one only_basic_moves step from random states.
    The states at every temperature give <E>, <m>, <m^2> within 4.5 sigma of the enumerated values, sigma = the exact standard
    deviation / sqrt(2048).  The mean of the recorded E series over the rounds from 24 on is held to the same 4.5 sigma at its own
    sample count, 24 * 2048 per temperature (successive rounds are correlated, so this is the stricter reading).  24 rounds are
    skipped: the batch tests of tests/test_classical_cpu.py call 48 steps equilibrated, and from random states the series mean over
    all 48 rounds is off by up to 38 sigma at the coldest temperature, by at most 3.8 from round 8 on and 2.4 from round 16 on;
    measured here at skip 24: at most 1.8 sigma over the three systems and four temperatures."""
    cl = _cl()
    edges, biases = cc.ENUM_SYSTEMS[name]
    out = pc.host_run(cl, edges, biases, pc.enum_pt_betas(name), pc.ENUM_PT_CHAINS, pc.ENUM_PT_ROUNDS, 1, only_basic_moves=True)
    assert len(out["states"]) == cc.ENUM_R and (out["epochs"] == pc.ENUM_PT_ROUNDS).all() and pc.ENUM_PT_SKIP == 24
    assert pc.enum_pt_violations(name, _by_temperature(out, 4, len(biases))) == []
    sigmas = pc.enum_pt_series_sigmas(name, out["energy"])
    assert max(sigmas) <= cc.ENUM_SIGMAS, sigmas
    rate = out["accepts"].sum(axis=0) / out["attempts"].sum(axis=0)
    assert (rate > 0.3).all() and (rate < 1.0).all(), rate  # the swaps do happen


def _worst_sigmas(name, by_temperature):
    """the largest miss of <E>, <m>, <m^2> in sigmas, per temperature"""
    edges, biases = cc.ENUM_SYSTEMS[name]
    out = []
    for t, bj in enumerate(pc.ENUM_PT_BETAJ):
        exact = CR.exact_moments(edges, biases, cc.enum_beta(name, bj))
        got = CR.sample_moments(edges, biases, by_temperature[:, t, :])
        out.append(max(float(abs(got[o].mean() - m) / (sd / np.sqrt(len(by_temperature)))) for o, (m, sd) in exact.items()))
    return out


def test_enumeration_inputs_catch_wrong_swap_rules(oracle):
    """The statistics test has power: on the restatement alone, at the inputs of the test above for frustrated2x4, the right rule
    passes and gives the host entry's states, and three wrong rules are seen in the states at some temperature.  Observed sigmas
    per temperature (states: the worst of E, m, m^2; series: the E series from round 24 on):
      right     states  1.1  1.1  2.0  0.9    series  1.2  0.7   1.0   1.1
      always    states 38.5  5.9 36.4 66.5    series 35.2  1.5 104.0 231.4   (every swap accepted)
      reversed  states 50.1  5.9 47.4 94.5    series 45.9  4.7 135.2 323.1   (the exponent's sign reversed)
      position  states  2.1  1.1  4.1  5.6    series  2.7  3.7  10.1  21.5   (energies by temperature position, not by slot, in
                                                                              the second phase)
    On ring9_biased and k5_random the position rule shows in the series only (19.0 and 11.3 sigma against 3.8 and 4.4 in the states)."""
    cl = _cl()
    name = "frustrated2x4"
    edges, biases = cc.ENUM_SYSTEMS[name]
    seen = {}
    for rule in pc.RULES:
        ref = pc.TemperingRef(edges, biases, cc.SEED, pc.enum_pt_betas(name), pc.ENUM_PT_CHAINS, basic=True, rule=rule)
        energy, _ = ref.run(pc.ENUM_PT_ROUNDS, 1)
        seen[rule] = (_worst_sigmas(name, ref.states_by_temperature()), pc.enum_pt_series_sigmas(name, energy))
        if rule == "right":
            host = pc.host_run(cl, edges, biases, pc.enum_pt_betas(name), pc.ENUM_PT_CHAINS, pc.ENUM_PT_ROUNDS, 1, only_basic_moves=True)
            assert np.array_equal(ref.states(), host["states"]) and np.array_equal(ref.temp_of.reshape(-1), host["temp_of"])
            assert np.array_equal(energy, host["energy"]) and np.array_equal(ref.accepts, host["accepts"])
    assert max(seen["right"][0]) <= cc.ENUM_SIGMAS and max(seen["right"][1]) <= cc.ENUM_SIGMAS, seen["right"]
    for rule in pc.RULES[1:]:
        assert max(seen[rule][0]) > cc.ENUM_SIGMAS and max(seen[rule][1]) > cc.ENUM_SIGMAS, (rule, seen[rule])


def test_argument_errors_need_no_device():
    """Every ISINGMC_EINVAL of attach, through the host entry that shares its check."""
    cl = _cl()
    edges, biases = cc.CASES["triangle"]
    ok = dict(edges=edges, biases=biases, seed=1, states=np.zeros((6, 3), dtype=np.uint8), epochs=0, betas=[0.5, 1.0, 2.0], rounds=1, steps=1)
    assert cl.host_tempering_run(**ok)["pt_step"] == 1
    for change, words in [
        (dict(betas=[1.0]), "ntemps >= 2"),
        (dict(betas=[]), "ntemps >= 2"),
        (dict(betas=[0.5, 1.0, 2.0, 3.0]), "multiple of ntemps"),
        (dict(replica_offset=4), "replica_offset must be a multiple"),
        (dict(betas=[0.5, float("inf"), 2.0]), "finite"),
        (dict(betas=[0.5, float("nan"), 2.0]), "finite"),
        (dict(betas=None), "ntemps >= 2"),
        (dict(temp_of=[0, 1, 1, 0, 1, 2]), "permutation"),
        (dict(temp_of=[0, 1, 3, 0, 1, 2]), "permutation"),
        (dict(kinds=6), "kinds"),
        (dict(edges=[((0, 0), 1.0)]), "self-loop"),
    ]:
        with pytest.raises(cl.IsingMcError) as ei:
            cl.host_tempering_run(**{**ok, **change})
        assert ei.value.code == -1 and words in str(ei.value), (change, str(ei.value))
    # a null ladder with a plausible ntemps: straight through the C ABI
    import ctypes as C
    import isingmontecarlo_amd as im
    lib = im.load_library()
    ed, js, hs = cl._model(edges, biases)
    cfg = cl._config(ed, js, hs, 1, 6)
    st, ep, tof, step = np.zeros((6, 3), dtype=np.uint8), np.zeros(6, dtype=np.uint64), np.arange(6, dtype=np.uint32) % 3, C.c_uint64(0)
    args = [1, 1, cl.NONE, cl.NONE, cl.NONE, 0, im._ptr(st, C.c_uint8), im._ptr(ep, C.c_uint64), im._ptr(tof, C.c_uint32), C.byref(step), None, None, None, None, None]
    assert lib.isingmc_classical_host_pt_run(C.byref(cfg), 3, None, *args) == -1
    assert b"non-null" in lib.isingmc_classical_last_error(None)
    ladder = np.array([0.5, 1.0, 2.0])
    assert lib.isingmc_classical_host_pt_run(C.byref(cfg), 3, im._ptr(ladder, C.c_double), *args) == 0 and step.value == 1
    for fn, nargs in ((lib.isingmc_classical_pt_attach, 2), (lib.isingmc_classical_pt_get, 2), (lib.isingmc_classical_pt_swap_counts, 2),
                      (lib.isingmc_classical_pt_set_swap_counts, 2)):
        assert fn(None, *([0, None] if fn is lib.isingmc_classical_pt_attach else [None] * nargs)) == -1
    assert lib.isingmc_classical_pt_set(None, None, 0) == -1 and lib.isingmc_classical_pt_run(None, 1, 1, 1, 1, 1, 0, None, None) == -1
