"""GPU tests of the sample record (isingmc_record_*): the recorded rows against the oracle's trajectory on every path through
isingmc_timesteps, the bit-series kernel against numpy on the recorded states, and the autocorrelation kernel bit for bit against
its host restatement (autocorrelations.bit_autocorrelation) and to 1e-10 against the float paths."""
import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import CASES, RVB_CASES, make_pair, assert_same

pytestmark = pytest.mark.gpu

T_STEPS = 64
FREQS = [1, 2, 5]
MODELS = {c[0]: c for c in CASES if c[0] in ("ring8_afm", "villain4", "ferro6_long", "ring5_randmag", "ferro8x8")}
RVB_MODELS = {c[0]: c for c in RVB_CASES if c[0] in ("villain4", "ferro8x8_long")}
assert len(MODELS) == 5 and len(RVB_MODELS) == 2
# mode -> (update flags, config flags, steps per launch or None, hand the batch to Qmc with loop updates)
MODES = {
    "default": (0, 0, None, False),
    "heatbath": (4, 0, None, False),
    "qmc_loop": (1, 0, None, True),
    "fused_spl0": (0, 2, 0, False),
    "fused_spl1": (0, 2, 1, False),
    "fused_spl7": (0, 2, 7, False),
}
RVB_MODES = {
    "rvb": (8, 0, None, False),
    "rvb_global_tables": (8, 4096, None, False),
}
T_VALUES = [1, 31, 32, 33, 64, 77, 200]
FIRSTS = [0, 5]


def record_parity(oracle, edges, gamma, h, beta, cutoff, cap, seed, R, t, freq, flags, cfg, spl, qmc, what, expect_lean=None):
    """Row k of the record = the oracle replica's state after (k + 1) * freq steps; afterwards the batch equals the oracle and its
    accumulators equal those of a twin batch that ran the same call without a record."""
    g, m, reps = make_pair(oracle, edges, gamma, h, cutoff, cap, seed, R, cfg_flags=cfg)
    twin, _, _ = make_pair(oracle, edges, gamma, h, cutoff, cap, seed, R, cfg_flags=cfg)
    if qmc:
        g, twin = g.into_qmc(True), twin.into_qmc(True)
        assert g._flags == flags
    if spl is not None:
        g.set_steps_per_launch(spl)
        twin.set_steps_per_launch(spl)
    nsamp = t // freq
    g.attach_sample_record(nsamp)
    assert g.record_count() == 0 and g.record_capacity() == nsamp
    g.run(t, beta, sampling_freq=freq, flags=flags)
    twin.run(t, beta, sampling_freq=freq, flags=flags)
    assert g.record_count() == nsamp
    rows = g.record_states()
    assert rows.shape == (nsamp, R, g.nvars) and rows.dtype == np.uint8
    for k in range(nsamp):
        for r, rep in enumerate(reps):
            rep.timesteps(freq, beta, freq, flags)
            assert np.array_equal(rows[k, r], rep.state()), f"{what}: row {k} of replica {r} differs from the oracle after {(k + 1) * freq} steps"
    for rep in reps:
        if t - nsamp * freq:
            rep.timesteps(t - nsamp * freq, beta, freq, flags)
    for r in range(R):
        assert np.array_equal(g.record_states(r=r), rows[:, r]), f"{what}: per-replica read differs r={r}"
    if expect_lean is not None:
        assert g.launch_info()["lean_cluster"] == expect_lean, g.launch_info()
    assert_same(g, reps, what)
    assert_same(twin, reps, what + " (twin without a record)")
    assert np.array_equal(g.accumulators(), twin.accumulators()), f"{what}: attaching a record changed the accumulators"
    assert g.verify().all()
    g.close(); twin.close()


@pytest.mark.parametrize("freq", FREQS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(MODELS))
def test_record_rows_match_the_oracle(oracle, name, mode, freq):
    _, edges, gamma, h, beta = MODELS[name]
    flags, cfg, spl, qmc = MODES[mode]
    record_parity(oracle, edges, gamma, h, beta, 8, 8192, 99, 3, T_STEPS, freq, flags, cfg, spl, qmc, f"{name} {mode} freq={freq}")


@pytest.mark.parametrize("freq", FREQS)
@pytest.mark.parametrize("mode", list(RVB_MODES))
@pytest.mark.parametrize("name", list(RVB_MODELS))
def test_record_rows_match_the_oracle_with_rvb(oracle, name, mode, freq):
    _, edges, gamma, h, beta, cutoff = RVB_MODELS[name]
    flags, cfg, spl, qmc = RVB_MODES[mode]
    record_parity(oracle, edges, gamma, h, beta, cutoff, 8192, 1357, 3, T_STEPS, freq, flags, cfg, spl, qmc, f"{name} {mode} freq={freq}")


@pytest.mark.parametrize("freq", FREQS)
@pytest.mark.parametrize("name", list(RVB_MODELS))
def test_record_rows_match_the_oracle_with_rvb_tables_in_hbm_inside_fused_launches(oracle, name, freq):
    """CFG_FUSED_LAUNCH around an RVB sweep that needs a launch of its own: the third loop of run()."""
    _, edges, gamma, h, beta, cutoff = RVB_MODELS[name]
    record_parity(oracle, edges, gamma, h, beta, cutoff, 8192, 1357, 3, T_STEPS, freq, 8, 4096 | 2, None, False, f"{name} rvb_g fused freq={freq}")


@pytest.mark.parametrize("freq", FREQS)
def test_record_rows_match_the_oracle_behind_the_lean_cluster_kernel(oracle, freq):
    """32x32 ferromagnet at beta = 2: the dedicated cluster kernel with deferred flips (asserted), whose op-strings in HBM wait for
    the next diagonal launch while the state the record copies is already current."""
    record_parity(oracle, lat.two_d_ferro(32), 1.0, 0.0, 2.0, 1024, 1 << 15, 4711, 3, T_STEPS, freq, 0, 0, None, False, f"ferro32 lean freq={freq}",
                  expect_lean=True)


def test_record_appends_clears_and_refuses_calls_that_do_not_fit(oracle):
    import isingmontecarlo_amd as im
    _, edges, gamma, h, beta = MODELS["villain4"]
    R = 3
    g, m, reps = make_pair(oracle, edges, gamma, h, 8, 8192, 31, R)
    assert g.record_count() == 0 and g.record_capacity() == 0
    with pytest.raises(im.IsingMcError) as ei:
        g.record_states(0, 1)
    assert ei.value.code == -1
    g.attach_sample_record(10)
    g.run(8, beta, sampling_freq=2)
    first = g.record_states()
    assert g.record_count() == 4 and first.shape == (4, R, g.nvars)
    g.run(6, beta, sampling_freq=2)
    assert g.record_count() == 7
    both = g.record_states()
    assert np.array_equal(both[:4], first)
    assert np.array_equal(both[6], g.state_ref())
    assert np.array_equal(g.record_states(4, 3), both[4:])
    # a call that does not fit: ECAPACITY before anything runs
    before = (g.get_epoch().copy(), g.get_n().copy(), g.state_ref().copy(), [g.export_ops(r) for r in range(R)])
    with pytest.raises(im.IsingMcError) as ei:
        g.run(8, beta, sampling_freq=2)  # 4 samples, room for 3
    assert ei.value.code == -3
    assert g.record_count() == 7
    assert np.array_equal(g.get_epoch(), before[0]) and np.array_equal(g.get_n(), before[1]) and np.array_equal(g.state_ref(), before[2])
    assert all(np.array_equal(g.export_ops(r), before[3][r]) for r in range(R))
    assert np.array_equal(g.record_states(), both)
    g.run(7, beta, sampling_freq=2)  # 3 samples: fits exactly
    assert g.record_count() == 10
    for rep in reps:
        rep.timesteps(8, beta, 2, 0); rep.timesteps(6, beta, 2, 0); rep.timesteps(7, beta, 2, 0)
    assert_same(g, reps, "after the refused call")
    g.record_clear()
    assert g.record_count() == 0 and g.record_capacity() == 10
    g.run(2, beta)
    assert g.record_count() == 2 and np.array_equal(g.record_states()[1], g.state_ref())
    with pytest.raises(im.IsingMcError):
        g.record_states(1, 2)  # beyond the rows written
    g.detach_sample_record()
    assert g.record_capacity() == 0
    g.run(3, beta)  # nothing attached, nothing recorded
    assert g.record_count() == 0


def recorded_batch(oracle, nsamples=205):
    """6x6 frustrated lattice (N = 36: the last state word is partial; couplings of both signs), R = 3, `nsamples` recorded sweeps."""
    edges = lat.two_d_periodic(6)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 36, 1 << 13, 2024, 3)
    assert g.nvars == 36
    g.attach_sample_record(nsamples)
    g.run(nsamples, 1.0)
    return g, g.record_states()


def observables(g):
    """name -> (groups, flips): the reference's three kinds of observables."""
    from isingmontecarlo_amd.autocorrelations import variable_groups, product_groups, bond_groups
    prods = [(0, 1), (2, 3, 4), (35,), (1, 6, 7, 15), (0, 31, 32, 33, 35), tuple(range(36))]
    return {"variables": variable_groups(g.nvars), "products": product_groups(prods), "bonds": bond_groups(g)}


def observe(states, groups, flips):
    """[T][n] of 0/1 from [T][N] states: parity of each group's bits ^ flip"""
    return np.stack([(states[:, list(vs)].sum(axis=1) + int(f)) & 1 for vs, f in zip(groups, flips)], axis=1).astype(np.uint8)


def test_record_series_equals_numpy_parities(oracle):
    g, states = recorded_batch(oracle)
    for what, (groups, flips) in observables(g).items():
        for first in FIRSTS:
            for T in T_VALUES:
                got = g.record_series(groups, flips, first, T)
                Tw = (T + 31) // 32
                assert got.shape == (3, len(groups), Tw) and got.dtype == np.uint32
                for r in range(3):
                    bits = observe(states[first:first + T, r], groups, flips)  # [T][n]
                    padded = np.zeros((Tw * 32, len(groups)), dtype=np.uint64)
                    padded[:T] = bits
                    want = (padded.reshape(Tw, 32, -1) << np.arange(32, dtype=np.uint64)[None, :, None]).sum(axis=1).astype(np.uint32).T
                    assert np.array_equal(got[r], want), f"{what} first={first} T={T} r={r}"  # (padding bits included: they are 0 in `want`)
        # without flips: the same series with the flipped observables inverted in their 77 valid bits
        valid = np.array([0xFFFFFFFF, 0xFFFFFFFF, (1 << 13) - 1], dtype=np.uint32)
        delta = g.record_series(groups, None, 0, 77) ^ g.record_series(groups, flips, 0, 77)
        assert np.array_equal(delta, np.broadcast_to(np.where(np.asarray(flips)[:, None] != 0, valid[None, :], 0), delta.shape)), what


def test_record_autocorrelation_equals_its_host_restatement_bit_for_bit(oracle):
    from isingmontecarlo_amd.autocorrelations import bit_autocorrelation
    g, states = recorded_batch(oracle)
    for what, (groups, flips) in observables(g).items():
        for first in FIRSTS:
            for T in T_VALUES:
                got = g.record_autocorrelation(groups, first, T)
                assert got.shape == (3, T) and got.dtype == np.float64
                assert np.array_equal(got, g.record_autocorrelation(groups, first, T)), f"{what}: two calls differ"
                for r in range(3):
                    want = bit_autocorrelation(observe(states[first:first + T, r], groups, flips))
                    diff = np.abs(got[r] - want).max()
                    print(f"record_autocorrelation vs bit_autocorrelation {what} first={first} T={T} r={r}: max diff {diff}")
                    assert np.array_equal(got[r], want), f"{what} first={first} T={T} r={r}: max diff {diff}"


def test_record_autocorrelation_against_the_float_paths(oracle):
    """The construction of test_variable_autocorrelation_values: the direct O(T^2) sum over the states the ORACLE samples on the same
    trajectory; then device="record" against the host FFT path on twin batches, for variables, products and bonds."""
    from isingmontecarlo_amd.autocorrelations import (variable_autocorrelation, spin_product_autocorrelation, bond_autocorrelation,
                                                     direct_autocorrelation, variable_groups)
    edges = lat.two_d_ferro(4)
    R, T, freq = 3, 48, 2
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 16, 1 << 11, 77, R)
    g.attach_sample_record(T)
    g.run(T * freq, 1.5, sampling_freq=freq)
    ac = g.record_autocorrelation(variable_groups(g.nvars)[0])
    samples = [[] for _ in range(R)]
    for _ in range(T):
        oracle.batch_timesteps(reps, freq, [1.5] * R)
        for k, rep in enumerate(reps):
            samples[k].append(rep.state().astype(np.float64) * 2.0 - 1.0)
    assert_same(g, reps, "after recording")
    for k in range(R):
        want = direct_autocorrelation(np.stack(samples[k]))
        err = np.abs(ac[k] - want).max()
        print("record vs direct over the oracle's samples", k, err)
        assert ac[k].shape == want.shape and err < 1e-10
    mixed = lat.two_d_periodic(4)
    prods = [(0, 1), (2, 3, 4), (5, 9, 10, 15)]
    for what, fn in (("variables", lambda gr, dev: variable_autocorrelation(gr, T * freq, 1.5, sampling_freq=freq, device=dev)),
                     ("products", lambda gr, dev: spin_product_autocorrelation(gr, T * freq, 1.5, prods, sampling_freq=freq, device=dev)),
                     ("bonds", lambda gr, dev: bond_autocorrelation(gr, T * freq, 1.5, sampling_freq=freq, device=dev))):
        a, _, _ = make_pair(oracle, mixed, 1.0, 0.0, 16, 1 << 11, 78, R)
        b, _, _ = make_pair(oracle, mixed, 1.0, 0.0, 16, 1 << 11, 78, R)
        got, want = fn(a, "record"), fn(b, None)
        err = np.abs(got - want).max()
        print("device=record vs host", what, err)
        assert got.shape == want.shape == (R, T) and err < 1e-10
        assert a.record_capacity() == 0  # the record of the call is gone
        assert np.array_equal(a.state_ref(), b.state_ref()) and np.array_equal(a.get_epoch(), b.get_epoch())
    one = variable_autocorrelation(a, T * freq, 1.5, sampling_freq=freq, r=1, device="record")
    assert one.shape == (T,)


def test_record_autocorrelation_at_size(oracle):
    """32x32, R = 64, T = 1024 at beta = 2: all 1024 variables and all 2048 bonds against fft_autocorrelation of the recorded states."""
    import isingmontecarlo_amd as im
    from isingmontecarlo_amd.autocorrelations import fft_autocorrelation, variable_groups, bond_groups, bond_values
    edges = lat.two_d_ferro(32)
    R, T = 64, 1024
    g = im.QmcIsingGraph(edges, 1.0, 0.0, 1024, 2025, nreplicas=R, capacity=1 << 15)  # (n is about 5.2 beta N = 10^4; the cutoff 1.5 n)
    g.run(64, 2.0)
    g.attach_sample_record(T)
    g.run(T, 2.0)
    assert g.record_count() == T
    acv = g.record_autocorrelation(variable_groups(g.nvars)[0])
    acb = g.record_autocorrelation(bond_groups(g)[0])
    assert acv.shape == acb.shape == (R, T) and len(bond_groups(g)[0]) == 2048
    for r in (0, 31, 63):
        st = g.record_states(r=r)
        wv = fft_autocorrelation(st.astype(np.float64) * 2.0 - 1.0)
        wb = fft_autocorrelation(bond_values(g, st))
        ev, eb = np.abs(acv[r] - wv).max(), np.abs(acb[r] - wb).max()
        print("at size r =", r, "variables", ev, "bonds", eb)
        assert ev < 1e-10 and eb < 1e-10


def test_timesteps_sample_returns_the_recorded_states_and_the_energy_of_timesteps(oracle):
    _, edges, gamma, h, beta = MODELS["ferro8x8"]
    R = 4
    g, m, reps = make_pair(oracle, edges, gamma, h, 8, 8192, 606, R)
    twin, _, _ = make_pair(oracle, edges, gamma, h, 8, 8192, 606, R)
    states, energy = g.timesteps_sample(30, beta, 3)
    want_e = twin.timesteps(30, beta, 3)
    assert states.shape == (10, R, g.nvars) and np.array_equal(energy, want_e)
    assert g.record_capacity() == 0
    for k in range(10):
        for r, rep in enumerate(reps):
            rep.timesteps(3, beta, 3, 0)
            assert np.array_equal(states[k, r], rep.state())
    # with a record attached that has room, the samples go there and stay
    g.attach_sample_record(12)
    g.run(4, beta, 2)
    states2, _ = g.timesteps_sample(20, beta, 2)
    twin.run(4, beta, 2); twin.timesteps(20, beta, 2)
    assert g.record_count() == 12 and np.array_equal(g.record_states(2, 10), states2)
    assert np.array_equal(states2[-1], twin.state_ref())
