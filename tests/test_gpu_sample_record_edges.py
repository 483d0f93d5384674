"""GPU tests of the sample record's kernels past one wave, one pass and 64 state words (tests/_record_cases.py has the cases and
the reasons): bit_autocorr_kernel against the exact host yardstick at every launch geometry up to five passes, record_series_kernel
against numpy parities of the recorded states on models of 1 to 639 state words, the two LDS refusals of record.hip with the
largest accepted sizes next to them, and isingmc_record_read's piece loop.

Every comparison is np.array_equal: the autocorrelation is integers up to one correctly rounded division per observable and lag,
added in a fixed order, so there is nothing to tolerate."""
import numpy as np
import pytest

import _lattices as lat
import _record_cases as rc
from test_gpu_parity import make_pair, assert_same

pytestmark = pytest.mark.gpu


# ---- autocorrelations: one recorded run of the 6x6 lattice for every length ----
def _autocorr_batch(nreplicas, replica_offset, samples=rc.AUTOCORR_SAMPLES):
    import isingmontecarlo_amd as im
    M = rc.AUTOCORR_MODEL
    g = im.QmcIsingGraph(lat.two_d_periodic(M["side"]), M["gamma"], 0.0, M["cutoff"], M["seed"], nreplicas=nreplicas, capacity=M["capacity"],
                         replica_offset=replica_offset)
    g.attach_sample_record(samples)
    g.run(samples, M["beta"])
    assert g.record_count() == samples
    return g


@pytest.fixture(scope="module")
def recorded():
    """(the R = 3 batch, its recorded states [T][3][36], an R = 1 batch that is replica 1 of it, the observables); read-only."""
    g = _autocorr_batch(rc.AUTOCORR_MODEL["R"], 0)
    states = g.record_states()
    one = _autocorr_batch(1, 1)
    # the same seed and replica index: the same trajectory (Philox counters carry the replica index, not the position in the batch)
    assert np.array_equal(one.record_states()[:, 0], states[:, 1]), "replica_offset = 1 does not reproduce replica 1 of the batch"
    assert np.array_equal(states[-1], g.state_ref())
    rc.check_rows(states, "6x6")
    states.setflags(write=False)
    yield g, states, one, rc.autocorr_observables(g)
    g.close(); one.close()


@pytest.mark.parametrize("T", list(rc.AUTOCORR_LENGTHS))
def test_autocorrelation_is_exact_at_every_launch_geometry(recorded, T):
    g, states, one, observables = recorded
    R = states.shape[1]
    for what, groups in observables.items():
        constant = rc.constant_by_construction(groups)
        for first in rc.AUTOCORR_FIRSTS:
            got = g.record_autocorrelation(groups, first, T)
            assert got.shape == (R, T) and got.dtype == np.float64
            assert np.array_equal(got, g.record_autocorrelation(groups, first, T)), f"{what} first={first} T={T}: two calls differ"
            for r in range(R):
                bits = rc.observe(states[first:first + T, r], groups)
                rc.check_series(bits, constant, f"{what} first={first} T={T} r={r}")
                want = rc.fast_bit_autocorrelation(bits)
                bad = np.flatnonzero(got[r] != want)
                print(f"{what} first={first} T={T} r={r}: {len(bad)} lags differ" + (f", the first at {bad[0]}, max diff {np.abs(got[r] - want).max()}" if len(bad) else ""))
                assert np.array_equal(got[r], want), f"{what} first={first} T={T} r={r}: {len(bad)} lags differ, the first at {bad[0]}"
            alone = one.record_autocorrelation(groups, first, T)
            assert alone.shape == (1, T) and np.array_equal(alone[0], got[1]), f"{what} first={first} T={T}: replica 1 alone differs from its row in the batch"


def test_autocorrelation_when_every_wave_counts_and_a_lane_counts_two_words():
    """T = 32769 (Tw = 1025): all 16 waves add their population counts to the shared counter and lane 0 counts words 0 and 1024;
    nine passes.  A record of its own (the same trajectory, twice as long), the product observables only."""
    T, geometry = rc.AUTOCORR_LONGEST
    assert rc.autocorr_geometry(T) == geometry and rc.counting_waves(T) == (16, 2)
    g = _autocorr_batch(rc.AUTOCORR_MODEL["R"], 0, T + max(rc.AUTOCORR_FIRSTS))
    states = g.record_states()
    rc.check_rows(states, "6x6 long")
    groups = rc.autocorr_observables(g)["products"]
    constant = rc.constant_by_construction(groups)
    for first in rc.AUTOCORR_FIRSTS:
        got = g.record_autocorrelation(groups, first, T)
        assert np.array_equal(got, g.record_autocorrelation(groups, first, T)), f"first={first}: two calls differ"
        for r in range(states.shape[1]):
            bits = rc.observe(states[first:first + T, r], groups)
            rc.check_series(bits, constant, f"products first={first} T={T} r={r}")
            want = rc.fast_bit_autocorrelation(bits)
            bad = np.flatnonzero(got[r] != want)
            assert np.array_equal(got[r], want), f"products first={first} T={T} r={r}: {len(bad)} lags differ, the first at {bad[0]}"
    g.close()


# ---- series: models of 1 to 639 state words ----
def _series_batch(nvars, R, seed, samples):
    import isingmontecarlo_amd as im
    g = im.QmcIsingGraph(rc.model_edges(nvars), rc.GAMMA, 0.0, 8, seed, state=rc.initial_state(nvars, seed), nreplicas=R,
                         capacity=rc.model_capacity(nvars), nvars=nvars)
    g.attach_sample_record(samples)
    g.run(samples, rc.BETA)
    assert g.record_count() == samples
    return g


@pytest.mark.parametrize("name", list(rc.MODELS))
def test_series_equals_numpy_parities(name):
    nvars, R, seed, samples = rc.MODELS[name]
    g = _series_batch(nvars, R, seed, samples)
    rows = g.record_states()
    assert rows.shape == (samples, R, nvars) and np.array_equal(rows[-1], g.state_ref())
    rc.check_rows(rows, name)
    lengths = rc.SERIES_LENGTHS + ([rc.SERIES_LONG] if samples >= rc.SERIES_LONG + max(rc.SERIES_FIRSTS) else [])
    for what, (groups, constant) in rc.group_lists(nvars).items():
        constant = rc.constant_by_construction(groups) if constant is None else constant
        flips = rc.random_flips(len(groups))
        full = [rc.observe(rows[:, r], groups) for r in range(R)]  # [samples][n] per replica: a window's parities are a slice
        for first in rc.SERIES_FIRSTS:
            for T in lengths:
                if what == "many" and T not in (65, 129, rc.SERIES_LONG):
                    continue
                with_flips = g.record_series(groups, flips, first, T)
                without = g.record_series(groups, None, first, T)
                assert with_flips.shape == without.shape == (R, len(groups), (T + 31) // 32) and with_flips.dtype == np.uint32
                for r in range(R):
                    bits = full[r][first:first + T]
                    rc.check_series(bits, constant, f"{name} {what} first={first} T={T} r={r}")
                    assert np.array_equal(without[r], rc.pack_series(bits)), f"{name} {what} first={first} T={T} r={r} without flips"
                    assert np.array_equal(with_flips[r], rc.pack_series(bits ^ flips[None, :])), f"{name} {what} first={first} T={T} r={r} with flips"
        if what == "three":  # [w, w] is the constant 0 and [w, w, v] is [v], on the device too
            got = g.record_series(groups, None, 0, 129)
            assert not got[:, 1].any() and np.array_equal(got[:, 2], got[:, 0]) and got[:, 0].any()
    if name == "n20448":  # the largest accepted model through both kernels
        for what in ("edges", "constants_around"):
            groups = rc.group_lists(nvars)[what][0]
            for first, T in ((0, 129), (5, 128)):
                got = g.record_autocorrelation(groups, first, T)
                for r in range(R):
                    assert np.array_equal(got[r], rc.fast_bit_autocorrelation(rc.observe(rows[first:first + T, r], groups))), f"{what} first={first} T={T} r={r}"
    g.close()


def test_recorded_rows_of_a_wide_model_are_the_oracles(oracle):
    """The numpy side of the series tests rests on record_states: rows 0, 1 and last of the 65-word model against the oracle's replicas."""
    nvars, R, seed, samples = rc.MODELS[rc.ORACLE_MODEL]
    g, m, reps = make_pair(oracle, rc.model_edges(nvars), rc.GAMMA, 0.0, 8, rc.model_capacity(nvars), seed, R, state=rc.initial_state(nvars, seed), nvars=nvars)
    g.attach_sample_record(samples)
    g.run(samples, rc.BETA)
    rows = g.record_states()
    for k in range(samples):
        for r, rep in enumerate(reps):
            rep.timesteps(1, rc.BETA)
            if k in (0, 1, samples - 1):
                assert np.array_equal(rows[k, r], rep.state()), f"row {k} of replica {r} differs from the oracle"
    assert np.array_equal(rows[-1], g.state_ref())
    assert_same(g, reps, "after recording")
    g.close()


# ---- refusals ----
def _refused(call, code, text):
    import isingmontecarlo_amd as im
    with pytest.raises(im.IsingMcError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    assert text in str(ei.value), str(ei.value)


def test_a_model_of_640_state_words_is_refused_by_the_kernels_only():
    nvars, R, seed = rc.REFUSED_MODEL
    g = _series_batch(nvars, R, seed, 4)
    rows = g.record_states()
    assert rows.shape == (4, R, nvars) and np.array_equal(rows[-1], g.state_ref()) and (rows[0] != rows[1]).any()
    groups = [[0], [nvars - 1]]
    _refused(lambda: g.record_series(groups, None, 0, 4), rc.ENOTIMPL, "exceed LDS")
    _refused(lambda: g.record_autocorrelation(groups, 0, 4), rc.ENOTIMPL, "exceed LDS")
    # the batch and its record work afterwards
    g.attach_sample_record(8)
    g.run(6, rc.BETA)
    again = g.record_states()
    assert g.record_count() == 6 and np.array_equal(again[-1], g.state_ref()) and np.array_equal(g.record_states(r=0), again[:, 0])
    assert g.verify().all()
    g.close()


def test_the_longest_series_and_the_order_of_the_checks():
    """isingmc_record_autocorrelation: the LDS limit comes first when a record is attached, then the row range; without a record
    the missing record is what is reported.  None of this needs a record of 655328 rows."""
    import isingmontecarlo_amd as im
    accepted, refused = rc.T_EDGE
    g = im.QmcIsingGraph(lat.two_d_periodic(4), 1.0, 0.0, 16, 7, nreplicas=2, capacity=1 << 11)
    groups = [[0], [1, 2]]
    _refused(lambda: g.record_autocorrelation(groups, 0, refused), rc.EINVAL, "no sample record attached")
    g.attach_sample_record(8)
    g.run(8, 1.0)
    _refused(lambda: g.record_autocorrelation(groups, 0, refused), rc.ENOTIMPL, "exceeds LDS")
    _refused(lambda: g.record_autocorrelation(groups, 0, accepted), rc.EINVAL, "bad row range")
    # the batch works afterwards
    states = g.record_states()
    got = g.record_autocorrelation(groups, 0, 8)
    for r in range(2):
        assert np.array_equal(got[r], rc.fast_bit_autocorrelation(rc.observe(states[:, r], groups)))
    g.record_clear()
    g.run(3, 1.0)
    assert g.record_count() == 3 and np.array_equal(g.record_states()[-1], g.state_ref())
    assert g.verify().all()
    g.close()


# ---- read-back in pieces ----
def test_record_read_in_more_than_one_piece():
    """N = 1, R = 4096, 4100 rows: R * nwords * count exceeds the 2^24 words of one piece, so isingmc_record_read's loop runs twice
    (4096 rows, then 4), while the unpacked output is 16.8 MB."""
    import isingmontecarlo_amd as im
    R, count = 4096, 4100
    assert R * rc.nwords_of(1) * count > rc.READ_PIECE_WORDS >= R * rc.nwords_of(1) * (count // 2) and rc.READ_PIECE_WORDS // R < count
    g = im.QmcIsingGraph([], 1.0, 0.0, 8, 31, nreplicas=R, capacity=256, nvars=1)
    g.attach_sample_record(count)
    g.run(count, 0.5)
    rows = g.record_states()
    assert rows.shape == (count, R, 1) and rows.dtype == np.uint8 and rows.max() == 1 and rows.min() == 0
    assert (rows[1:] != rows[:-1]).any(axis=(1, 2)).all()  # every row differs from the one before
    for r in (0, 1, 63, 64, 2047, 2048, 4094, 4095):       # a replica alone is one piece
        assert np.array_equal(g.record_states(r=r), rows[:, r]), f"replica {r}"
    half = count // 2
    halves = np.concatenate([g.record_states(0, half), g.record_states(half, count - half)])
    assert np.array_equal(halves, rows)
    assert np.array_equal(rows[-1], g.state_ref())
    g.close()
