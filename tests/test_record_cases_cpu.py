"""CPU tests of tests/_record_cases.py: the fast yardstick of the exact autocorrelation equals autocorrelations.bit_autocorrelation
bit for bit, the table of lengths equals the restated launch rule of bit_autocorr_kernel, and the two LDS boundaries of
record.hip follow from the header's size functions and 160 KiB.  The inputs of the device cases (tests/test_gpu_sample_record_edges.py)
are checked here on the CPU oracle's trajectory, which the device's equals bit for bit."""
import numpy as np
import pytest

import _record_cases as rc


def test_constants_come_from_the_launch_header():
    assert set(rc.K) >= {"OBS_TILE", "OBS_SERIES_WAVES", "OBS_LAGS", "OBS_MAX_THREADS"}
    assert rc.OBS_TILE == 64  # one wave's ballot: record_series_kernel writes a tile as two words
    assert rc.OBS_MAX_THREADS % 64 == 0 and rc.OBS_MAX_THREADS <= 1024 and rc.OBS_LAGS >= 1 and rc.OBS_SERIES_WAVES >= 1


# (T, n, constant column): lengths of the table up to 8193; bit_autocorrelation is O(T^2) with a Python loop, so n stays small
FAST_SHAPES = [(1, 3, None), (33, 5, 2), (256, 4, 0), (257, 7, 3), (1000, 3, 1), (2049, 3, 2), (4097, 6, 5), (8193, 2, 0)]


@pytest.mark.parametrize("tmax,n,constant", FAST_SHAPES)
def test_fast_bit_autocorrelation_equals_bit_autocorrelation(tmax, n, constant):
    from isingmontecarlo_amd.autocorrelations import bit_autocorrelation
    bits = rc.correlated_bits(31 + tmax, tmax, n, constant=constant)
    got, want = rc.fast_bit_autocorrelation(bits), bit_autocorrelation(bits)
    assert got.shape == want.shape == (tmax,) and got.dtype == want.dtype == np.float64
    assert np.array_equal(got, want)
    if tmax > 1:
        assert np.abs(want).max() > 0  # (not the comparison of two zero arrays)


def test_fast_bit_autocorrelation_of_constant_and_single_sample_series():
    from isingmontecarlo_amd.autocorrelations import bit_autocorrelation
    for bits in (np.ones((9, 3), dtype=np.uint8), np.zeros((257, 2), dtype=np.uint8), np.array([[0, 1, 1]]), np.array([[1]])):
        got = rc.fast_bit_autocorrelation(bits)
        assert np.array_equal(got, bit_autocorrelation(bits)) and np.array_equal(got, np.zeros(len(bits)))
    with pytest.raises(ValueError):
        rc.fast_bit_autocorrelation(np.zeros((0, 3)))


def test_length_table_equals_the_launch_rule():
    for tmax, geometry in rc.AUTOCORR_LENGTHS.items():
        assert rc.autocorr_geometry(tmax) == geometry, tmax
        assert rc.autocorr_accepted(tmax)
    # what the issue's table says each length is there for
    assert rc.autocorr_geometry(256) == (64, 1) and rc.autocorr_geometry(257) == (128, 1)
    assert rc.dead_lag_lanes(1000) == [0, 0, 0, 256 - 232]       # the 4th lag is dead for lanes >= 232
    assert rc.dead_lag_lanes(4096) == [0, 0, 0, 0]
    assert rc.dead_lag_lanes(4095) == [0, 0, 0, 1]
    assert rc.dead_lag_lanes(4097) == [1023, 1024, 1024, 1024]   # the second pass has one live lag
    assert rc.dead_lag_lanes(8192) == [0, 0, 0, 0]               # two full passes
    assert [rc.autocorr_geometry(t)[1] for t in (8193, 16385)] == [3, 5]
    assert {g[0] for g in rc.AUTOCORR_LENGTHS.values()} >= {64, 128, 256, 512, 1024}
    assert {2047, 2048, 2049} <= set(rc.AUTOCORR_LENGTHS)        # around a word end inside the multi-wave range
    # the existing exact test (T <= 200) is one wave, one pass throughout
    assert {rc.autocorr_geometry(t) for t in (1, 31, 32, 33, 64, 77, 200)} == {(64, 1)}
    assert rc.AUTOCORR_SAMPLES == 16390
    # which waves add to the shared population count: wave 0 alone up to Tw = 64, nine of sixteen at the table's longest
    assert [rc.counting_waves(t) for t in (257, 1000, 2048, 2049, 4096, 16385)] == [(1, 1), (1, 1), (1, 1), (2, 1), (2, 1), (9, 1)]
    longest, geometry = rc.AUTOCORR_LONGEST
    assert rc.autocorr_geometry(longest) == geometry == (1024, 9) and rc.counting_waves(longest) == (16, 2) and rc.autocorr_accepted(longest)
    assert rc.counting_waves(longest - 32) == (16, 1)


def test_series_lengths_and_models_reach_what_they_are_there_for():
    assert rc.SERIES_LENGTHS == [63, 65, 95, 96, 97, 127, 128, 129] and rc.SERIES_LONG == 4097
    assert rc.series_tiles(63) == 1 and rc.series_tiles(65) == 2 and rc.series_tiles(128) == 2 and rc.series_tiles(129) == 3
    assert rc.series_tiles(4097) == 65
    assert all(m[3] >= 130 for m in rc.MODELS.values())
    by_n = {m[0]: name for name, m in rc.MODELS.items()}
    assert set(by_n) == {1, 32, 2048, 2080, 20448} and {m[1] for m in rc.MODELS.values()} == {1, 3, 5}
    assert rc.nwords_of(32) == 1 and rc.nwords_of(1) == 1
    assert rc.nwords_of(2048) == 64 and rc.obs_row_stride(64) == 65 and rc.staging_trips(64) == (1, 64)
    assert rc.nwords_of(2080) == 65 and rc.obs_row_stride(65) == 65 and rc.staging_trips(65) == (2, 1)
    assert rc.nwords_of(20448) == 639 and rc.staging_trips(639) == (10, 63)
    # the odd stride differs from nwords + 1 only for odd nwords
    assert rc.obs_row_stride(65) != 65 + 1 and rc.obs_row_stride(639) == 639 and rc.obs_row_stride(640) == 641
    for name, (nvars, R, seed, samples) in rc.MODELS.items():
        lists = rc.group_lists(nvars)
        assert {len(lists[k][0]) for k in ("one", "three", "four", "constants_around")} == {1, 3, 4, 5}
        assert len(lists["many"][0]) > 3000
        for what, (groups, constant) in lists.items():
            assert all(0 <= v < nvars for g in groups for v in g), (name, what)
            if constant is not None:
                assert constant == rc.constant_by_construction(groups), (name, what)
        want = {v for v in (31, 32, 63, 64, 32 * (rc.nwords_of(nvars) - 1), nvars - 1) if v < nvars}
        assert want <= {g[0] for g in lists["edges"][0]}
    assert len(rc.group_lists(2080)["all"][0][0]) == 2080


def test_lds_boundaries_follow_from_the_header_and_160_kib():
    assert rc.LDS_WORDS == 40960
    lo, hi = rc.NWORDS_EDGE
    assert (lo, hi) == (639, 640)
    assert rc.obs_series_lds_words(lo) == 64 * 639 == 40896 and rc.series_accepted(lo)
    assert rc.obs_series_lds_words(hi) == 64 * 641 == 41024 and not rc.series_accepted(hi)
    assert rc.nwords_of(rc.MODELS["n20448"][0]) == lo and rc.nwords_of(rc.REFUSED_MODEL[0]) == hi
    assert rc.series_accepted(rc.nwords_of(20448)) and not rc.series_accepted(rc.nwords_of(20449))
    lo, hi = rc.T_EDGE
    assert (lo, hi) == (655328, 655329)
    assert rc.obs_autocorr_lds_words(lo) + 2 == 2 * 20479 + 2 == 40960 and rc.autocorr_accepted(lo)
    assert rc.obs_autocorr_lds_words(hi) + 2 == 40962 and not rc.autocorr_accepted(hi)
    assert hi <= 1 << 20  # isingmc_record_attach accepts a record of that many rows: the refusal is the kernel's, not the record's


def test_pack_series_and_observe():
    rng = np.random.default_rng(3)
    states = (rng.random((77, 40)) < 0.5).astype(np.uint8)
    groups = [[0], [39, 39], [1, 2, 3], [5, 5, 7]]
    flips = np.array([0, 1, 1, 0], dtype=np.uint8)
    bits = rc.observe(states, groups, flips)
    assert np.array_equal(bits[:, 0], states[:, 0]) and (bits[:, 1] == 1).all()
    assert np.array_equal(bits[:, 2], (states[:, 1] + states[:, 2] + states[:, 3] + 1) & 1) and np.array_equal(bits[:, 3], states[:, 7])
    words = rc.pack_series(bits)
    assert words.shape == (4, 3) and words.dtype == np.uint32
    for g in range(4):
        for t in range(96):
            assert (int(words[g, t >> 5]) >> (t & 31)) & 1 == (int(bits[t, g]) if t < 77 else 0)


def oracle_rows(oracle, edges, nvars, gamma, beta, cutoff, capacity, seed, R, samples, state=None):
    """[samples][R][nvars]: the states the oracle's replicas hold after each of `samples` timesteps."""
    import _lattices as lat
    e, j = lat.split(edges)
    m = oracle.Model(nvars, e, j, gamma, 0.0)
    reps = [oracle.Replica(m, capacity, cutoff, seed, r, state) for r in range(R)]
    rows = np.zeros((samples, R, nvars), dtype=np.uint8)
    for k in range(samples):
        for r, rep in enumerate(reps):
            rep.timesteps(1, beta)
            rows[k, r] = rep.state()
    return rows


@pytest.mark.parametrize("name", list(rc.MODELS))
def test_series_inputs_are_not_trivial(oracle, name):
    """The condition of the device cases on their inputs (check_rows, check_series), on the oracle's trajectory."""
    nvars, R, seed, samples = rc.MODELS[name]
    rows = oracle_rows(oracle, rc.model_edges(nvars), nvars, rc.GAMMA, rc.BETA, 8, rc.model_capacity(nvars), seed, R, samples, rc.initial_state(nvars, seed))
    rc.check_rows(rows, name)
    first, shortest = max(rc.SERIES_FIRSTS), min(rc.SERIES_LENGTHS)
    for what, (groups, constant) in rc.group_lists(nvars).items():
        constant = rc.constant_by_construction(groups) if constant is None else constant
        for r in range(R):
            rc.check_series(rc.observe(rows[first:first + shortest, r], groups), constant, f"{name} {what} r={r} T={shortest}")


def test_autocorrelation_inputs_are_not_trivial(oracle):
    import _lattices as lat
    from test_sample_record_cpu import _Graph  # what bond_groups asks of a graph
    M = rc.AUTOCORR_MODEL
    edges = lat.two_d_periodic(M["side"])
    nvars = M["side"] ** 2
    # one trajectory: the record of the table's lengths is the first half of the record of the longest length
    samples = rc.AUTOCORR_LONGEST[0] + max(rc.AUTOCORR_FIRSTS)
    assert samples >= rc.AUTOCORR_SAMPLES
    rows = oracle_rows(oracle, edges, nvars, M["gamma"], M["beta"], M["cutoff"], M["capacity"], M["seed"], M["R"], samples)
    rc.check_rows(rows, "6x6")
    g = _Graph(edges)
    first, shortest = max(rc.AUTOCORR_FIRSTS), min(rc.AUTOCORR_LENGTHS)
    for what, groups in rc.autocorr_observables(g).items():
        constant = rc.constant_by_construction(groups)
        if what == "products":
            assert constant == [0, 3, 9] and len(groups) == 10  # a constant series before, between and after live ones
        for r in range(M["R"]):
            rc.check_series(rc.observe(rows[first:first + shortest, r], groups), constant, f"6x6 {what} r={r} T={shortest}")
