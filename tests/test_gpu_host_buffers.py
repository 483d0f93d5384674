"""The host layer's device buffers on the paths that grow, reuse and replace them (csrc/hip_host.h DevBuf behind the sample record's
scratch, the fold scratch, the accumulator table, the tempering state and the classical overlap histograms): a second and a third call
that meet a smaller, a larger or a fresh buffer return what the first kind of call returns.  A 4-site ring, two replicas (the
classical case needs two chains of two temperatures: four); every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RING = [((0, 1), 1.0), ((1, 2), -1.0), ((2, 3), 1.0), ((3, 0), 1.0)]
R, N, BETA = 2, 4, 1.0


def batch(seed=11):
    import isingmontecarlo_amd as im
    return im.QmcIsingGraph(RING, 1.0, 0.0, 16, seed, nreplicas=R, capacity=256)


def observe(states, groups, flips):
    """[T][N] states of one replica -> [T][G] bits: parity of the group's state bits ^ flip."""
    return np.stack([states[:, g].sum(axis=1) & 1 for g in groups], axis=1).astype(np.uint8) ^ np.asarray(flips, dtype=np.uint8)[None, :]


def pack_series(bits):
    """[T][G] bits -> uint32 [G][(T + 31) // 32], bit t & 31 of word t >> 5."""
    T, G = bits.shape
    padded = np.zeros((((T + 31) // 32) * 32, G), dtype=np.uint64)
    padded[:T] = bits
    return (padded.reshape(-1, 32, G) << np.arange(32, dtype=np.uint64)[None, :, None]).sum(axis=1).astype(np.uint32).T


def check_series(g, groups, flips, first, count):
    got = g.record_series(groups, flips, first, count)
    states = g.record_states()
    assert got.shape == (R, len(groups), (count + 31) // 32) and got.dtype == np.uint32
    for r in range(R):
        assert np.array_equal(got[r], pack_series(observe(states[first:first + count, r], groups, flips))), (groups, first, count, r)


def check_autocorrelation(g, groups, first, count):
    from isingmontecarlo_amd.autocorrelations import bit_autocorrelation
    got = g.record_autocorrelation(groups, first, count)
    states = g.record_states()
    assert got.shape == (R, count)
    for r in range(R):
        assert np.array_equal(got[r], bit_autocorrelation(observe(states[first:first + count, r], groups, [0] * len(groups)))), (groups, first, count, r)


def test_record_scratch_grows_is_reused_and_survives_a_new_record():
    g = batch()
    g.attach_sample_record(8)
    g.run(8, BETA)
    assert g.record_count() == 8
    one, three = ([[0]], [0]), ([[0], [1, 2], [0, 1, 2, 3]], [0, 1, 1])
    check_series(g, *one, 0, 2)    # the first buffers
    check_series(g, *three, 0, 8)  # groups and series both grow
    check_series(g, *one, 3, 2)    # the larger buffers serve a smaller call
    check_autocorrelation(g, three[0], 0, 2)
    check_autocorrelation(g, three[0], 0, 8)  # the output buffer grows
    check_autocorrelation(g, one[0], 1, 2)
    g.attach_sample_record(16)  # a new record, the scratch stays
    assert g.record_count() == 0 and g.record_capacity() == 16
    g.run(8, BETA)
    assert g.record_count() == 8
    check_series(g, *three, 0, 8)
    assert g.verify().all()
    g.close()


def host_folds(g, groups, flips):
    """(sum_all, sum_occ) of itime_groups by imaginary_time_fold over the exported strings."""
    out = np.zeros((2, R, len(groups)), dtype=np.int64)
    for r in range(R):
        ops = g.export_ops(r)
        slot = [0]

        def fold(acc, state):
            x = 2 * (observe(state[None, :].astype(np.int64), groups, flips)[0].astype(np.int64)) - 1
            acc[0] += x
            if ops[slot[0]]:
                acc[1] += x
            slot[0] += 1
            return acc
        acc = g.imaginary_time_fold(fold, [np.zeros(len(groups), dtype=np.int64), np.zeros(len(groups), dtype=np.int64)], r)
        assert slot[0] == len(ops)
        out[0, r], out[1, r] = acc
    return out[0], out[1]


def test_fold_scratch_grows_and_is_reused():
    g = batch(seed=12)
    g.run(8, BETA)
    assert (g.get_n() > 0).all()
    calls = [([[0]], [0]), ([[0], [1], [2, 3], [0, 1, 2, 3], [1, 3]], [0, 1, 0, 1, 1]), None, ([[2]], [1])]  # None: the bond counts in between
    for call in calls:
        if call is None:
            counts = g.bond_counts()
            assert counts.shape == (R, g.num_bonds())
            for r in range(R):
                assert [int(x) for x in counts[r]] == [g.get_bond_count(b, r) for b in range(g.num_bonds())]
            assert np.array_equal(counts.sum(axis=1), g.get_n())
            continue
        got_all, got_occ = g.itime_groups(*call)
        want_all, want_occ = host_folds(g, *call)
        assert np.array_equal(got_all, want_all) and np.array_equal(got_occ, want_occ), call
    g.close()


def test_accumulator_table_is_replaced_and_keeps_its_rows():
    g, twin = batch(seed=13), batch(seed=13)  # the twin keeps the identity rows it was created with
    for nrows, rows in [(2, [1, 0]), (4, [3, 1]), (2, [0, 1])]:
        resized = nrows != g.accumulators().shape[0]
        g.set_accumulator_rows(nrows, rows)
        if resized:  # a new table starts at zero
            assert not g.accumulators().any()
            twin.reset_accumulators()
        g.run(3, BETA)
        twin.run(3, BETA)
        acc, want = g.accumulators(), twin.accumulators()
        assert acc.shape == (nrows, 8) and want.shape == (R, 8) and want.any()
        assert np.array_equal(acc[rows], want), (nrows, rows)
        assert not np.delete(acc, rows, axis=0).any()  # rows that no replica maps to
        assert np.array_equal(g.state_ref(), twin.state_ref())
    g.close(); twin.close()


def pt_state(g):
    step, swaps = C.c_uint64(0), C.c_uint64(0)
    g._check(g._lib.isingmc_pt_get_state(g._h, C.byref(step), C.byref(swaps)))
    return int(step.value), int(swaps.value)


def test_tempering_state_created_twice():
    import isingmontecarlo_amd as im
    from isingmontecarlo_amd.tempering import NativeTemperingContainer
    g = batch(seed=14)
    betas = np.array([0.5, 2.0])

    def step_matches_pt_decide(pt, seed, step):
        pt.timesteps(4)
        config_at = np.zeros(R, dtype=np.uint32)
        config_at[pt.slot_of] = np.arange(R, dtype=np.uint32)
        want = im.pt_decide(seed, step, 1, 2, betas, g.get_n(), config_at)
        assert pt.tempering_step() == want
        assert np.array_equal(pt.slot_of[config_at], np.arange(R)), (step, pt.slot_of, config_at)
        return want

    first = NativeTemperingContainer(g, betas, 1, 77)
    swaps = sum(step_matches_pt_decide(first, 77, s) for s in range(3))
    assert pt_state(g) == (3, swaps)
    second = NativeTemperingContainer(g, betas, 1, 78)  # isingmc_pt_create again: the first state is released
    assert pt_state(g) == (0, 0) and np.array_equal(second.slot_of, np.arange(R)) and np.array_equal(second.local_betas, betas)
    swaps = sum(step_matches_pt_decide(second, 78, s) for s in range(3))
    assert pt_state(g) == (3, swaps) and second.verify()
    g.close()


def test_classical_overlaps_attached_detached_and_attached_again():
    import isingmontecarlo_amd as im
    import isingmontecarlo_amd.classical as cl
    betas, biases, nrep = [0.3, 1.2], [0.0] * N, 4  # two chains of two temperatures: one group of two copies
    init = (np.arange(nrep * N).reshape(nrep, N) * 7 // 3 & 1).astype(np.uint8)
    g = im.GraphState(RING, biases, 21, state=init, nreplicas=nrep)
    g.attach_tempering(betas)
    g.attach_overlaps(2)
    g.attach_overlaps(0)
    with pytest.raises(im.IsingMcError):
        g.overlap_histograms()
    g.attach_overlaps(2)
    assert not g.overlap_histograms()[0].any()
    got = g.tempering_run(2, 3, kinds=cl.KINDS_ALL, record=True, overlaps=True)
    want = cl.host_tempering_run(RING, biases, 21, init, 0, betas, 2, 3, kinds=cl.KINDS_ALL, ncopies=2)
    for key in ("energy", "magnetization", "overlap", "link_overlap"):
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    hq, hl = g.overlap_histograms()
    assert np.array_equal(hq, want["overlap_hist"]) and np.array_equal(hl, want["link_hist"]) and hq.sum() == 2 * 2  # rounds x temperatures
    assert np.array_equal(g.state_ref(), want["states"]) and np.array_equal(g.temperature_of(), want["temp_of"])
    assert np.array_equal(g.swap_counts()[0], want["attempts"]) and np.array_equal(g.swap_counts()[1], want["accepts"])
    g.attach_tempering(betas)  # detaches the overlaps
    assert g.tempering_step_number() == 0
    with pytest.raises(im.IsingMcError):
        g.overlap_histograms()
    assert g._lib.isingmc_classical_overlap_histograms(g._h, None, None) == -1  # (the library itself, not only the wrapper)
    assert g._lib.isingmc_classical_last_error(g._h).decode() == "isingmc_classical_overlap_histograms: call isingmc_classical_overlap_attach first"
    g.close()
