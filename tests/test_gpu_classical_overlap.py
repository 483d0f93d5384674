"""Overlaps between copies of a realisation on the device (GraphState.attach_overlaps / tempering_run(overlaps=True),
csrc/sse_classical_overlap.hip.h) against isingmc_classical_host_pt_run_overlaps, the same rounds by the sequential rule on the CPU,
which tests/test_classical_overlap_cpu.py holds to the numpy restatement and to exact enumeration.  The measured values are integers
and the runs they are measured on equal the host's bit for bit (tests/test_gpu_classical_pt.py), so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _classical_cases as cc
import _classical_overlap_cases as oc
import _classical_pt_cases as pc

pytestmark = pytest.mark.gpu


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


def _graph(edges, biases, betas, chains, ncopies=2, replica_offset=0, cfg_flags=0, couplings=None, attach=True):
    import isingmontecarlo_amd as im
    g = im.GraphState(edges, biases, cc.SEED, nreplicas=chains * len(betas), replica_offset=replica_offset, cfg_flags=cfg_flags, couplings=couplings)
    g.attach_tempering(betas)
    if attach:
        g.attach_overlaps(ncopies)
    return g


def _assert_equals_host(g, want, what, series=None, hists=True):
    assert np.array_equal(g.state_ref(), want["states"]), (what, "states")
    assert np.array_equal(g.get_epoch(), want["epochs"]), (what, "epochs")
    assert np.array_equal(g.counters(), want["counters"]), (what, "counters")
    assert np.array_equal(g.temperature_of(), want["temp_of"]) and g.tempering_step_number() == want["pt_step"], (what, "maps")
    if hists:
        hq, hl = g.overlap_histograms()
        assert hq.shape == want["overlap_hist"].shape and np.array_equal(hq, want["overlap_hist"]), (what, "overlap histogram")
        assert hl.shape == want["link_hist"].shape and np.array_equal(hl, want["link_hist"]), (what, "link histogram")
    if series is not None:
        for key in oc.SERIES:
            assert series[key].dtype == want[key].dtype and np.array_equal(series[key], want[key]), (what, key)


@pytest.mark.parametrize("name", list(oc.CASES))
def test_device_matches_the_host_run(name):
    """Every parity case in one call: both overlap series, both histograms, E and M, and the states, epochs, counters and maps."""
    cl = _cl()
    c = oc.CASES[name]
    g = _graph(c["edges"], c["biases"], c["betas"], c["chains"], c["ncopies"], oc.offset(name), cl.CFG_GLOBAL_TABLES if c["global_tables"] else 0, c["couplings"])
    series = g.tempering_run(c["rounds"], c["steps"], kinds=cl.KINDS_ALL, overlaps=True)
    _assert_equals_host(g, oc.host_parity_reference(name), name, series)
    assert g.launch_plan()["packed_edges"] == (len(c["biases"]) <= 65536)


RING = cc.CASES["ring33"]
LADDER4 = [0.2, 0.5, 1.0, 2.0]


def _host_ring(chains, rounds, replica_offset=0, **kw):
    cl = _cl()
    return oc.host_run(cl, RING[0], RING[1], LADDER4, chains, 2, rounds, 2, replica_offset=replica_offset, kinds=cl.KINDS_ALL, **kw)


def test_calls_compose_and_a_checkpoint_carries_the_histograms(tmp_path):
    """10 rounds in one call = 3 + 7 in two calls = 3 + 7 across a format-4 checkpoint into a fresh handle: the histograms add up and
    the series concatenate."""
    cl = _cl()
    want = _host_ring(4, 10)
    a, b = _graph(*RING, LADDER4, 4), _graph(*RING, LADDER4, 4)
    _assert_equals_host(a, want, "one call", a.tempering_run(10, 2, kinds=cl.KINDS_ALL, overlaps=True))
    s3 = b.tempering_run(3, 2, kinds=cl.KINDS_ALL, overlaps=True)
    assert (b.overlap_histograms()[0].sum(axis=3) == 3).all()
    path = str(tmp_path / "overlaps.npz")
    b.save_checkpoint(path)
    s7 = b.tempering_run(7, 2, kinds=cl.KINDS_ALL, overlaps=True)
    _assert_equals_host(b, want, "two calls", {k: np.concatenate([s3[k], s7[k]]) for k in s3})
    z = np.load(path)
    assert int(z["format"][0]) == 4 and int(z["ncopies"][0]) == 2 and z["ncopies"].dtype == np.uint32 and int(z["pt_step"][0]) == 3
    assert z["overlap_hist"].shape == (2, 1, 4, 34) and z["link_hist"].shape == (2, 1, 4, 34) and (z["link_hist"].sum(axis=3) == 3).all()
    d = _graph(*RING, LADDER4, 4, attach=False)  # the file brings the copies and the histograms
    d.load_checkpoint(path)
    s7 = d.tempering_run(7, 2, kinds=cl.KINDS_ALL, overlaps=True)
    _assert_equals_host(d, want, "checkpoint", {k: np.concatenate([s3[k], s7[k]]) for k in s3})


def test_a_plain_run_between_measured_calls_leaves_the_histograms_alone():
    """Thermalisation: tempering_run() on a handle with overlaps measures nothing; the states are those of the host run of all rounds."""
    cl = _cl()
    want = _host_ring(4, 10)
    g = _graph(*RING, LADDER4, 4)
    s3 = g.tempering_run(3, 2, kinds=cl.KINDS_ALL, overlaps=True)
    before = g.overlap_histograms()
    plain = g.tempering_run(4, 2, kinds=cl.KINDS_ALL)
    assert set(plain) == {"energy", "magnetization"} and np.array_equal(plain["energy"], want["energy"][3:7])
    after = g.overlap_histograms()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    s3b = g.tempering_run(3, 2, kinds=cl.KINDS_ALL, overlaps=True)
    _assert_equals_host(g, want, "3 measured + 4 plain + 3 measured", hists=False)
    rounds = [0, 1, 2, 7, 8, 9]
    for key in ("overlap", "link_overlap"):
        assert np.array_equal(np.concatenate([s3[key], s3b[key]]), want[key][rounds]), key
    hq, hl = g.overlap_histograms()
    assert (hq.sum(axis=3) == 6).all() and (hl.sum(axis=3) == 6).all()
    n = (33 - want["overlap"][rounds].astype(np.int64)) // 2
    assert all(np.array_equal(hq[i, 0, t], np.bincount(n[:, i, 0, t], minlength=34)) for i in range(2) for t in range(4))


def test_groups_shard_over_handles():
    """Two groups in one handle = two handles of one group at the replica offsets 0 and K T."""
    cl = _cl()
    whole = _graph(*RING, LADDER4, 4)
    lo, hi = _graph(*RING, LADDER4, 2, 2, 0), _graph(*RING, LADDER4, 2, 2, 8)
    sw, sl, sh = (g.tempering_run(5, 2, kinds=cl.KINDS_ALL, overlaps=True) for g in (whole, lo, hi))
    for key in ("overlap", "link_overlap"):
        assert np.array_equal(sw[key], np.concatenate([sl[key], sh[key]], axis=1)), key
    for i in range(2):
        assert np.array_equal(whole.overlap_histograms()[i], np.concatenate([lo.overlap_histograms()[i], hi.overlap_histograms()[i]]))
    _assert_equals_host(whole, _host_ring(4, 5), "whole", sw)


def test_reset_zeroes_and_the_series_is_optional():
    cl = _cl()
    want = _host_ring(4, 6)
    a, b = _graph(*RING, LADDER4, 4), _graph(*RING, LADDER4, 4)
    assert a.tempering_run(6, 2, kinds=cl.KINDS_ALL, record=False, overlaps=True) is None
    _assert_equals_host(a, want, "record = False")
    b.tempering_run(2, 2, kinds=cl.KINDS_ALL, overlaps=True)
    b.reset_overlaps()
    assert not b.overlap_histograms()[0].any() and not b.overlap_histograms()[1].any()
    s = b.tempering_run(4, 2, kinds=cl.KINDS_ALL, overlaps=True)
    assert np.array_equal(s["overlap"], want["overlap"][2:]) and (b.overlap_histograms()[0].sum(axis=3) == 4).all()
    m = a.overlap_moments()
    q = want["overlap"][:, :, 0, :].astype(np.float64) / 33.0  # [rounds][G][T]: one pair a group
    assert m["q2"].shape == (2, 4) and np.allclose(m["q2"], (q ** 2).mean(axis=0), rtol=1e-13) and np.allclose(m["q4"], (q ** 4).mean(axis=0), rtol=1e-13)
    assert np.allclose(m["binder"], 0.5 * (3.0 - (q ** 4).mean(axis=0) / (q ** 2).mean(axis=0) ** 2), rtol=1e-12)
    assert a.tempering_run(0, 2, overlaps=True)["overlap"].shape == (0, 2, 1, 4)


def test_importance_sampling_rebuild_keeps_the_overlap_state():
    cl = _cl()
    edges, biases = cc.CASES["ring33_positive"]
    g = _graph(edges, biases, LADDER4, 4)
    g.tempering_run(4, 2, kinds=cl.KINDS_ALL, overlaps=True)
    hq, hl = g.overlap_histograms()
    st, ep, tof = g.state_ref(), g.get_epoch(), g.temperature_of()
    g.enable_edge_importance_sampling(True)
    assert np.array_equal(g.overlap_histograms()[0], hq) and np.array_equal(g.overlap_histograms()[1], hl)
    s = g.tempering_run(3, 2, kinds=cl.KINDS_ALL, overlaps=True)
    want = cl.host_tempering_run(edges, biases, cc.SEED, st, ep, LADDER4, 3, 2, kinds=cl.KINDS_ALL, temp_of=tof, pt_step=4, flags=cl.CFG_EDGE_IMPORTANCE, ncopies=2,
                                 histograms=(hq, hl))
    assert np.array_equal(s["overlap"], want["overlap"]) and np.array_equal(s["link_overlap"], want["link_overlap"])
    assert np.array_equal(g.overlap_histograms()[0], want["overlap_hist"]) and np.array_equal(g.overlap_histograms()[1], want["link_hist"])


@pytest.mark.parametrize("name", list(cc.ENUM_SYSTEMS))
def test_device_overlaps_match_exact_enumeration(name):
    """The inputs of the CPU enumeration test on the device: 1024 groups of 2 copies, T = 4, 48 rounds of one only_basic_moves step;
    Q^2 / N^2 and QL of the last round within 4.5 exact standard deviations over sqrt(1024) at every temperature.  The device equals
    the host entry bit for bit, so the CPU run predicts the outcome: at most 1.7 sigma."""
    edges, biases = cc.ENUM_SYSTEMS[name]
    g = _graph(edges, biases, pc.enum_pt_betas(name), pc.ENUM_PT_CHAINS)
    s = g.tempering_run(pc.ENUM_PT_ROUNDS, 1, only_basic_moves=True, overlaps=True)
    assert s["overlap"].shape == (pc.ENUM_PT_ROUNDS, oc.ENUM_GROUPS, 1, 4) and (g.get_epoch() == pc.ENUM_PT_ROUNDS).all()
    sigmas = oc.enum_overlap_sigmas(name, s["overlap"][-1, :, 0, :], s["link_overlap"][-1, :, 0, :])
    assert max(max(x) for x in sigmas) <= cc.ENUM_SIGMAS, sigmas
    hq, hl = g.overlap_histograms()
    assert (hq.sum(axis=3) == pc.ENUM_PT_ROUNDS).all() and (hl.sum(axis=3) == pc.ENUM_PT_ROUNDS).all()


def test_refusals_on_a_handle():
    """Overlaps need tempering and the other overlap calls need overlaps; a refused attach leaves the handle as it was; attaching
    tempering again detaches the overlaps."""
    cl = _cl()
    import isingmontecarlo_amd as im
    g = im.GraphState(*RING, cc.SEED, nreplicas=16)
    lib, h = g._lib, g._h
    assert lib.isingmc_classical_overlap_attach(h, 2) == -1 and b"isingmc_classical_pt_attach first" in lib.isingmc_classical_last_error(h)
    with pytest.raises(im.IsingMcError):
        g.attach_overlaps(2)
    g.attach_tempering(LADDER4)
    buf = np.zeros(4 * 4 * 34, dtype=np.uint64)
    for rc in (lib.isingmc_classical_pt_run_overlaps(h, 1, 1, cl.NONE, cl.NONE, cl.NONE, 0, None, None, None, None),
               lib.isingmc_classical_overlap_histograms(h, im._ptr(buf, C.c_uint64), None),
               lib.isingmc_classical_overlap_set_histograms(h, im._ptr(buf, C.c_uint64), im._ptr(buf, C.c_uint64)),
               lib.isingmc_classical_overlap_reset(h)):
        assert rc == -1 and b"isingmc_classical_overlap_attach first" in lib.isingmc_classical_last_error(h)
    for call in (lambda: g.tempering_run(1, 1, overlaps=True), g.overlap_histograms, g.reset_overlaps, g.overlap_moments):
        with pytest.raises(im.IsingMcError):
            call()
    for ncopies, words in ((1, "ncopies >= 2"), (3, "multiple of ncopies"), (8, "multiple of ncopies")):
        with pytest.raises(im.IsingMcError) as ei:
            g.attach_overlaps(ncopies)
        assert ei.value.code == -1 and words in str(ei.value)
    g.attach_overlaps(4)  # one group of four copies: six pairs
    assert g.overlap_histograms()[0].shape == (1, 6, 4, 34)
    with pytest.raises(im.IsingMcError):
        g.attach_overlaps(3)
    assert g.tempering_run(2, 1, overlaps=True)["overlap"].shape == (2, 1, 6, 4)  # refused: the four copies stay attached
    assert lib.isingmc_classical_overlap_set_histograms(h, None, im._ptr(buf, C.c_uint64)) == -1 and b"null buffer" in lib.isingmc_classical_last_error(h)
    g.attach_tempering(LADDER4)  # the shape of the batch may have changed: the overlaps are detached
    with pytest.raises(im.IsingMcError):
        g.tempering_run(1, 1, overlaps=True)
    g.attach_overlaps(2)
    g.attach_overlaps(0)  # detaches
    with pytest.raises(im.IsingMcError):
        g.overlap_histograms()
    with pytest.raises(im.IsingMcError) as ei:
        _graph(*RING, LADDER4, 2, 2, replica_offset=4)
    assert "a group does not straddle" in str(ei.value)
    rows = np.tile(np.array([j for _, j in RING[0]]), (16, 1))
    rows[4:8] = -rows[4:8]  # the second chain of group 0 is another realisation
    with pytest.raises(im.IsingMcError) as ei:
        _graph(*RING, LADDER4, 4, couplings=rows)
    assert "group 0 (replicas 0 .. 7) differ" in str(ei.value)
