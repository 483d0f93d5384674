"""Isoenergetic cluster moves on the device (GraphState.attach_cluster_moves / tempering_run(cluster_moves=True),
csrc/sse_classical_icm.hip.h) against isingmc_classical_host_pt_run_icm, the same rounds by the sequential rule on the CPU, which
tests/test_classical_icm_cpu.py holds to the numpy restatement, to the move's transition matrix and to exact enumeration.  The moves
are integer work on runs that equal the host's bit for bit (tests/test_gpu_classical_overlap.py), so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _classical_cases as cc
import _classical_icm_cases as ic
import _classical_overlap_cases as oc
import _classical_pt_cases as pc

pytestmark = pytest.mark.gpu

STEPS_MAX_VARS = cc.LAYOUT_MAX_VARS  # the most variables a device batch takes: the state bits and stamps of one replica of the steps launch


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


def _graph(c, replica_offset=0, attach=True, waves=None, chains=None):
    """The batch of case dict `c` with tempering, overlaps and (attach) its window of cluster moves."""
    import isingmontecarlo_amd as im
    cl = _cl()
    chains = c["chains"] if chains is None else chains
    state = None if c["states"] is None else c["states"]
    g = im.GraphState(c["edges"], c["biases"], cc.SEED, state=state, nreplicas=chains * len(c["betas"]), replica_offset=replica_offset,
                      cfg_flags=cl.CFG_GLOBAL_TABLES if c["global_tables"] else 0, couplings=c["couplings"])
    g.attach_tempering(c["betas"])
    g.attach_overlaps(c["ncopies"])
    if attach:
        g.attach_cluster_moves(*c["window"], waves=waves)
    return g


def _counts_equal(g, want, what):
    got = g.cluster_move_counts()
    for key, name in zip(ic.COUNTS, ("moves", "empty", "size_sum")):
        assert got[name].shape == want[key].shape and got[name].dtype == np.uint64 and np.array_equal(got[name], want[key]), (what, key)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = want["cluster_size_sum"].astype(np.float64) / want["cluster_moves"].astype(np.float64)
    assert np.array_equal(got["mean_size"], mean, equal_nan=True), (what, "mean_size")


def _assert_equals_host(g, want, what, series=None, hists=True, counts=True):
    assert np.array_equal(g.state_ref(), want["states"]), (what, "states")
    assert np.array_equal(g.get_epoch(), want["epochs"]), (what, "epochs")
    assert np.array_equal(g.counters(), want["counters"]), (what, "counters")
    assert np.array_equal(g.temperature_of(), want["temp_of"]) and g.tempering_step_number() == want["pt_step"], (what, "maps")
    att, acc = g.swap_counts()
    assert np.array_equal(att, want["attempts"]) and np.array_equal(acc, want["accepts"]), (what, "swap counts")
    if hists:
        hq, hl = g.overlap_histograms()
        assert np.array_equal(hq, want["overlap_hist"]) and np.array_equal(hl, want["link_hist"]), (what, "histograms")
    if counts:
        _counts_equal(g, want, what)
    if series is not None:
        for key in series:
            assert series[key].dtype == want[key].dtype and np.array_equal(series[key], want[key]), (what, key)


@pytest.mark.parametrize("name", list(ic.CASES))
def test_device_matches_the_host_run(name):
    """Every case in one call, in every respect: states, epochs, counters, maps, swap counts, the four series, both histograms and the
    three cluster counts; launch_plan and cluster_move_plan agree with icm_plan and with what ran.
    A device batch holds at most 145632 variables at 160 KB of LDS (the state bits and stamps of one replica of the steps launch), which
    is below the two-wave gate of the cluster-move launch, 218432: the ring past that gate cannot be created, so the case asserts that
    refusal, and the one-wave launch runs on the ring past the four-wave gate with the waves forced to one."""
    cl = _cl()
    c = ic.case(name)
    n = len(c["biases"])
    if n > STEPS_MAX_VARS:
        assert name == "ring_past_2_waves_T2_K2" and cl.icm_plan(n, ic.LDS_BYTES)["waves"] == 1
        with pytest.raises(cl.IsingMcError) as ei:
            _graph(c, ic.offset(name))
        assert ei.value.code == -5 and f"at most {STEPS_MAX_VARS} variables" in str(ei.value)
        name, forced = "ring_past_4_waves_T2_K2", 1
        c, n = ic.case(name), len(ic.case(name)["biases"])
    else:
        forced = None
    g = _graph(c, ic.offset(name), waves=forced)
    series = g.tempering_run(c["rounds"], c["steps"], kinds=cl.KINDS_ALL, overlaps=True, cluster_moves=True)
    _assert_equals_host(g, ic.host_parity_reference(name), name, series)
    assert set(series) == set(ic.SERIES)
    plan, want = g.cluster_move_plan(), cl.icm_plan(n, ic.LDS_BYTES)
    assert plan == (dict(want, waves=forced, lds_words=forced * want["wave_words"]) if forced else want)
    assert plan["waves"] == (forced or (2 if c["gate"] == 4 else 4)) and plan["wave_words"] == 3 * ((n + 31) // 32)
    assert g.launch_plan()["packed_edges"] == (n <= 65536)


@pytest.mark.parametrize("waves", [1, 2])
def test_fewer_waves_move_the_same(waves):
    """The two-wave and the one-wave launch on a small case: 48 items over 24 and 48 workgroups."""
    cl = _cl()
    name = "lattice4x4_T8_K4"
    c = ic.case(name)
    g = _graph(c, ic.offset(name), waves=waves)
    series = g.tempering_run(c["rounds"], c["steps"], kinds=cl.KINDS_ALL, overlaps=True, cluster_moves=True)
    _assert_equals_host(g, ic.host_parity_reference(name), (name, waves), series)
    assert g.cluster_move_plan()["waves"] == waves
    with pytest.raises(cl.IsingMcError) as ei:
        g.attach_cluster_moves(waves=3)
    assert "waves must be 1, 2 or 4" in str(ei.value)


RING = cc.CASES["ring33"]
LADDER4 = [0.2, 0.5, 1.0, 2.0]
RING_CASE = ic._case(RING, LADDER4, 2, 4, window=(1, 4))
ON = dict(overlaps=True, cluster_moves=True)


def _host_ring(rounds, **kw):
    return ic.host_run(_cl(), RING_CASE, rounds=rounds, **kw)


def _continue_host(prev, rounds, cluster, ncopies=2, **kw):
    """`rounds` more rounds of the host run `prev`: with cluster moves, with the measurement only (ncopies = 2) or plain (None)."""
    cl = _cl()
    c = RING_CASE
    if ncopies is not None:
        kw["histograms"] = (prev["overlap_hist"], prev["link_hist"])
    if cluster:
        kw.update(cluster_moves=c["window"], cluster_counts=tuple(prev[k] for k in ic.COUNTS))
    out = cl.host_tempering_run(c["edges"], c["biases"], cc.SEED, prev["states"], prev["epochs"], c["betas"], rounds, c["steps"], kinds=cl.KINDS_ALL, temp_of=prev["temp_of"],
                                pt_step=prev["pt_step"], ncopies=ncopies, **kw)
    for key in ("counters", "attempts", "accepts"):  # (every host call counts from zero)
        out[key] = out[key] + prev[key]
    for key in ic.HISTS + ic.COUNTS:
        out.setdefault(key, prev[key])
    return out


def test_calls_compose_and_a_checkpoint_carries_the_cluster_state(tmp_path):
    """10 rounds in one call = 3 + 7 in two calls = 3 + 7 across a format-5 checkpoint into a fresh handle."""
    cl = _cl()
    want = _host_ring(10)
    a, b = _graph(RING_CASE), _graph(RING_CASE)
    _assert_equals_host(a, want, "one call", a.tempering_run(10, 2, kinds=cl.KINDS_ALL, **ON))
    s3 = b.tempering_run(3, 2, kinds=cl.KINDS_ALL, **ON)
    counts = b.cluster_move_counts()
    assert ((counts["moves"] + counts["empty"])[:, :, 1:] == 3).all() and not counts["moves"][:, :, 0].any()
    path = str(tmp_path / "cluster.npz")
    b.save_checkpoint(path)
    s7 = b.tempering_run(7, 2, kinds=cl.KINDS_ALL, **ON)
    _assert_equals_host(b, want, "two calls", {k: np.concatenate([s3[k], s7[k]]) for k in s3})
    z = np.load(path)
    assert int(z["format"][0]) == 5 and z["cluster_window"].tolist() == [1, 4] and z["cluster_window"].dtype == np.uint32 and int(z["ncopies"][0]) == 2
    assert z["cluster_moves"].shape == (2, 1, 4) and np.array_equal(z["cluster_moves"], counts["moves"]) and np.array_equal(z["cluster_size_sum"], counts["size_sum"])
    d = _graph(RING_CASE, attach=False)  # the file brings the window and the counts
    d.attach_overlaps(0)
    d.load_checkpoint(path)
    s7 = d.tempering_run(7, 2, kinds=cl.KINDS_ALL, **ON)
    _assert_equals_host(d, want, "checkpoint", {k: np.concatenate([s3[k], s7[k]]) for k in s3})
    plain = _graph(RING_CASE, attach=False)  # formats 1 to 4 still load: a format-4 file into a handle
    plain.tempering_run(2, 2, kinds=cl.KINDS_ALL, overlaps=True)
    path4 = str(tmp_path / "overlaps.npz")
    plain.save_checkpoint(path4)
    assert int(np.load(path4)["format"][0]) == 4
    d.load_checkpoint(path4)
    assert d.tempering_step_number() == 2
    with pytest.raises(cl.IsingMcError):  # ... whose ladder it attached again: the cluster moves are gone
        d.cluster_move_counts()


def test_runs_without_cluster_moves_leave_the_counts_alone():
    """3 rounds with cluster moves, 4 plain, 2 with the measurement only, 3 with cluster moves and no measurement, 2 with both: the plain
    and the measured calls make no move and leave the counts as they are, and every stretch equals the host's."""
    cl = _cl()
    g = _graph(RING_CASE)
    h = _host_ring(3)
    s = g.tempering_run(3, 2, kinds=cl.KINDS_ALL, **ON)
    _assert_equals_host(g, h, "3 with moves", s)
    before = g.cluster_move_counts()
    h = _continue_host(h, 4, False, ncopies=None)
    s = g.tempering_run(4, 2, kinds=cl.KINDS_ALL)
    _assert_equals_host(g, h, "4 plain", s)
    assert set(s) == {"energy", "magnetization"}
    h = _continue_host(h, 2, False)
    s = g.tempering_run(2, 2, kinds=cl.KINDS_ALL, overlaps=True)
    _assert_equals_host(g, h, "2 measured", s)
    after = g.cluster_move_counts()
    assert all(np.array_equal(before[k], after[k]) for k in ("moves", "empty", "size_sum"))
    h = _continue_host(h, 3, True, measure=False)
    s = g.tempering_run(3, 2, kinds=cl.KINDS_ALL, cluster_moves=True)
    assert set(s) == {"energy", "magnetization"}
    _assert_equals_host(g, h, "3 with moves, unmeasured", s)
    h = _continue_host(h, 2, True)
    _assert_equals_host(g, h, "2 with both", g.tempering_run(2, 2, kinds=cl.KINDS_ALL, **ON))
    assert (g.overlap_histograms()[0].sum(axis=3) == 7).all()
    counts = g.cluster_move_counts()
    assert ((counts["moves"] + counts["empty"])[:, :, 1:] == 8).all()


def test_groups_shard_over_handles():
    """Two groups in one handle = two handles of one group at the replica offsets 0 and K T."""
    cl = _cl()
    whole = _graph(RING_CASE)
    lo, hi = _graph(RING_CASE, 0, chains=2), _graph(RING_CASE, 8, chains=2)
    sw, sl, sh = (g.tempering_run(5, 2, kinds=cl.KINDS_ALL, **ON) for g in (whole, lo, hi))
    for key in ic.SERIES:
        assert np.array_equal(sw[key], np.concatenate([sl[key], sh[key]], axis=1)), key
    for key in ("moves", "empty", "size_sum"):
        assert np.array_equal(whole.cluster_move_counts()[key], np.concatenate([lo.cluster_move_counts()[key], hi.cluster_move_counts()[key]])), key
    assert np.array_equal(whole.state_ref(), np.concatenate([lo.state_ref(), hi.state_ref()]))
    _assert_equals_host(whole, _host_ring(5), "whole", sw)


def test_reset_zeroes_the_counts_and_the_series_is_optional():
    cl = _cl()
    want = _host_ring(6)
    a, b = _graph(RING_CASE), _graph(RING_CASE)
    assert a.tempering_run(6, 2, kinds=cl.KINDS_ALL, record=False, **ON) is None
    _assert_equals_host(a, want, "record = False")
    b.tempering_run(2, 2, kinds=cl.KINDS_ALL, **ON)
    assert b.cluster_move_counts()["moves"].any()
    b.reset_cluster_moves()
    counts = b.cluster_move_counts()
    assert not counts["moves"].any() and not counts["empty"].any() and not counts["size_sum"].any() and np.isnan(counts["mean_size"]).all()
    assert (b.overlap_histograms()[0].sum(axis=3) == 2).all()  # the histograms are not the counts
    b.tempering_run(4, 2, kinds=cl.KINDS_ALL, **ON)
    h2 = _host_ring(2)
    for key, name in zip(ic.COUNTS, ("moves", "empty", "size_sum")):
        assert np.array_equal(b.cluster_move_counts()[name], want[key] - h2[key]), key
    assert a.tempering_run(0, 2, **ON)["overlap"].shape == (0, 2, 1, 4)


def test_importance_sampling_rebuild_keeps_the_window_and_the_counts():
    cl = _cl()
    edges, biases = cc.CASES["ring33_positive"]
    c = ic._case((edges, biases), LADDER4, 2, 4, window=(1, 3))
    g = _graph(c)
    g.tempering_run(4, 2, kinds=cl.KINDS_ALL, **ON)
    counts, (hq, hl) = g.cluster_move_counts(), g.overlap_histograms()
    st, ep, tof = g.state_ref(), g.get_epoch(), g.temperature_of()
    g.enable_edge_importance_sampling(True)
    assert g._icm_window == (1, 3) and all(np.array_equal(g.cluster_move_counts()[k], counts[k]) for k in ("moves", "empty", "size_sum"))
    s = g.tempering_run(3, 2, kinds=cl.KINDS_ALL, **ON)
    want = cl.host_tempering_run(edges, biases, cc.SEED, st, ep, LADDER4, 3, 2, kinds=cl.KINDS_ALL, temp_of=tof, pt_step=4, flags=cl.CFG_EDGE_IMPORTANCE, ncopies=2,
                                 histograms=(hq, hl), cluster_moves=(1, 3), cluster_counts=(counts["moves"], counts["empty"], counts["size_sum"]))
    for key in ic.SERIES:
        assert np.array_equal(s[key], want[key]), key
    _counts_equal(g, want, "rebuilt")
    assert np.array_equal(g.state_ref(), want["states"]) and not want["cluster_moves"][:, :, 0].any() and not want["cluster_moves"][:, :, 3].any()


@pytest.mark.parametrize("name", list(cc.ENUM_SYSTEMS))
def test_device_cluster_moves_match_exact_enumeration(name):
    """The inputs of the CPU enumeration test on the device: 1024 groups of 2 copies, T = 4, 48 rounds of one only_basic_moves step with
    cluster moves at every temperature; Q^2 / N^2, QL and each copy's energy of the last round within 4.5 exact standard deviations over
    sqrt(1024) at every temperature.  The device equals the host entry bit for bit, so the CPU run predicts the outcome: at most 2.0
    sigma."""
    import isingmontecarlo_amd as im
    edges, biases = cc.ENUM_SYSTEMS[name]
    g = im.GraphState(edges, biases, cc.SEED, nreplicas=pc.ENUM_PT_CHAINS * 4)
    g.attach_tempering(pc.enum_pt_betas(name))
    g.attach_overlaps(2)
    g.attach_cluster_moves()
    s = g.tempering_run(pc.ENUM_PT_ROUNDS, 1, only_basic_moves=True, **ON)
    assert s["overlap"].shape == (pc.ENUM_PT_ROUNDS, oc.ENUM_GROUPS, 1, 4) and (g.get_epoch() == pc.ENUM_PT_ROUNDS).all()
    sigmas = ic.enum_icm_sigmas(name, s["overlap"][-1, :, 0, :], s["link_overlap"][-1, :, 0, :], s["energy"][-1])
    print(name, sigmas)
    assert max(max(x) for x in sigmas) <= cc.ENUM_SIGMAS, sigmas
    counts = g.cluster_move_counts()
    assert ((counts["moves"] + counts["empty"]) == pc.ENUM_PT_ROUNDS).all() and counts["moves"].sum() > 98304


def test_refusals_on_a_handle():
    """Cluster moves need overlaps (and tempering), and the other cluster calls need cluster moves, each with its own message; a refused
    attach leaves the handle as it was; attaching tempering or overlaps again detaches the cluster moves."""
    cl = _cl()
    import isingmontecarlo_amd as im
    g = im.GraphState(*RING, cc.SEED, nreplicas=16)
    lib, h = g._lib, g._h
    assert lib.isingmc_classical_icm_attach(h, 0, 0) == -1 and b"isingmc_classical_icm_attach: call isingmc_classical_pt_attach first" in lib.isingmc_classical_last_error(h)
    with pytest.raises(im.IsingMcError):
        g.attach_cluster_moves()
    g.attach_tempering(LADDER4)
    assert lib.isingmc_classical_icm_attach(h, 0, 0) == -1 and b"isingmc_classical_icm_attach: call isingmc_classical_overlap_attach first" in lib.isingmc_classical_last_error(h)
    with pytest.raises(im.IsingMcError):
        g.attach_cluster_moves()
    g.attach_overlaps(2)
    buf = np.zeros(2 * 1 * 4, dtype=np.uint64)
    p = im._ptr(buf, C.c_uint64)
    out4 = (C.c_uint32 * 4)()
    for rc in (lib.isingmc_classical_pt_run_icm(h, 1, 1, cl.NONE, cl.NONE, cl.NONE, 0, None, None, None, None, 1),
               lib.isingmc_classical_icm_counts(h, p, None, None), lib.isingmc_classical_icm_set_counts(h, p, p, p), lib.isingmc_classical_icm_reset(h),
               lib.isingmc_classical_icm_window(h, None, None), lib.isingmc_classical_icm_launch_plan(h, out4), lib.isingmc_classical_icm_force_waves(h, 1)):
        assert rc == -1 and b"isingmc_classical_icm_attach first" in lib.isingmc_classical_last_error(h)
    for call in (lambda: g.tempering_run(1, 1, cluster_moves=True), lambda: g.tempering_run(1, 1, **ON), g.cluster_move_counts, g.reset_cluster_moves, g.cluster_move_plan):
        with pytest.raises(im.IsingMcError) as ei:
            call()
        assert "cluster moves are not attached" in str(ei.value)
    for window, words in (((2, 2), "[2, 2) is empty or reversed"), ((3, 1), "[3, 1) is empty or reversed"), ((4, None), "[4, 4) is empty or reversed"),
                          ((0, 5), "t_last = 5 exceeds the 4 temperatures")):
        with pytest.raises(im.IsingMcError) as ei:
            g.attach_cluster_moves(*window)
        assert ei.value.code == -1 and words in str(ei.value)
    g.attach_cluster_moves(1, 3)
    assert g._icm_window == (1, 3)
    with pytest.raises(im.IsingMcError):
        g.attach_cluster_moves(3, 1)
    g.tempering_run(2, 1, cluster_moves=True)  # refused: the window [1, 3) stays attached
    counts = g.cluster_move_counts()
    assert ((counts["moves"] + counts["empty"])[:, :, 1:3] == 2).all() and not (counts["moves"] + counts["empty"])[:, :, [0, 3]].any()
    assert lib.isingmc_classical_icm_set_counts(h, None, p, p) == -1 and b"null buffer" in lib.isingmc_classical_last_error(h)
    g.attach_cluster_moves()  # attaching again zeroes the counts; t_last None is T
    assert g._icm_window == (0, 4) and not g.cluster_move_counts()["moves"].any()
    g.attach_overlaps(2)  # the groups may have changed: the cluster moves are detached
    with pytest.raises(im.IsingMcError):
        g.tempering_run(1, 1, cluster_moves=True)
    g.attach_cluster_moves()
    g.attach_tempering(LADDER4)
    with pytest.raises(im.IsingMcError):
        g.cluster_move_counts()
    g.attach_overlaps(2)
    g.attach_cluster_moves()
    g.attach_cluster_moves(cl.NONE, cl.NONE)  # detaches
    with pytest.raises(im.IsingMcError):
        g.cluster_move_counts()
    assert g.tempering_run(1, 1, overlaps=True)["overlap"].shape == (1, 2, 1, 4)  # the overlaps stay
