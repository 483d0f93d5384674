"""GPU parity of the imaginary-time folds (isingmc_itime_groups, isingmc_bond_counts): the device's integers against the sequential
fold of tests/_itime_reference.py over ORACLE replicas, bit for bit.  Every case first runs the same steps on both sides and checks
that the batch and the oracle hold the same strings (assert_same), so the reference never reads anything the code under test wrote."""
import ctypes as C

import numpy as np
import pytest

import _itime_reference as ref
import _lattices as lat
from test_gpu_parity import assert_same, make_pair

pytestmark = pytest.mark.gpu


def products(groups):
    """Flip bits that make a group the product of its +-1 spins (autocorrelations.product_groups)."""
    return np.array([1 - (len(np.atleast_1d(g)) & 1) for g in groups], dtype=np.uint8)


def check_folds(oracle, g, reps, bond_vars, groups, flips, what, fold_first=False):
    """The device folds and bond counts against the reference over the oracle replicas.  fold_first: call the device before anything
    exports a string, so that it meets the flip bytes the last cluster update left pending."""
    nb = g.num_bonds()
    if fold_first:
        got_all, got_occ = g.itime_groups(groups, flips)
        got_counts = g.bond_counts()
    assert_same(g, reps, what)
    if not fold_first:
        got_all, got_occ = g.itime_groups(groups, flips)
        got_counts = g.bond_counts()
    want_all, want_occ = ref.fold_replicas(reps, bond_vars, groups, flips)
    assert got_all.dtype == np.int64 and got_all.shape == want_all.shape == (len(reps), len(groups))
    assert np.array_equal(got_all, want_all), (what, np.argwhere(got_all != want_all)[:4].tolist())
    assert np.array_equal(got_occ, want_occ), (what, np.argwhere(got_occ != want_occ)[:4].tolist())
    assert got_counts.dtype == np.uint32 and got_counts.shape == (len(reps), nb)
    assert np.array_equal(got_counts, oracle.batch_bond_counts(oracle.pointers(reps), nb)), what
    assert np.array_equal(got_counts, np.stack([ref.bond_counts(rep.ops(), nb) for rep in reps])), what
    assert np.array_equal(got_counts.sum(axis=1), g.get_n()), what
    return got_all, got_occ


def snapshot(g):
    cut = g.get_cutoff()
    return dict(ops=[g.export_ops(r, int(cut[r])) for r in range(g.nreplicas)], state=g.state_ref(), n=g.get_n(), cutoff=cut,
                epoch=g.get_epoch(), acc=g.accumulators())


def same_snapshot(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a["ops"], b["ops"])) and all(np.array_equal(a[k], b[k]) for k in ("state", "n", "cutoff", "epoch", "acc"))


def lattice_groups(edges, nvars):
    """Every site, every edge with the flip bit of its bond observable (J < 0), and one group of all variables."""
    e, j = lat.split(edges)
    groups = [[v] for v in range(nvars)] + [list(ab) for ab in e] + [list(range(nvars))]
    flips = np.array([0] * nvars + [1 if x < 0 else 0 for x in j] + [1 - (nvars & 1)], dtype=np.uint8)
    return groups, flips


def test_one_variable_without_edges(oracle):
    """N = 1, one bond (the transverse field), a cutoff below 64: one row of slots, every wave but the first has no work."""
    g, m, reps = make_pair(oracle, [], 1.0, 0.0, 8, 64, 31, 3, nvars=1)
    g.run(20, 1.5)
    oracle.batch_timesteps(reps, 20, [1.5] * 3)
    assert (g.get_cutoff() < 64).all() and g.num_bonds() == 1
    got_all, _ = check_folds(oracle, g, reps, ref.tfim_bond_vars([], 1, 0.0), [[0], [0, 0]], np.array([0, 1], dtype=np.uint8), "N = 1")
    assert (got_all[:, 1] == g.get_cutoff().astype(np.int64)).all()  # a variable twice: parity 0, flipped: bit 1, the constant +1


def test_fresh_batch(oracle):
    """n = 0: sum_all = M x(0), sum_occ = 0, no bond counted."""
    edges = lat.two_d_ferro(4)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 37, 256, 5, 4)
    groups, flips = lattice_groups(edges, 16)
    got_all, got_occ = check_folds(oracle, g, reps, ref.tfim_bond_vars(lat.split(edges)[0], 16, 0.0), groups, flips, "fresh")
    assert (g.get_n() == 0).all() and (got_occ == 0).all() and (np.abs(got_all) == 37).all()
    st = g.state_ref().astype(np.int64)
    assert np.array_equal(got_all[:, :16], 37 * (2 * st - 1))


@pytest.mark.parametrize("cfg", ["default", "no_lds_tables", "fused_launch"])
def test_8x8_ferromagnet(oracle, cfg):
    """8x8 ferromagnet, a different beta per replica (different cutoffs); sites, bonds and the product of all 64 spins.  In the
    default geometry the cluster update defers its flips, and the fold is the first to need the strings."""
    import isingmontecarlo_amd as im
    edges = lat.two_d_ferro(8)
    R = 5
    betas = np.array([3.0, 2.0, 1.0, 2.5, 0.5])
    flags = {"default": 0, "no_lds_tables": im.CFG_NO_LDS_TABLES, "fused_launch": im.CFG_FUSED_LAUNCH}[cfg]
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 64, 1 << 13, 99, R, cfg_flags=flags)
    g.run(25, betas)
    oracle.batch_timesteps(reps, 25, betas)
    info = g.launch_info()
    if cfg == "default":  # trimmed diagonal kernel + dedicated cluster kernel: the flips of the last cluster update are still pending
        assert info["split_launches"] and info["fast_diagonal"] and info["lean_cluster"], info
    elif cfg == "fused_launch":
        assert not info["split_launches"], info
    else:
        assert not info["lds_edge_table"], info
    groups, flips = lattice_groups(edges, 64)
    bv = ref.tfim_bond_vars(lat.split(edges)[0], 64, 0.0)
    got_all, got_occ = check_folds(oracle, g, reps, bv, groups, flips, cfg, fold_first=True)
    assert len(set(g.get_cutoff().tolist())) > 1
    # the single-variable sums add up to the magnetisation fold, on the device and in the oracle
    s1, _, _ = g.itime_magnetization()
    assert np.array_equal(got_all[:, :64].sum(axis=1), s1) and [int(x) for x in s1] == [rep.itime_magnetization()[0] for rep in reps]
    # the calls left the batch as it was, and it goes on as the oracle does
    before = snapshot(g)
    g.itime_groups(groups, flips)
    g.bond_counts()
    assert same_snapshot(before, snapshot(g))
    g.run(10, betas)
    oracle.batch_timesteps(reps, 10, betas)
    check_folds(oracle, g, reps, bv, groups, flips, cfg + " + 10", fold_first=True)
    assert g.verify().all()


def test_one_variable_in_more_groups_than_lanes(oracle):
    """70-site ring: variable 0 paired with each of the other 69 (its list of groups is longer than a wave), and a group across two
    state words."""
    edges = lat.one_d_periodic(70, -1.0)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 70, 1 << 12, 707, 3)
    g.run(30, 2.0)
    oracle.batch_timesteps(reps, 30, [2.0] * 3)
    groups = [[0, v] for v in range(1, 70)] + [[31, 32]] + [[0]]
    check_folds(oracle, g, reps, ref.tfim_bond_vars(lat.split(edges)[0], 70, 0.0), groups, products(groups), "ring70", fold_first=True)


def test_3x3_with_a_longitudinal_field(oracle):
    """N = 9 (no multiple of 32), h = 0.3: longitudinal bonds behind the transverse ones."""
    edges = lat.two_d_ferro(3)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.3, 9, 1 << 11, 33, 4)
    g.run(40, 2.0)
    oracle.batch_timesteps(reps, 40, [2.0] * 4)
    assert g.num_bonds() == 18 + 9 + 9
    groups, flips = lattice_groups(edges, 9)
    check_folds(oracle, g, reps, ref.tfim_bond_vars(lat.split(edges)[0], 9, 0.3), groups, flips, "3x3 h", fold_first=True)
    assert g.bond_counts()[:, 27:].sum() > 0


def test_generic_interactions_with_two_variable_flips(oracle):
    """The XXZ ring of test_generic_interactions_match_oracle: hopping ops flip both of their variables; groups hold one leg, and
    both legs, of such ops."""
    import isingmontecarlo_amd as im
    n, R, beta, cutoff, cap, seed = 7, 5, 1.5, 8, 1 << 12, 909
    ints = lat.xxz_ring_interactions(n)
    g = im.Qmc.from_interactions(n, ints, cutoff, seed, nreplicas=R, capacity=cap, do_loop_updates=True, do_cluster_updates=False)
    m = oracle.Model.generic(n, ints)
    reps = [oracle.Replica(m, cap, cutoff, seed, r, None) for r in range(R)]
    flags = im.FLAG_NO_CLUSTER | im.FLAG_LOOP
    g.run(60, beta, sampling_freq=2, flags=flags)
    for rep in reps:
        rep.timesteps(60, beta, 2, flags)
    groups = [[i] for i in range(n)] + [[i, (i + 1) % n] for i in range(n)] + [[0, 1, 2], list(range(n))]
    check_folds(oracle, g, reps, ref.generic_bond_vars(ints), groups, products(groups), "xxz")
    assert sum(1 for rep in reps for w in rep.ops() if w and ((int(w) ^ (int(w) >> 2)) & 3) == 3) > 0


def test_per_replica_couplings(oracle):
    """One disorder realisation per replica (per-replica bond tables): the bonds' variables are the same in every table."""
    import isingmontecarlo_amd as im
    l, R = 4, 4
    edges = lat.cubic_periodic(l)
    J = np.random.default_rng(20260).choice([-1.0, 1.0], size=(R, len(edges)))
    gamma, h, beta, cutoff, cap, seed = 1.0, 0.1, 2.0, 64, 1 << 13, 4096
    g = im.QmcIsingGraph(edges, gamma, h, cutoff, seed, nreplicas=R, capacity=cap, couplings=J)
    e = [ab for ab, _ in edges]
    reps = [oracle.Replica(oracle.Model(g.nvars, e, list(J[r]), gamma, h), cap, cutoff, seed, r, None) for r in range(R)]
    g.run(15, beta)
    oracle.batch_timesteps(reps, 15, [beta] * R)
    groups = [[v] for v in range(g.nvars)] + [list(ab) for ab in e[:40]]
    check_folds(oracle, g, reps, ref.tfim_bond_vars(e, g.nvars, h), groups, products(groups), "per-replica J", fold_first=True)


def test_native_tempering_rows_are_replicas(oracle):
    """A 4x4 tempering batch after swaps: row r is replica r, whatever temperature slot it holds now."""
    import _pt_cases as pc
    import test_gpu_tempering_edges as te
    c = pc.case("ferro4x4_itime", ("ferro2d", 4), np.linspace(0.8, 1.2, 4), 2, 9601, 2048, 16, 6, 2)
    pt_ref = pc.check_preconditions(c)
    g, tc = te.build(c)
    te.drive(tc, c, te.DEVICE, c["steps"])
    te.compare(g, tc, c, pt_ref, "4x4 tempering")
    assert pt_ref.swaps > 0
    slot_of = tc.slot_of
    assert not np.array_equal(slot_of, np.arange(g.nreplicas))  # labels did move
    reps = [pt_ref.by_slot[int(s) % c["K"]][int(s) // c["K"]] for s in slot_of]  # the reference's replica behind every batch row
    edges = pc.edges_of(c)
    groups, flips = lattice_groups(edges, 16)
    check_folds(oracle, g, reps, ref.tfim_bond_vars(lat.split(edges)[0], 16, 0.0), groups, flips, "4x4 tempering")


def test_long_string(oracle):
    """More than 4100 slots: every wave's range spans several rows of 64 slots, with 16 waves and with 4."""
    edges = lat.two_d_ferro(8)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 4200, 1 << 13, 1234, 2)
    g.run(30, 6.0)
    oracle.batch_timesteps(reps, 30, [6.0] * 2)
    assert (g.get_cutoff() > 4100).all() and (g.get_n() > 1000).all()
    groups, flips = lattice_groups(edges, 64)
    check_folds(oracle, g, reps, ref.tfim_bond_vars(lat.split(edges)[0], 64, 0.0), groups, flips, "long", fold_first=True)


def test_histogram_beyond_lds(oracle):
    """64x64 lattice, every site a group: the variable lists stay in LDS, the 12288-bond histogram does not (global atomics)."""
    edges = lat.two_d_ferro(64)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 4096, 1 << 14, 640, 2)
    g.run(6, 0.5)
    oracle.batch_timesteps(reps, 6, [0.5] * 2)
    groups = [[v] for v in range(4096)]
    check_folds(oracle, g, reps, ref.tfim_bond_vars(lat.split(edges)[0], 4096, 0.0), groups, None, "64x64", fold_first=True)


@pytest.mark.parametrize("ngroups", [300, 6000])
def test_32768_variables(oracle, ngroups):
    """A chain of 32768 sites: neither the variable lists nor the histogram fit in LDS; with 6000 groups not even 16 waves' bit
    arrays do, and the kernel runs with 4."""
    n = 32768
    edges = lat.chain(n, lat.uni_chain)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 4096, 1 << 16, 3276, 2)
    g.run(6, 0.25)
    oracle.batch_timesteps(reps, 6, [0.25] * 2)
    rng = np.random.default_rng(ngroups)
    some = np.sort(rng.choice(n, size=ngroups // 2, replace=False))  # variables all over the state words
    groups = [[int(v)] for v in some] + [[int(v), int((v + 1) % n)] for v in some[:ngroups - len(some)]]
    assert len(groups) == ngroups
    check_folds(oracle, g, reps, ref.tfim_bond_vars(lat.split(edges)[0], n, 0.0), groups, products(groups), f"chain {n}", fold_first=True)


def test_bad_arguments_and_the_group_cap(oracle):
    """EINVAL / ENOTIMPL with a message, and the batch goes on working."""
    import isingmontecarlo_amd as im
    edges = lat.two_d_ferro(4)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 16, 1 << 10, 77, 2)
    g.run(10, 1.0)
    oracle.batch_timesteps(reps, 10, [1.0] * 2)
    lib, h = g._lib, g._h
    u32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32))
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    out = np.zeros((2, 4), dtype=np.int64)
    po = out.ctypes.data_as(C.POINTER(C.c_int64))
    start, vs = u32([0, 1, 3]), u32([0, 1, 2])
    assert lib.isingmc_itime_groups(None, 2, p32(start), p32(vs), None, po, po) == -1
    assert lib.isingmc_bond_counts(None, None) == -1
    bad = [("ngroups == 0", 0, start, vs), ("an empty group", 2, u32([0, 1, 1]), vs), ("a variable >= N", 2, start, u32([0, 1, 16])),
           ("group_start[0] != 0", 2, u32([1, 2, 3]), vs)]
    for what, ng, s, v in bad:
        assert lib.isingmc_itime_groups(h, ng, p32(s), p32(v), None, po, po) == -1, what
        assert b"itime_groups" in lib.isingmc_last_error(h), what
    assert lib.isingmc_itime_groups(h, 2, p32(start), p32(vs), None, None, None) == -1
    assert lib.isingmc_bond_counts(h, None) == -1
    # more groups than LDS holds sums for: refused before anything runs, with the cap in the message
    many = [[v % 16] for v in range(12000)]
    with pytest.raises(im.IsingMcError) as ei:
        g.itime_groups(many)
    assert ei.value.code == -5 and "at most" in str(ei.value)
    cap = int(str(ei.value).split("at most ")[1].split()[0])
    assert 3072 <= cap < 12000
    # either output alone
    groups, flips = lattice_groups(edges, 16)
    want_all, want_occ = ref.fold_replicas(reps, ref.tfim_bond_vars(lat.split(edges)[0], 16, 0.0), groups, flips)
    ng, s, v = g._groups(groups)
    one = np.zeros((2, ng), dtype=np.int64)
    p1 = one.ctypes.data_as(C.POINTER(C.c_int64))
    pf = flips.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.isingmc_itime_groups(h, ng, p32(s), p32(v), pf, p1, None) == 0 and np.array_equal(one, want_all)
    assert lib.isingmc_itime_groups(h, ng, p32(s), p32(v), pf, None, p1) == 0 and np.array_equal(one, want_occ)
    # ... and the batch is as usable as before
    check_folds(oracle, g, reps, ref.tfim_bond_vars(lat.split(edges)[0], 16, 0.0), groups, flips, "after the refusals")
    g.run(5, 1.0)
    oracle.batch_timesteps(reps, 5, [1.0] * 2)
    assert_same(g, reps, "after the refusals + 5")


def test_estimator_helpers_on_the_device_sums(oracle):
    """itime_average / itime_susceptibility are the documented functions of the device's integers."""
    edges = lat.one_d_periodic(8, -1.0)
    R = 3
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 8, 1 << 10, 11, R)
    betas = np.array([1.0, 2.0, 0.5])
    g.run(20, betas)
    groups = [[0], [0, 4]]
    flips = products(groups)
    sa, so = g.itime_groups(groups, flips)
    M, n = g.get_cutoff().astype(np.float64)[:, None], g.get_n().astype(np.float64)[:, None]
    assert np.allclose(g.itime_average(groups, flips), sa / M, rtol=0, atol=1e-15)
    assert np.allclose(g.itime_susceptibility(groups, betas, flips), betas[:, None] * (so * so + n) / (n * (n + 1)), rtol=1e-15)
    assert np.allclose(g.itime_susceptibility(groups, betas, flips, slots="all"), betas[:, None] * (sa * sa + M) / (M * (M + 1)), rtol=1e-15)
    avg, chi_occ, chi_all = g.timesteps_measure_itime(6, betas, groups, sampling_freq=3, flips=flips)
    assert avg.shape == chi_occ.shape == chi_all.shape == (R, 2) and (np.abs(avg) <= 1).all()
    assert (chi_occ > 0).all() and (chi_occ <= betas[:, None] + 1e-12).all() and (chi_all > 0).all()
    oracle.batch_timesteps(reps, 26, betas)
    assert_same(g, reps, "measure_itime ran 6 plain timesteps")
