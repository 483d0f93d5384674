"""Per-replica couplings (ISINGMC_CLASSICAL_CFG_PER_REPLICA_J) without a device.  The oracle is the shared-coupling path: a run is a
function of (seed, global replica, epoch), so replica r of a per-replica batch must equal, bit for bit, a one-replica run with
J = couplings[r] at replica_offset + r: through isingmc_classical_host_steps as it was before the flag, and through the numpy
restatement.  Also: the table formats, the launch plans by arithmetic, the argument checks and tempering over C realisations x T
temperatures."""
import numpy as np
import pytest

import _classical_cases as cc
import _classical_disorder_cases as dc
import _classical_pt_cases as pc
import _classical_reference as CR


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


def _assert_chains(got, want, what):
    assert len(got) == len(want)
    for run, (g, w) in zip(cc.RUNS, zip(got, want)):
        assert np.array_equal(g[0], w[0]), (what, run, "states")
        assert np.array_equal(g[1], w[1]), (what, run, g[1].tolist(), w[1].tolist())
        assert np.array_equal(g[2], w[2]), (what, run, "epochs")


# ---- parity ----
@pytest.mark.parametrize("name", dc.PARITY + dc.IMPORTANCE)
def test_host_rows_are_the_shared_coupling_runs(oracle, name):
    """Every run of cc.RUNS at R = 5, replica_offset = cc.OFFSET: states, counters and epochs of the per-replica host call against the
    five one-replica shared-coupling calls and against the restatement."""
    got = dc.host_per_replica_chain(name)
    _assert_chains(got, dc.oracle_chain(name), (name, "host rows"))
    _assert_chains(got, dc.restatement_chain(name), (name, "restatement"))
    assert got[-1][1][:, CR.C_WORM].sum() > 0 and got[-1][1][:, CR.C_SPIN_ACC].sum() > 0


def test_realisations_differ_where_the_tests_need_it():
    """Conditions on the inputs: every case but one_edge has five different rows (one_edge: both signs), the duplicate edge's copies
    differ in some replica and not in the same way everywhere, ring65 has an odd number of code bytes modulo 4, and one case keeps a
    zero coupling in some rows only."""
    for name in dc.PARITY + dc.IMPORTANCE:
        cj = dc.realisations(name)
        assert len({row.tobytes() for row in cj}) == (2 if name == "one_edge" else dc.R), name
    dup = dc.realisations("duplicate_edge")
    assert len({(row[0], row[2], row[4]) for row in dup}) > 1 and any(len({row[0], row[2], row[4]}) > 1 for row in dup)
    assert (2 * len(cc.CASES["ring65"][0])) % 4 == 2 and 2 * len(cc.CASES["one_edge"][0]) == 2
    zeros = (dc.realisations(dc.ZERO_ROWS_CASE) == 0.0).any(axis=1)
    assert zeros.any() and not zeros.all()


def test_summation_order(oracle):
    """Couplings and biases that are not dyadic: the energy differences depend on the order of the additions.  300 distinct values:
    the doubles format."""
    e, b, cj, betas, _ = dc.case("order300")
    assert _cl().plan(e, b, couplings=cj)["coupling_format"] == 2
    got = dc.host_per_replica_chain("order300")
    _assert_chains(got, dc.oracle_chain("order300"), "order300 host rows")
    _assert_chains(got, dc.restatement_chain("order300"), "order300 restatement")


@pytest.mark.parametrize("distinct,fmt", [(256, 1), (257, 2)])
def test_dictionary_boundary(oracle, distinct, fmt):
    """Each replica alone has at most 200 distinct couplings; the batch has exactly 256 (the dictionary's last size) or 257 (doubles)."""
    name = f"dict{distinct}"
    e, b, cj, betas, _ = dc.case(name)
    p = _cl().plan(e, b, couplings=cj)
    assert p["coupling_format"] == fmt and p["compact_couplings"] == (fmt == 1)
    assert p["tables"] == (1 | 2 | 8 | 16 | 64) | (4 if fmt == 1 else 0) and p["in_lds"] == (p["tables"] if fmt == 1 else p["tables"] & ~64)
    for r in range(len(cj)):  # every replica alone would still be a dictionary
        assert _cl().plan(dc.with_couplings(e, cj[r]), b)["compact_couplings"]
    got = dc.host_per_replica_chain(name)
    _assert_chains(got, dc.oracle_chain(name), name + " host rows")
    _assert_chains(got, dc.restatement_chain(name), name + " restatement")


# ---- sensitivity: on the host alone ----
@pytest.mark.parametrize("name", ["k8", "ring65", "duplicate_edge", "k8_positive"])
def test_parity_tells_wrong_table_indexing(oracle, name):
    """What a wrong index would read gives other results: the rows of `couplings` rotated by one replica (tables indexed by the wrong
    replica) and every row rotated by one entry (a wrong entry index)."""
    e, b, cj, betas, imp = dc.case(name)
    right = dc.host_per_replica_chain(name)
    for wrong in (dc.rotate_rows(cj), dc.rotate_entries(e, cj)):
        assert not np.array_equal(wrong, cj)
        got = dc.host_chain(e, b, wrong, betas, cc.RUNS, imp)
        assert not np.array_equal(got[-1][0], right[-1][0]) or not np.array_equal(got[-1][1], right[-1][1]), name
        # ... in every replica whose row changed, by the end of the runs
    rot = dc.host_chain(e, b, dc.rotate_rows(cj), betas, cc.RUNS, imp)
    differs = [not np.array_equal(rot[-1][0][r], right[-1][0][r]) or not np.array_equal(rot[-1][1][r], right[-1][1][r]) for r in range(dc.R)]
    assert sum(differs) >= dc.R - 1, (name, differs)


# ---- errors ----
def _error(fn, *a, **kw):
    import isingmontecarlo_amd as im
    with pytest.raises(im.IsingMcError) as ei:
        fn(*a, **kw)
    return str(ei.value)


def test_argument_checks(oracle):
    cl = _cl()
    e, b = cc.CASES["k8_positive"]
    cj = dc.realisations("k8_positive")
    st = dc.initial_states(dc.R, 8)
    run = lambda couplings, flags=0, states=st: cl.host_steps(e, b, cc.SEED, states, 0, 1, 1.0, couplings=couplings, flags=flags)
    run(cj)
    assert "shape" in _error(run, cj[:4]) and "shape" in _error(run, cj[:, :-1]) and "shape" in _error(run, cj[0])
    assert "shape" in _error(cl.plan, e, b, couplings=cj[:, :-1])
    bad = cj.copy(); bad[2, 5] = np.nan
    msg = _error(run, bad)
    assert "finite" in msg and "replica 2" in msg
    bad = cj.copy(); bad[3, 0] = np.inf
    assert "replica 3" in _error(cl.plan, e, b, couplings=bad)
    neg = cj.copy(); neg[4, 1] = 0.0
    run(neg)  # fine without importance sampling
    msg = _error(run, neg, cl.CFG_EDGE_IMPORTANCE)
    assert "J > 0" in msg and "replica 4" in msg
    assert "unknown flag" in _error(run, cj, 64)
    assert "unknown flag" in _error(cl.host_steps, e, b, cc.SEED, st, 0, 1, 1.0, flags=64)
    assert "couplings" in _error(cl.host_steps, e, b, cc.SEED, st, 0, 1, 1.0, flags=cl.CFG_PER_REPLICA_J)  # the flag without the rows
    assert cl.CFG_PER_REPLICA_J == 8


def test_tempering_needs_one_realisation_per_chain(oracle):
    """Rows that differ inside a chain: EINVAL naming the chain.  Equal inside each chain, different between chains: accepted."""
    cl = _cl()
    e, b, betas, chains, cj = dc.pt_case("ring65_T3")
    t = len(betas)
    run = lambda couplings: pc.host_run(cl, e, b, betas, chains, 1, 1, replica_offset=t, couplings=couplings)
    run(cj)
    assert len({row.tobytes() for row in cj}) == chains
    bad = cj.copy(); bad[2 * t + 1, 4] = -bad[2 * t + 1, 4]
    msg = _error(run, bad)
    assert "chain 2" in msg and "differ" in msg
    bad = cj.copy(); bad[1, 0] = 0.0 if bad[1, 0] != 0.0 else 1.0
    assert "chain 0" in _error(run, bad)
    neg0 = cj.copy(); neg0[:t, 3] = 0.0; neg0[1, 3] = -0.0  # equal as numbers, not as bits
    assert "chain 0" in _error(run, neg0)
    # the doubles format compares bytes as well
    e3, b3, c3 = dc.order_case()[:3]
    rows = np.repeat(c3[:2], 2, axis=0)
    pc.host_run(cl, e3, b3, [0.3, 4.0], 2, 1, 1, replica_offset=2, couplings=rows)
    rows[3, 299] *= -1.0
    assert "chain 1" in _error(pc.host_run, cl, e3, b3, [0.3, 4.0], 2, 1, 1, replica_offset=2, couplings=rows)


# ---- plans ----
@pytest.mark.parametrize("name", list(dc.PLAN_CASES))
def test_plans(oracle, name):
    """The launch of +-J realisations on the 48 x 48, 64 x 64 and 72 x 72 lattices at 160 KB, by arithmetic that does not call the carve."""
    c = dc.PLAN_CASES[name]
    e, b, cj = dc.lattice_pmj(c["l"])
    got = _cl().plan(e, b, lds_bytes=4 * dc.LDS_WORDS, flags=c["flags"], couplings=cj)
    for k, v in c["plan"].items():
        assert got[k] == v, (name, k, got)
    assert got["packed_edges"]
    codes = bool(got["in_lds"] & 64)
    assert got["wave_words"] == dc.wave_words(c["l"], codes)
    if not c["flags"] & _cl().CFG_GLOBAL_TABLES:
        assert got["lds_words"] == dc.carve_words(c["l"], got["waves"], codes, bool(got["in_lds"] & 16)) <= dc.LDS_WORDS


def test_plan_rule_by_arithmetic():
    """Why the three lattices plan as they do: the most waves of 4, 2, 1 with everything in LDS."""
    assert dc.carve_words(48, 4, True) == 27942 <= dc.LDS_WORDS
    assert dc.carve_words(64, 4, True) == 49670 > dc.LDS_WORDS >= dc.carve_words(64, 2, True) == 39174
    assert dc.carve_words(64, 4, False) == 33286  # the shared-coupling launch of this lattice
    assert dc.carve_words(72, 1, True) == 42936 > dc.LDS_WORDS >= dc.carve_words(72, 2, False) == 39210
    assert dc.carve_words(72, 4, False, edges_in_lds=False) == 31758 and dc.carve_words(72, 4, False) > dc.LDS_WORDS


def test_shared_plans_are_unchanged(oracle):
    """A shared-coupling plan's eight slots: an existing layout case against the values committed with it, format 0."""
    cl = _cl()
    for name in ("lat48_noncompact", "lat64_bias_importance", "hightail145632"):
        c = cc.LAYOUT_CASES[name]
        got = cl.plan(c["edges"], c["biases"], flags=cl.CFG_EDGE_IMPORTANCE if c["importance"] else 0)
        for k, v in c["plan"].items():
            assert got[k] == v, (name, k, got)
        assert got["coupling_format"] == 0 and not got["tables"] & 64
    c = cc.LAYOUT_CASES["lat48_noncompact"]
    got = cl.plan(c["edges"], c["biases"])
    assert (got["waves"], got["in_lds"], got["lds_words"], got["wave_words"], got["tables"], got["compact_couplings"], got["packed_edges"],
            got["coupling_format"]) == (2, 31, 40466, 648, 31, False, True, 0)
    # R equal rows are still a per-replica batch: same results as the shared one (parity), another table format
    e, b = cc.CASES["k8"]
    assert cl.plan(e, b, couplings=np.tile([j for _, j in e], (3, 1)))["coupling_format"] == 1


# ---- tempering on the host ----
@pytest.mark.parametrize("name", list(dc.PT_CASES))
def test_host_tempering_chains_are_the_shared_coupling_runs(oracle, name):
    """6 rounds of 2 KINDS_ALL steps over C realisations x T temperatures: chain c equals host_tempering_run on realisation c alone
    (R = T, replica_offset moved on by c T), on every output."""
    edges, biases, betas, chains, cj = dc.pt_case(name)
    t = len(betas)
    got = dc.pt_host_reference(name)
    assert got["pt_step"] == pc.PT_ROUNDS and got["accepts"].sum() > 0
    for c in range(chains):
        want = dc.pt_oracle_chain(name, c)
        assert want["pt_step"] == pc.PT_ROUNDS
        for k in ("states", "epochs", "counters", "temp_of"):
            assert np.array_equal(got[k][c * t:(c + 1) * t], want[k]), (name, c, k)
        for k in ("attempts", "accepts"):
            assert np.array_equal(got[k][c], want[k][0]), (name, c, k)
        for k in ("energy", "magnetization"):
            assert np.array_equal(got[k][:, c], want[k][:, 0]), (name, c, k)
    # the chains are different runs
    assert not np.array_equal(got["energy"][:, 0], got["energy"][:, 1])
