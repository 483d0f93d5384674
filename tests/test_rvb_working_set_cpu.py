"""The RVB working-set cases of _rvb_cases.py, checked in the oracle alone: the statistics call changes nothing, every case reaches
the branch it is there for at least as often as it must, passing cases stay inside every large cap, loud cases name the first
(replica, sweep, attempt) past a cap and the cap, and the caps that cannot bind do not.  The census printed here (pytest -s) is the
table of DESIGN.md, "RVB working set"."""
import os

import numpy as np
import pytest

import _rvb_cases as rc
from test_gpu_parity import RVB_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["single_bond_long", "villain4", "ferro8x8_long"])
def test_statistics_leave_the_sweep_as_it_is(oracle, name):
    """ora_rvb_update_stats against ora_rvb_update on twins: successes, op words, state, n, cutoff, epoch and accumulators agree after
    every sweep; the rows add up (accepted attempts = successes, csize = the draw that cluster_size() repeats, ncl <= csize)."""
    import _lattices as lat
    _, edges, gamma, h, beta, cutoff = next(c for c in RVB_CASES if c[0] == name)
    e, j = lat.split(edges)
    nvars = 1 + max(max(ab) for ab in e)
    m = oracle.Model(nvars, e, j, gamma, h)
    seed = 1357
    for r in range(3):
        a, b = (oracle.Replica(m, 8192, cutoff, seed, r, None) for _ in range(2))
        for it in range(6):
            rc.oracle_step([a, b], ("diag",), beta)
            epoch = a.epoch
            upd = (nvars + 1) // 2
            succ, st = a.rvb_update(upd, stats=True)
            assert succ == b.rvb_update(upd), (name, r, it)
            assert st.shape == (upd, len(oracle.RVB_STATS))
            col = {k: st[:, i] for i, k in enumerate(oracle.RVB_STATS)}
            assert int(col["accept"].sum()) == succ and set(np.unique(col["accept"])) <= {0, 1}
            assert [int(x) for x in col["csize"]] == [rc.cluster_size(oracle, seed, epoch, r, at) for at in range(upd)]
            assert (col["ncl"] <= col["csize"]).all() and (col["ncl"] >= 1).all()
            assert (col["nsub"] <= col["ncand"]).all() and (col["ncand"] <= col["ncl"] + col["bf"] + col["bn"]).all()
            assert (col["bonds_mut"][col["accept"] == 0] == 0).all()
            rc.oracle_step([a, b], ("cluster",), beta)
            rc.oracle_step([a, b], ("free",), beta)
            assert a.n == b.n and a.cutoff == b.cutoff and a.epoch == b.epoch, (name, r, it)
            assert np.array_equal(a.ops(), b.ops()) and np.array_equal(a.state(), b.state()), (name, r, it)
            assert np.array_equal(a.accumulators(), b.accumulators())


def test_the_lattice_seed_is_the_first_with_a_large_draw(oracle):
    """find_seed repeats the search: 4 replicas x 8 attempts at epoch 1 (one diagonal step behind the start), a draw of at least
    SSE_RVB_SLOT_CL + 1; the draw belongs to an attempt of the case's first sweep, and that attempt's cluster gets all its members."""
    want = rc.SMALL["cl"] + 1
    assert rc.find_seed(oracle, 4, 8, 1, at_least=want) == rc.LATTICE_SEED
    case = rc.BY_NAME["ferro8x8_csize18"]
    assert case["seed"] == rc.LATTICE_SEED and case["R"] == 4
    _, rows = rc.analyse(oracle, "ferro8x8_csize18")["sweeps"][0]
    hits = [(r, a) for r in range(4) for a in range(8) if rc.cluster_size(oracle, rc.LATTICE_SEED, 1, r, a) >= want]
    assert hits
    for r, a in hits:
        assert rows[r][a]["csize"] == rc.cluster_size(oracle, rc.LATTICE_SEED, 1, r, a) and rows[r][a]["ncl"] >= want, (r, a, rows[r][a])


@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES])
def test_case_reaches_its_branch(oracle, name):
    case, cs = rc.BY_NAME[name], rc.census(oracle, name)
    print("\n" + rc.census_row(oracle, name))
    assert cs["branch"] >= case["at_least"], (name, case["branch"], cs)
    if case["loud"] is None:
        assert cs["first_bad"] is None, (name, cs)  # (analyse looks at every attempt of every sweep: inside every large cap)
        assert cs["ncl"] <= rc.LARGE["cl"] and cs["bf"] <= rc.LARGE["set"] and cs["bn"] <= rc.LARGE["set"] and cs["bonds"] <= rc.BONDCAP
    else:
        assert cs["first_bad"] is not None, (name, cs)
        replica, sweep, attempt, cap = cs["first_bad"]
        assert cap == case["loud"], (name, cs)
        assert (replica, sweep, attempt) == rc.STOPS_AT[name], (name, cs)
        bad = rc.analyse(oracle, name)["bad"]
        assert all(c == case["loud"] for _, c in bad.values()) and 0 < len(bad) <= case["R"]


def test_loud_cases_have_sweeps_before_and_replicas_beside_the_stop(oracle):
    """What the device test needs from them: whole sweeps before the one that stops, and (where the sweep is the case's own choice)
    replicas that get through it."""
    for name in rc.LOUD:
        an, case = rc.analyse(oracle, name), rc.BY_NAME[name]
        assert an["first_bad"][1] >= 1, name
        if name != "star70_bf":
            assert len(an["bad"]) < case["R"], name


def test_caps_that_cannot_bind(oracle):
    """Of the four caps of a growth area only the members (small area) and the two boundary sets decide: there are at most ncl + 1
    windows and both areas hold more than cap_cl + 1; the sub-variable candidates are ncl + bf.n + bn.n <= cap_cl + 2 cap_set <=
    cap_sub; a cluster has at most 65 members, fewer than SSE_RVB_MAXCL."""
    for area in (rc.SMALL, rc.LARGE):
        assert area["win"] > area["cl"] and area["sub"] >= area["cl"] + 2 * area["set"], area
    assert 65 < rc.LARGE["cl"]
    assert rc.AHEAD <= rc.STRIDE and 8 + 4 * rc.SMALL["cl"] + 2 * rc.SMALL["sub"] + 2 * rc.SMALL["win"] <= rc.AHEAD
    seen = 0
    for name in rc.BY_NAME:
        for *_, row in rc.all_rows(rc.analyse(oracle, name)):
            assert row["nwin"] <= row["ncl"] + 1 and row["csize"] <= 65 and row["ncl"] <= row["csize"], (name, row)
            assert row["ncand"] <= row["ncl"] + row["bf"] + row["bn"], (name, row)
            assert row["ntog"] <= 2 * row["ncl"] and row["nsub"] <= row["ncand"], (name, row)
            seen += 1
    assert seen > 5000


def test_the_edge_list_cases_straddle_the_fetched_ahead_part(oracle):
    """record_words on both sides of SSE_RVB_PROD_AHEAD: every record of the one complete graph lists its edges, none of the next
    one does, and neither is fetched whole."""
    full = {}
    for name in ("k24_edges_listed", "k25_edges_not_listed"):
        rows = [row for *_, row in rc.all_rows(rc.analyse(oracle, name))]
        full[name] = [rc.record_words(row["nsub"], row["ntog"], row["nwin"], row["nadj"]) for row in rows]
        assert not any(rc.whole_record(row) for row in rows)
    print("\nrecord words with edges:", {k: (min(f for _, f in v), max(f for _, f in v)) for k, v in full.items()}, "fetched ahead:", rc.AHEAD)
    assert max(f for _, f in full["k24_edges_listed"]) <= rc.AHEAD < min(f for _, f in full["k25_edges_not_listed"])
    assert max(l for l, _ in full["k25_edges_not_listed"]) <= rc.AHEAD
    assert rc.record_words(3, 2, 1, 10) == (8 + 4 + 6 + 2, 8 + 4 + 6 + 2 + 4 + 10)


def test_regrown_attempts_in_every_partial_group(oracle):
    """star130_group_tails: sweeps of 1, 63, 64, 65 and 129 attempts; wherever the last group of 64 is a partial one, its last attempt
    is grown again in some replica (the regrow scan has to look at the tail), and the sweep of 64 has no tail."""
    an = rc.analyse(oracle, "star130_group_tails")
    assert tuple(len(rows[0]) for _, rows in an["sweeps"]) == rc.TAIL_ATTEMPTS
    for _, rows in an["sweeps"]:
        u = len(rows[0])
        if u % rc.GROUP:
            assert any(rc.regrown(rr[u - 1]) for rr in rows), u
        assert any(rc.regrown(rr[a]) for rr in rows for a in range(u))


def test_the_design_document_holds_the_census(oracle):
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    for name in rc.BY_NAME:
        assert rc.census_row(oracle, name) in text, rc.census_row(oracle, name)
