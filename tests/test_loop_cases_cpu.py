"""The directed-loop cases (tests/_loop_cases.py) on the CPU oracle alone: the traced loop update is the plain one, its rows
describe the walk, every case reaches every feature it claims at least MIN_COUNT times, the placed strings are valid before and
after the walks, and between them the cases claim every feature on every kernel that owes it."""
from collections import Counter

import numpy as np
import pytest

import _lattices as lat
import _loop_cases as lc


def twin_models(oracle):
    e, j = lat.split(lat.one_d_periodic(6, -1.0))
    return [("xxz7", oracle.Model.generic(7, lat.xxz_ring_interactions(7)), 1.5, 3), ("ferro6_long", oracle.Model(6, e, j, 1.0, 0.3), 2.0, 1)]


def same(a, b):
    return (a.n == b.n and a.cutoff == b.cutoff and a.epoch == b.epoch and np.array_equal(a.ops(), b.ops()) and
            np.array_equal(a.state(), b.state()) and np.array_equal(a.accumulators(), b.accumulators()))


@pytest.mark.parametrize("cap_rows", [1 << 12, 3, 0])
def test_traced_call_equals_plain_call(oracle, cap_rows):
    """Twin replicas: one takes the traced call, one the plain call; strings, states, epochs and accumulators (acc[4] among them)
    stay identical loop after loop, also with a buffer shorter than the walks (the rows stop, the walk does not)."""
    longest = 0
    for name, m, beta, flags in twin_models(oracle):
        a, b = (oracle.Replica(m, 1 << 12, 8, 909, 2, None) for _ in range(2))
        for rep in (a, b):
            rep.timesteps(20, beta, 1, flags)
        assert same(a, b)
        for it in range(40):
            length, rows, start = a.loop_update_trace(cap_rows)
            assert length == b.loop_update(), (name, it)
            assert same(a, b), (name, it)
            assert len(rows) == min(length, cap_rows)
            if len(rows):
                assert rows[0, lc.P] == start[1]
            longest = max(longest, length)
        assert a.accumulators()[4] == b.accumulators()[4] > 0
        assert a.verify() and b.verify()
    assert longest > 3  # the short buffer was shorter than a walk


def test_trace_rows_describe_the_walk(oracle):
    """Every row follows from the one before: the next slot lies at the recorded distance in the recorded direction, wrapped says
    whether p = 0 was passed, the entry leg is the far side of the exit leg, the start slot is the nth occupied one, and only the
    last row is closed."""
    m = oracle.Model.generic(7, lat.xxz_ring_interactions(7))
    rep = oracle.Replica(m, 1 << 12, 8, 31, 0, None)
    rep.timesteps(30, 1.5, 1, 3)
    rows_seen = 0
    for it in range(30):
        before, M = rep.ops(), rep.cutoff
        length, t, (nth, p0) = rep.loop_update_trace()
        t = t.astype(np.int64)
        assert length == len(t) and np.flatnonzero(before)[nth] == p0 == t[0, lc.P]
        assert (t[:-1, lc.CLOSED] == 0).all() and t[-1, lc.CLOSED] in (1, 2)
        for a, b in zip(t[:-1], t[1:]):
            q = a[lc.P] + a[lc.DIST] if a[lc.FORWARD] else a[lc.P] - a[lc.DIST]
            assert b[lc.P] == q % M and bool(a[lc.WRAPPED]) == (q >= M or q < 0)
            assert a[lc.FORWARD] == a[lc.XSIDE] and b[lc.ESIDE] == a[lc.XSIDE] ^ 1
        assert np.array_equal(rep.ops()[t[:, lc.P]][::-1][np.unique(t[::-1, lc.P], return_index=True)[1]],
                              t[::-1][np.unique(t[::-1, lc.P], return_index=True)[1], lc.WORD])  # the last word written to a slot is there
        rows_seen += len(t)
    assert rows_seen > 200


def test_features_of_a_hand_made_walk():
    """features() on three rows written by hand: W = 1 (T = 256), M = 513, CH = 512."""
    rows = np.zeros((3, 11), dtype=np.uint32)
    rows[0, [lc.P, lc.VAR, lc.DIST, lc.FORWARD, lc.WRAPPED]] = [512, 32, 1, 1, 1]   # from p = M - 1 forward across p = 0
    rows[1, [lc.P, lc.VAR, lc.DIST, lc.FORWARD, lc.WRAPPED, lc.EREL]] = [0, 5, 256, 1, 0, 1]  # d = T, entered through rel 1
    rows[2, [lc.P, lc.VAR, lc.DIST, lc.WRAPPED, lc.CLOSED]] = [256, 9, 513, 1, 2]  # backward, the op itself
    rows[:, lc.WORD] = lc.op_word(3, 1, 2)
    ops = np.zeros(513, dtype=np.uint32)
    ops[512] = 1
    f = lc.features(rows, (0, 512), 513, 1, 512, ops)
    assert f == Counter(tile_last_lane=1, self_found=1, self_in_tail_tile=1, wrap_fwd=1, wrap_bwd=1, wrap_var_31_32=1, near_wrap_fwd=1,
                        spec_on=3, two_var_rel1=1, hop_visited=3, start_chunk_k=1, start_first_of_chunk=1, start_behind_empty_chunk=1,
                        closed_on_arrival=1, far_search_3=1), f
    assert lc.features(rows[:0], (0, 0), 513, 1, 512) == Counter()


@pytest.mark.parametrize("case", lc.CASES, ids=lc.CASE_IDS)
def test_case_reaches_its_features(oracle, case):
    m, reps = lc.oracle_replicas(oracle, case)
    assert all(rep.verify() for rep in reps)  # (a placed string is a valid configuration)
    if case.layout is not None:
        assert all(rep.cutoff == case.cutoff0 and not rep.state().any() for rep in reps)
    total = Counter()
    for _ in range(case.loops):
        total.update(lc.oracle_round(case, reps)[1])
    missing = {f: total[f] for f in case.claims if total[f] < lc.MIN_COUNT}
    assert not missing, f"{case.name}: claimed features reached fewer than {lc.MIN_COUNT} times: {missing} (all: {dict(total)})"
    assert all(rep.verify() for rep in reps)
    assert set(case.claims) <= set(lc.FEATURES)


def test_every_owed_feature_is_claimed():
    """Every feature is claimed on generic W = 1, generic W = 4 and the trimmed kernel (far searches, spec and the start search on
    generic W = 16 too); M = 2 T and M = 2 T + 1 both occur among the placed strings of each of them."""
    for group, owed in lc.OWED.items():
        cases = [c for c in lc.CASES if c.group == group]
        claimed = set().union(*(c.claims for c in cases))
        assert not set(owed) - claimed, (group, sorted(set(owed) - claimed))
        T = lc.tile(lc.launch_waves(cases[0]))
        assert all(lc.launch_waves(c) * 256 == T for c in cases)
        assert {2 * T, 2 * T + 1} <= {c.cutoff0 for c in cases if c.layout == "dist"}, group
    assert all(c.fast for c in lc.CASES if c.group == "trimmed") and all(c.mode == "step" for c in lc.CASES if c.group == "trimmed")
    for c in lc.CASES:
        if c.layout is not None:  # a chunk of two sub-tiles or more
            assert lc.chunk_size(c.cap) >= 2 * lc.tile(lc.launch_waves(c)), c.name


def test_mixed_batch_walks_far_next_to_an_empty_replica(oracle):
    case = lc.MIXED
    m, reps = lc.oracle_replicas(oracle, case)
    lc.empty_first_replica(reps)
    assert reps[0].n == 0 and reps[0].cutoff > 64
    rounds = 0
    for _ in range(case.loops):
        e0 = reps[0].epoch
        lens, _ = lc.oracle_round(case, reps)
        assert lens[0] == 0 and reps[0].epoch == e0 + 1
        rounds += max(lens[1:]) > 64
    assert rounds >= lc.MIN_COUNT, rounds


@pytest.mark.parametrize("case", list(lc.CASES) + [lc.MIXED], ids=lc.CASE_IDS + [lc.MIXED.name])
def test_case_gets_the_launch_it_was_chosen_for(case):
    """isingmc_plan_batch (no device needed) for the case's config on 160 KB of LDS: the wave count its tile size was computed
    from, the chunk size, four slots per lane, the trimmed diagonal kernel exactly where the case is meant for it, the edge table
    in LDS exactly on TFIM batches without CFG_NO_LDS_TABLES, per-variable tables in LDS."""
    import isingmontecarlo_amd as im
    import _plan_cases as pc
    nvars, ints, edges, gamma, _ = lc.model_parts(case.model)
    model = dict(edges=edges or [], nvars=nvars, transverse=gamma, longitudinal=0.0, interactions=ints)
    wishes = dict(nreplicas=case.R, capacity=case.cap, cutoff=case.cutoff0, flags=case.cfg, waves_per_replica=case.waves,
                  slots_per_lane=4 if case.waves else 0)
    cfg, keep = pc.config_of(im, wishes, model=model)
    rc, out = pc.plan_batch(im, cfg, 160 * 1024)
    assert rc == 0
    p = dict(zip(pc.SLOTS, out))
    assert p["W"] == lc.launch_waves(case) and p["K"] == 4 and p["CH"] == lc.chunk_size(case.cap), p
    assert bool(p["fast_diag"]) == case.fast, p
    assert p["mode"] == (pc.MODE_LDS_EDGES if ints is None and case.cfg == 0 else pc.MODE_GENERAL), p
