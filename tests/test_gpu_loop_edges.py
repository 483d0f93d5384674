"""The directed loop (csrc/sse_loop.hip.h) where its walks are long and its searches leave the first tile, bit for bit against the
CPU oracle: the cases of tests/_loop_cases.py (what each is for, and why it reaches it, is written there and in DESIGN.md).

Every case builds the device batch and the oracle's replicas from the same seed, brings both to the same string (whole timesteps,
or a placed string), checks that they agree, asserts from the ORACLE's trace that the case still reaches the features it claims,
and only then compares round by round: walk lengths, op words, n, cutoff, epoch, p = 0 states, accumulators.  A round is one
g.loop_update() (general kernel) or one whole timestep with a loop (the trimmed kernel, which no primitive reaches).  Every call
of the binding raises on a replica's error flag, so a case that ends has no sticky error."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import _lattices as lat
import _loop_cases as lc
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

NEVER = 1 << 20  # sampling frequency of the single-timestep calls: no call ever samples


def plan_chunk_size(cap):
    import isingmontecarlo_amd as im
    out = (C.c_uint32 * 4)()
    assert im.load_library().isingmc_plan_geometry(cap, 4, 4, 16, out) == 0
    return int(out[0])


def device_batch(model, waves, cfg, cap, cutoff0, seed, R, placed):
    import isingmontecarlo_amd as im
    nvars, ints, edges, gamma, _ = lc.model_parts(model)
    state = np.zeros(nvars, dtype=np.uint8) if placed else None
    k = 4 if waves else 0
    if ints is not None:
        assert cfg == 0  # (CFG_NO_LDS_TABLES only keeps the Ising edge table out of LDS: a generic batch has none)
        return im.Qmc.from_interactions(nvars, ints, cutoff0, seed, state=state, nreplicas=R, capacity=cap, waves_per_replica=waves,
                                        slots_per_lane=k, do_loop_updates=True, do_cluster_updates=False)
    return im.QmcIsingGraph(edges, gamma, 0.0, cutoff0, seed, state=state, nreplicas=R, capacity=cap, waves_per_replica=waves,
                            slots_per_lane=k, cfg_flags=cfg, nvars=nvars)


def check_geometry(g, case):
    """What the launch reports, against what the case's features were computed for."""
    info = g.launch_info()
    generic = case.model[0] == "xxz"
    assert info["waves_per_replica"] == lc.launch_waves(case) and info["slots_per_lane"] == 4, info
    assert info["fast_diagonal"] == case.fast, info
    assert info["lds_edge_table"] == (not generic and case.cfg == 0), info
    assert not info["global_tables"], info
    assert plan_chunk_size(case.cap) == lc.chunk_size(case.cap)


def same_accumulators(g, reps, what):
    acc = g.accumulators()
    for r, rep in enumerate(reps):
        assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), f"{what}: accumulators differ r={r}: {acc[r]} vs {rep.accumulators()}"
    return acc


def start_pair(oracle, case):
    """Device batch and oracle replicas at the same string, checked."""
    g = device_batch(case.model, case.waves, case.cfg, case.cap, case.cutoff0, case.seed, case.R, case.layout is not None)
    check_geometry(g, case)
    m, reps = lc.oracle_replicas(oracle, case)
    if case.layout is None:
        g.run(case.warm, case.beta, flags=lc.warm_flags(case))
    else:
        words = lc.placed_words(case)
        for r in range(case.R):
            g.import_ops(words, r)
        assert g.verify().all() and all(rep.verify() for rep in reps)
    return g, reps


def compare_rounds(g, reps, case, rounds):
    """`rounds` rounds on both sides, the oracle first and traced; returns the features the oracle's walks reached."""
    total = Counter()
    for it in range(rounds):
        what = f"{case.name} round {it}"
        lens, feats = lc.oracle_round(case, reps)
        total.update(feats)
        if case.mode == "prim":
            got = g.loop_update()
        else:
            before = g.accumulators()[:, 4].copy()
            g.run(1, case.beta, sampling_freq=NEVER, flags=lc.FLAG_LOOP | lc.FLAG_NO_CLUSTER)
            got = g.accumulators()[:, 4] - before
        assert np.array_equal(np.asarray(got, dtype=np.int64), np.asarray(lens, dtype=np.int64)), f"{what}: walk lengths {got} vs {lens}"
        assert_same(g, reps, what)
        same_accumulators(g, reps, what)
    return total


@pytest.mark.parametrize("case", lc.CASES, ids=lc.CASE_IDS)
def test_loop_matches_oracle(oracle, case):
    g, reps = start_pair(oracle, case)
    assert_same(g, reps, f"{case.name} start")
    same_accumulators(g, reps, f"{case.name} start")
    # the features first, from twins of the oracle's replicas: nothing is compared before the case is known to be what it claims
    _, twins = lc.oracle_replicas(oracle, case)
    total = Counter()
    for _ in range(case.loops):
        total.update(lc.oracle_round(case, twins)[1])
    missing = {f: total[f] for f in case.claims if total[f] < lc.MIN_COUNT}
    assert not missing, f"{case.name}: claimed features reached fewer than {lc.MIN_COUNT} times: {missing}"
    assert compare_rounds(g, reps, case, case.loops) == total
    assert g.verify().all() and all(rep.verify() for rep in reps)
    if case.fast:
        assert g.launch_info()["fast_diagonal"]


def test_empty_replica_next_to_long_walks(oracle):
    """One launch holds a replica without any op (it returns at once: length 0, epoch + 1) and replicas that walk past a refill."""
    case = lc.MIXED
    g, reps = start_pair(oracle, case)
    lc.empty_first_replica(reps)
    g.import_ops(np.zeros(reps[0].cutoff, dtype=np.uint32), 0)
    assert_same(g, reps, "mixed start")
    assert g.get_n()[0] == 0 and (g.get_cutoff() > 64).all()
    far = 0
    for it in range(case.loops):
        lens, _ = lc.oracle_round(case, reps)
        got = g.loop_update()
        assert np.array_equal(got, lens), (it, got, lens)
        assert got[0] == 0
        far += max(lens[1:]) > 64
        assert_same(g, reps, f"mixed round {it}")
        same_accumulators(g, reps, f"mixed round {it}")
    assert far >= lc.MIN_COUNT
    assert g.verify().all()


@pytest.mark.parametrize("name,model,waves,cap,beta,seed,flags", lc.RUN_CASES, ids=[c[0] for c in lc.RUN_CASES])
def test_loop_inside_run(oracle, name, model, waves, cap, beta, seed, flags):
    """The loop inside run(): 30 timesteps of warm-up, then 20 with 7 steps per launch, against batch_timesteps; the oracle's walks
    of those 20 steps are long (asserted on twins)."""
    R = 4
    g = device_batch(model, waves, 0, cap, 8, seed, R, False)
    info = g.launch_info()
    assert info["fast_diagonal"] == (model[0] != "xxz") and info["waves_per_replica"] == 4, info
    m = lc.oracle_model(oracle, model)
    reps, twins = ([oracle.Replica(m, cap, 8, seed, r, None) for r in range(R)] for _ in range(2))
    g.set_steps_per_launch(7)
    g.run(30, beta, flags=flags)
    for group in (reps, twins):
        oracle.batch_timesteps(group, 30, [beta] * R, 1, flags)
    assert_same(g, reps, f"{name} warm-up")
    before = np.array([t.accumulators()[4] for t in twins])
    oracle.batch_timesteps(twins, 20, [beta] * R, 1, lc.FLAG_LOOP | lc.FLAG_NO_CLUSTER)  # (the loops alone add to acc[4])
    assert ((np.array([t.accumulators()[4] for t in twins]) - before) > 20 * 8).all()  # on average far more than a bounce per loop
    g.run(20, beta, flags=flags)
    oracle.batch_timesteps(reps, 20, [beta] * R, 1, flags)
    assert_same(g, reps, name)
    same_accumulators(g, reps, name)
    assert g.verify().all()
