"""Parallel tempering: the C-ABI decision function and the label-swapping driver against the oracle's
restatement of TemperingContainer::tempering_step, single process and 2 ranks over gloo (CPU only)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _lattices as lat
import _oracle as O
import _pt_cases as pc
import _pt_reference as ptref
from _pt_backend import OracleBackend

HERE = os.path.dirname(os.path.abspath(__file__))


def small_model():
    e, j = lat.split(lat.one_d_periodic(6, -1.0))
    return O.Model(6, e, j, 1.0, 0.0)


def reference_pt(model, betas, nchains, seed, cap, cutoff, nsteps, sweeps_per_step):
    """The reference formulation: graphs live at (chain, temperature) slots and are swapped (_pt_reference.py)."""
    ref = ptref.reference_pt(model, betas, nchains, seed, cap, cutoff, nsteps, sweeps_per_step)
    return ref.by_slot, ref.swaps


def test_pt_decide_matches_oracle_step():
    import isingmontecarlo_amd as im
    rng = np.random.default_rng(7)
    m = O.Model(2, [[0, 1]], [1.0], 1.0, 0.0)
    for trial in range(20):
        T, K = int(rng.integers(2, 9)), int(rng.integers(1, 4))
        betas = np.sort(rng.uniform(0.5, 4.0, T))
        ns = rng.integers(0, 40, size=T * K)
        # oracle replicas with prescribed operator counts (transverse ops on spin 0), config id = t*K + k
        reps = []
        for c in range(T * K):
            r = O.Replica(m, 64, 2, 1, c, [0, 0])
            r.set_ops([O.op_make(1, 0, 0)] * int(ns[c]) + [0])
            reps.append(r)
        config_at = np.arange(T * K, dtype=np.uint32)
        swaps = im.pt_decide(99, trial, K, T, betas, ns.astype(np.uint32), config_at)
        oswaps = 0
        for k in range(K):
            chain = [reps[t * K + k] for t in range(T)]
            oswaps += O.pt_step(chain, betas, 99, k, trial)
            got = [reps[int(config_at[t * K + k])] for t in range(T)]
            assert [id(x) for x in got] == [id(x) for x in chain], f"trial {trial} chain {k}"
        assert swaps == oswaps


def test_label_swapping_driver_equals_graph_swapping():
    import isingmontecarlo_amd as im
    m = small_model()
    betas = np.array([0.5, 0.8, 1.2, 1.7, 2.5])
    K, seed = 3, 4321
    by_slot, swaps_ref = reference_pt(m, betas, K, seed, 2048, 6, nsteps=12, sweeps_per_step=3)
    backend = OracleBackend(m, len(betas) * K, 2048, 6, seed)
    tc = im.TemperingContainer(backend, betas, K, seed)
    for _ in range(12):
        tc.timesteps(3)
        tc.tempering_step()
    assert tc.get_total_swaps() == swaps_ref and swaps_ref > 0
    for k in range(K):
        for t in range(len(betas)):
            c = int(tc.config_at[t * K + k])
            assert np.array_equal(backend.reps[c].state(), by_slot[k][t].state())
            assert np.array_equal(backend.reps[c].ops(), by_slot[k][t].ops())
    assert tc.verify()
    # per-slot accumulators: every slot sampled every sweep
    acc = tc.slot_accumulators()
    assert (acc[:, 1] == 36).all()


@pytest.mark.parametrize("c", pc.ALL_CASES, ids=[c["name"] for c in pc.ALL_CASES])
def test_references_of_the_gpu_cases_swap_where_the_cases_look(c):
    """The references the GPU tempering tests compare against (tests/_pt_cases.py), alone: every pair of neighbouring temperatures is
    accepted at least once, the pair across the rank boundary of a two-rank case at least three times, and with per-slot Hamiltonians
    fewer than all attempts are accepted.  A case that misses one gets another seed or beta window, not a weaker condition."""
    ref = pc.check_preconditions(c)
    T, K = len(c["betas"]), c["K"]
    assert ref.attempts == (T - 1) * K * c["steps"] and sorted(ref.ids.tolist()) == list(range(T * K))
    assert (ref.acc[:, 1] == c["steps"] * c["sweeps"]).all()  # every slot sampled every sweep
    if T > 1:
        assert not np.array_equal(ref.ids, np.arange(T * K))


def test_reference_with_slot_hamiltonians_restates_the_single_chain_loop():
    """_pt_reference with per-slot Hamiltonians and K = 1 against the loop the GPU tests were written with first (one chain,
    relative weights spelled out in place): the same swaps, the same graphs."""
    edges = [((0, 1), -1.0), ((1, 2), 1.0), ((2, 3), -1.0), ((3, 0), -1.0), ((0, 2), 0.5)]
    T, beta, seed, cap, steps, E, N = 8, 3.0, 2718, 4096, 14, 5, 4
    J = np.array([[j * (1.0 + 0.04 * t) for _, j in edges] for t in range(T)])
    gam, hl = np.array([0.8 + 0.05 * t for t in range(T)]), np.array([0.30 - 0.02 * t for t in range(T)])
    e = [list(ab) for ab, _ in edges]
    hams = ptref.SlotHamiltonians(N, e, J, gam, hl)
    ref = ptref.reference_pt(None, np.full(T, beta), 1, seed, cap, 8, steps, 10, hams=hams)
    reps = [O.Replica(hams.models[t], cap, 8, seed, t) for t in range(T)]
    ids, swaps = list(range(T)), 0

    def weight(graph, t_from, t_to):
        w = 1.0
        for b_ in range(E):
            w *= ptref.powi(J[t_to][b_] / J[t_from][b_], graph.bond_count(b_))
        w *= ptref.powi(gam[t_to] / gam[t_from], sum(graph.bond_count(E + v) for v in range(N)))
        return w * ptref.powi(hl[t_to] / hl[t_from], sum(graph.bond_count(E + N + v) for v in range(N)))

    for step in range(steps):
        for t in range(T):
            reps[t].timesteps(10, beta)
        maxcut = max(r.cutoff for r in reps)
        for r in reps:
            assert r.set_cutoff(maxcut) == 0
        a_first = (ptref.philox(seed, 0, step, 0) >> 31) != 0
        for phase in range(2):
            for t in range(0 if a_first == (phase == 0) else 1, T - 1, 2):
                u = ptref.philox(seed, 1 + t, step, 0) / 4294967296.0
                ga, gb = reps[t], reps[t + 1]
                if 1.0 * (weight(ga, t, t + 1) * weight(gb, t + 1, t)) > u:
                    swaps += 1
                    na = O.Replica(hams.models[t], cap, maxcut, seed, ids[t + 1], gb.state()); na.set_ops(gb.ops()); na.set_epoch(gb.epoch)
                    nb = O.Replica(hams.models[t + 1], cap, maxcut, seed, ids[t], ga.state()); nb.set_ops(ga.ops()); nb.set_epoch(ga.epoch)
                    reps[t], reps[t + 1] = na, nb
                    ids[t], ids[t + 1] = ids[t + 1], ids[t]
    assert swaps == ref.swaps and 0 < swaps < ref.attempts and ids == ref.ids.tolist()
    for t in range(T):
        assert np.array_equal(reps[t].state(), ref.by_slot[0][t].state()) and np.array_equal(reps[t].ops(), ref.by_slot[0][t].ops())


def test_timesteps_sample_shapes_and_energy_sum():
    import isingmontecarlo_amd as im
    m = small_model()
    betas = np.array([0.7, 1.4])
    backend = OracleBackend(m, 2, 1024, 6, 5)
    tc = im.TemperingContainer(backend, betas, 1, 5)
    tc.timesteps(300)  # equilibrate: E = -<n>/beta + offset starts at +offset for an empty string
    states, esum = tc.timesteps_sample(20, replica_swap_freq=4, sampling_freq=5)
    assert [len(s) for s in states] == [4, 4]
    # reference quirk (tempering_container.rs:187-189): sum over blocks of E*t, i.e. ~ 20 * <E>
    assert esum.shape == (2,) and (esum / 20.0 < 0).all()


@pytest.mark.timeout(300)
def test_two_ranks_over_gloo_match_single_process(tmp_path):
    script = os.path.join(HERE, "_pt_gloo_worker.py")
    out = tmp_path / "result.npz"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29517")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29517", script, str(out)]
    subprocess.check_call(cmd, env=env, cwd=os.path.dirname(HERE))
    got = np.load(out)
    import isingmontecarlo_amd as im
    m = small_model()
    betas = np.array([0.5, 0.9, 1.3, 2.0])
    K, seed = 2, 777
    backend = OracleBackend(m, len(betas) * K, 2048, 6, seed)
    tc = im.TemperingContainer(backend, betas, K, seed)
    for _ in range(10):
        tc.timesteps(2)
        tc.tempering_step()
    assert int(got["swaps"]) == tc.get_total_swaps()
    assert np.array_equal(got["config_at"], tc.config_at)
    assert np.array_equal(got["n"], backend.get_n())
    assert np.array_equal(got["acc"], tc.slot_accumulators())
