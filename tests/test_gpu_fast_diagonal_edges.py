"""The trimmed diagonal kernel (csrc/sse_fast.hip.h) at the edges of its integer acceptance rule (csrc/sse_accept.h), bit-exact
against the CPU oracle: temperatures from beta = 0.05 to 4096 (a non-dyadic one among them), with and without a longitudinal
field (its own weight class), a starting cutoff of 16 so that the first sweeps run with M - n down to 1, both tile shapes, with
and without a directed loop behind the pass — and one batch whose capacity lies beyond 2^21, which takes the kernel's f64
rounds.  Every case asserts that the trimmed kernel really ran."""
import numpy as np
import pytest

import _lattices as lat

pytestmark = pytest.mark.gpu


def make_pair(oracle, edges, gamma, h, cutoff, cap, seed, R, waves=0, k=0):
    import isingmontecarlo_amd as im
    g = im.QmcIsingGraph(edges, gamma, h, cutoff, seed, nreplicas=R, capacity=cap, waves_per_replica=waves, slots_per_lane=k)
    e, j = lat.split(edges)
    m = oracle.Model(g.nvars, e, j, gamma, h)
    reps = [oracle.Replica(m, cap, cutoff, seed, r, None) for r in range(R)]
    return g, m, reps


def assert_same(g, reps, what=""):
    n = g.get_n()
    cut = g.get_cutoff()
    st = g.state_ref()
    ep = g.get_epoch()
    for r, rep in enumerate(reps):
        assert n[r] == rep.n, f"{what}: n differs for replica {r}: {n[r]} vs {rep.n}"
        assert cut[r] == rep.cutoff, f"{what}: cutoff differs for replica {r}"
        assert ep[r] == rep.epoch, f"{what}: epoch differs for replica {r}"
        assert np.array_equal(st[r], rep.state()), f"{what}: state differs for replica {r}"
        ops = g.export_ops(r)
        assert np.array_equal(ops, rep.ops()), f"{what}: op words differ for replica {r}"


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("h", [0.0, 0.3])
@pytest.mark.parametrize("beta", [0.05, 1.0 / 3.0, 4.0, 64.0, 4096.0])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("l", [4, 8])
def test_trimmed_diagonal_at_the_edges_of_the_rule(oracle, l, k, beta, h, flags):
    R, steps = 8, 30
    g, m, reps = make_pair(oracle, lat.two_d_ferro(l), 1.0, h, 16, 1 << 20, 8642, R, waves=4, k=k)
    info = g.launch_info()
    assert info["fast_diagonal"] and info["waves_per_replica"] == 4 and info["slots_per_lane"] == k
    g.run(steps, beta, flags=flags)
    oracle.batch_timesteps(reps, steps, [beta] * R, 1, flags)
    what = f"{l}x{l} k={k} beta={beta} h={h} flags={flags}"
    assert_same(g, reps, what)
    acc = g.accumulators()
    for r, rep in enumerate(reps):
        assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), what
    assert g.verify().all(), what


def test_capacity_beyond_the_exactness_bound_takes_the_f64_rounds(oracle):
    """Cutoffs beyond 2^21 are beyond the range in which the oracle's f64 product is exact: such a batch runs the f64 rounds."""
    R, steps, beta = 2, 6, 4.0
    g, m, reps = make_pair(oracle, lat.two_d_ferro(4), 1.0, 0.0, 16, (1 << 21) + 1024, 97531, R, waves=4, k=4)
    assert g.launch_info()["fast_diagonal"]
    g.run(steps, beta)
    oracle.batch_timesteps(reps, steps, [beta] * R)
    assert_same(g, reps, "capacity 2^21 + 1024")
    assert g.verify().all()
