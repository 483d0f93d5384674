"""GPU dense-end parity: few variables with long operator strings, bit-exact against the CPU oracle.

Every other parity module sits at the sparse end (2-8 sites at beta <= 3, long strings only on 8x8 to 64x64 lattices).  Here a
64-slot row holds many ops on the same variable, so the lane-order fallbacks of the kernels become their main path:
  * the trimmed diagonal kernel (sse_fast.hip.h) and the general diagonal pass: two off-diagonal ops of a row on one variable;
  * the general cluster scan and the dedicated cluster kernel (sse_cluster.hip.h): two cuts of a row on one variable;
and the dedicated cluster kernel meets its own gate: with S = 16 N + C ids (C transverse ops) its S flip bits need more words
than the 16 (N + 1) of the per-wave tables they reuse, which sends the replica to the general kernel (at the plan, or in the
kernel itself when the cuts grow inside one call).  Every case proves from the oracle's op words that it is at that edge.
"""
import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import make_pair, assert_same

pytestmark = pytest.mark.gpu

RING5 = [((0, 1), 0.7), ((1, 2), -1.3), ((2, 3), 1.9), ((3, 4), -0.6), ((4, 0), 1.1)]
CAP = 1 << 16
# name, edges, gamma, h, beta: all cross the flip-bit bound of the dedicated cluster kernel within 60 timesteps
DENSE = [
    ("ring8_fm_b600", lat.one_d_periodic(8, -1.0), 1.0, 0.0, 600.0),
    ("ring4_afm_b500", lat.one_d_periodic(4, 1.0), 1.0, 0.0, 500.0),
    ("bond_b800", [((0, 1), 1.0)], 1.0, 0.0, 800.0),
    ("ring6_fm_h_b500", lat.one_d_periodic(6, -1.0), 1.0, 0.3, 500.0),
    ("ring5_rand_b300", RING5, 1.2, 0.0, 300.0),
    ("ring5_rand_h_b300", RING5, 1.2, -0.4, 300.0),
]
IDS = [c[0] for c in DENSE]


def nvars_of(edges):
    return max(max(e) for e, _ in edges) + 1


def dense_stats(reps, E, N):
    """From the oracle's op words: the largest S = 16 N + C over the replicas, its flip-bit words (S + 31) / 32, and the share of
    occupied 64-slot rows that hold two or more off-diagonal ops / two or more cuts (transverse ops) on one variable."""
    import isingmontecarlo_amd as im
    S, rows, off2, cut2 = [], 0, 0, 0
    for rep in reps:
        w = rep.ops()
        nz = np.flatnonzero(w)
        for p in nz[:: max(1, len(nz) // 200)]:  # the vectorised decode below agrees with op_fields
            bond, i, o = im.op_fields(int(w[p]))
            assert bond == (int(w[p]) >> 4) - 1 and i == int(w[p]) & 3 and o == (int(w[p]) >> 2) & 3
        w = np.pad(w, (0, -len(w) % 64)).reshape(-1, 64)
        bond = (w >> 4).astype(np.int64) - 1
        cut = (w != 0) & (bond >= E) & (bond < E + N)
        offd = (w != 0) & ((w & 3) != ((w >> 2) & 3))  # (in a transverse-field model only transverse ops are off-diagonal)
        assert not (offd & ~cut).any()
        key = np.arange(w.shape[0])[:, None] * N + (bond - E)
        def rows_with_two(mask):
            cnt = np.bincount(key[mask], minlength=w.shape[0] * N).reshape(-1, N)
            return int((cnt >= 2).any(axis=1).sum())
        occ = int((w != 0).any(axis=1).sum())
        rows += occ
        off2 += rows_with_two(offd)
        cut2 += rows_with_two(cut)
        S.append(16 * N + int(cut.sum()))
    return dict(S=S, maxS=max(S), bits=[(s + 31) // 32 for s in S], table=16 * (N + 1), rows=rows,
                off2=off2 / max(rows, 1), cut2=cut2 / max(rows, 1))


def assert_dense(st, what, off2=0.8, cut2=0.8):
    """At least one replica beyond the dedicated kernel's flip-bit bound, and the fallbacks of the row scans taken in most rows."""
    assert max(st["bits"]) > st["table"], f"{what}: not at the edge: {st}"
    assert st["off2"] >= off2 and st["cut2"] >= cut2, f"{what}: too few rows take the lane-order fallbacks: {st}"


def assert_acc(g, reps):
    acc = g.accumulators()
    for r, rep in enumerate(reps):
        assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), f"accumulators differ r={r}: {acc[r]} vs {rep.accumulators()}"


def run_both(g, reps, t, beta, freq, flags):
    g.run(t, beta, sampling_freq=freq, flags=flags)
    betas = np.broadcast_to(np.asarray(beta, dtype=np.float64), (len(reps),))
    for rep, b in zip(reps, betas):
        rep.timesteps(t, float(b), freq, flags)


# whole timesteps in the default geometry (trimmed diagonal kernel, then the dedicated cluster kernel with deferred flips):
# 0 = diagonal + cluster, 1 = + directed loop, 4 = heat-bath diagonal update (general diagonal kernel), 8 = + RVB sweep
# (growth + main launches), 8 with CFG_RVB_FUSED = RVB through the fused kernel
@pytest.mark.parametrize("flags,rvb_fused", [(0, False), (1, False), (4, False), (8, False), (8, True)], ids=["f0", "f1", "f4", "f8", "f8fused"])
@pytest.mark.parametrize("name,edges,gamma,h,beta", DENSE, ids=IDS)
def test_dense_timesteps(oracle, name, edges, gamma, h, beta, flags, rvb_fused):
    import isingmontecarlo_amd as im
    N, R = nvars_of(edges), 4
    g, m, reps = make_pair(oracle, edges, gamma, h, N, CAP, 4711, R, cfg_flags=im.CFG_RVB_FUSED if rvb_fused else 0)
    uniform = len({abs(j) for _, j in edges}) == 1
    assert g.launch_info()["fast_diagonal"] == uniform  # (couplings of several sizes: no LDS edge table, the general kernels)
    run_both(g, reps, 60, beta, 3, flags)
    assert_same(g, reps, f"{name} flags={flags}")
    assert_acc(g, reps)
    assert g.verify().all()
    st = dense_stats(reps, len(edges), N)
    assert_dense(st, name)
    # Which gate sent the replicas to the general kernel.  Without RVB, run() replans every 16 timesteps from the transverse-op
    # counts, and the plan drops the dedicated kernel.  With RVB, the plan is made once, before the call has seen any count: the
    # dedicated kernel runs every cluster update and its own gate flags each replica beyond the bound.
    info = g.launch_info()
    assert info["lean_cluster"] == (uniform and bool(flags & 8)), (info, st)
    if flags & 8:
        assert info["rvb_split"] == (not rvb_fused)


# single primitives, compared one by one: diagonal update, cluster update, directed loop, RVB sweep, free spins; default
# geometry, the dedicated kernel applying its flips itself, and the general cluster kernel only
@pytest.mark.parametrize("cfg", ["default", "no_deferred", "no_lean"])
@pytest.mark.parametrize("name,edges,gamma,h,beta", DENSE, ids=IDS)
def test_dense_primitives(oracle, name, edges, gamma, h, beta, cfg):
    import isingmontecarlo_amd as im
    N, R = nvars_of(edges), 4
    cfgf = {"default": 0, "no_deferred": im.CFG_NO_DEFERRED_FLIPS, "no_lean": im.CFG_NO_LEAN_CLUSTER}[cfg]
    g, m, reps = make_pair(oracle, edges, gamma, h, N, CAP, 2024, R, cfg_flags=cfgf)
    run_both(g, reps, 40, beta, 1, 0)
    assert_same(g, reps, f"{name} warm-up")
    for it in range(4):
        g.single_diagonal_step(beta)
        for rep in reps:
            rep.diagonal_update(beta)
            want = rep.n + rep.n // 2
            if want > rep.cutoff:
                assert rep.set_cutoff(want) == 0
        assert_same(g, reps, f"{name} diag it={it}")
        st = dense_stats(reps, len(edges), N)
        nc = g.single_cluster_step(flip_free=False)
        for r, rep in enumerate(reps):
            assert nc[r] == rep.cluster_update(0.5), f"{name}: cluster count differs it={it} r={r}"
        assert_same(g, reps, f"{name} cluster it={it}")
        assert g.launch_info()["lean_cluster"] is False  # (the plan: these counts are far beyond the bound)
        lens = g.loop_update()
        for r, rep in enumerate(reps):
            assert lens[r] == rep.loop_update(), f"{name}: loop length differs it={it} r={r}"
        assert_same(g, reps, f"{name} loop it={it}")
        succ, upd = g.single_rvb_sweep()
        for r, rep in enumerate(reps):
            assert succ[r] == rep.rvb_update(upd), f"{name}: RVB successes differ it={it} r={r}"
        assert_same(g, reps, f"{name} rvb it={it}")
        g.flip_free_spins()
        for rep in reps:
            rep.flip_free_spins()
        assert_same(g, reps, f"{name} free it={it}")
    assert_dense(st, name)
    assert g.verify().all()


# explicit geometries: the general kernels only (an explicit wave count switches the trimmed and dedicated kernels off), whose
# sub-rounds of 64 slots take their lane-order fallbacks
@pytest.mark.parametrize("waves", [1, 4, 16])
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("name,edges,gamma,h,beta", [DENSE[0], DENSE[3], DENSE[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_dense_explicit_geometries(oracle, name, edges, gamma, h, beta, waves, k):
    N, R = nvars_of(edges), 3
    g, m, reps = make_pair(oracle, edges, gamma, h, N, CAP, 99, R, waves=waves, k=k)
    info = g.launch_info()
    assert info["waves_per_replica"] == waves and info["slots_per_lane"] == k and not info["lean_cluster"]
    run_both(g, reps, 50, beta, 2, 1)
    assert_same(g, reps, f"{name} W={waves} K={k}")
    assert_acc(g, reps)
    assert g.verify().all()
    assert_dense(dense_stats(reps, len(edges), N), name)


def test_dense_kernel_gate_inside_one_call(oracle):
    """The dedicated kernel's own gate, not the plan's.  A ring of 8 at beta = 200 stays inside the bound, so the plan keeps the
    dedicated kernel; a call of fewer than 16 timesteps plans once (run() replans every 16), so when the cuts grow at beta = 600
    during that call, the kernel itself must flag the replicas beyond the bound and the general kernel follow up.  The second
    call runs a batch with replicas on both sides of the bound (per-replica beta)."""
    edges = lat.one_d_periodic(8, -1.0)
    N, R = 8, 4
    for betas in ([600.0] * R, [200.0, 600.0, 200.0, 600.0]):
        g, m, reps = make_pair(oracle, edges, 1.0, 0.0, N, CAP, 555, R)
        run_both(g, reps, 60, 200.0, 2, 0)
        assert_same(g, reps, "beta 200")
        st0 = dense_stats(reps, len(edges), N)
        assert max(st0["bits"]) <= st0["table"] and g.launch_info()["lean_cluster"], st0  # the plan accepted
        run_both(g, reps, 15, betas, 2, 0)
        assert g.launch_info()["lean_cluster"]  # no replan inside this call: the dedicated kernel ran every cluster update
        assert_same(g, reps, f"beta {betas}")
        assert_acc(g, reps)
        assert g.verify().all()
        st = dense_stats(reps, len(edges), N)
        assert_dense(st, f"gate {betas}")
        for bits, b in zip(st["bits"], betas):  # (mixed batch: both sides of the bound in every launch of the call)
            assert (bits > st["table"]) == (b == 600.0), st


def test_dense_sixteen_bit_ids(oracle):
    """32x32 ferromagnet at betas where S = 16 N + C straddles 65535 across the replicas: the ids no longer fit 16 bits for some
    of them (the general kernel's 32-bit union-find in HBM) while the others stay below."""
    edges = lat.two_d_ferro(32)
    N, R = 1024, 4
    betas = [34.0, 37.0, 40.0, 43.0]
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, N, 1 << 20, 4242, R)
    g.run(40, betas)
    oracle.batch_timesteps(reps, 40, betas)
    assert_same(g, reps, "32x32 16-bit edge")
    assert_acc(g, reps)
    assert g.verify().all()
    st = dense_stats(reps, len(edges), N)
    assert min(st["S"]) < 65535 <= max(st["S"]), st
    assert st["cut2"] > 0.05, st  # (1024 variables: a row holds two cuts on one variable less often)
    assert not g.launch_info()["lean_cluster"]


@pytest.mark.parametrize("rvb_fused", [False, True])
def test_dense_rvb_constant_table_beyond_lds_is_loud(oracle, rvb_fused):
    """The RVB sweep keeps its table of constant (transverse) ops in LDS.  The smallest model, one bond at beta = 12000, holds
    more than 40960 of them: beyond the 160 KiB of LDS a workgroup can have, whatever sits in front of the table.  The sweep must
    end in ECAPACITY with the documented message, after whole timesteps that match the oracle."""
    import isingmontecarlo_amd as im
    edges = [((0, 1), 1.0)]
    R, beta = 2, 12000.0
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 2, 1 << 17, 808, R, cfg_flags=im.CFG_RVB_FUSED if rvb_fused else 0)
    run_both(g, reps, 40, beta, 1, 0)
    assert_same(g, reps, "bond beta 12000")
    assert g.verify().all()
    st = dense_stats(reps, len(edges), 2)
    assert min(st["S"]) - 32 > 40960, st
    with pytest.raises(im.IsingMcError) as ei:
        g.single_rvb_sweep()
    assert ei.value.code == -3 and "RVB working set exceeds the LDS scratch" in str(ei.value), str(ei.value)
