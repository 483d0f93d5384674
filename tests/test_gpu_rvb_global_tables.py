"""RVB sweeps with their per-variable tables in HBM (ISINGMC_CFG_RVB_GLOBAL_TABLES, sse_rvb.hip.h rvb_pass<.., G = true>): forced on
small models in both bond decodes, on the +-J models whose scan tables live in HBM (BASELINE configs[4], in small and at full size),
and on a model with more constant ops than LDS holds.  Bit-exact against the oracle: n, cutoff, epoch, state, op words and RVB
successes."""
import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import RVB_CASES, make_pair, assert_same
from test_gpu_dense_end import assert_acc, dense_stats, run_both

pytestmark = pytest.mark.gpu


def rvb_sweeps_match(g, reps, its, beta, what, cluster=True):
    """Diagonal step, standalone RVB sweep (attempt by attempt: successes, then everything else), cluster step; `its` times."""
    for it in range(its):
        g.single_diagonal_step(beta)
        for rep in reps:
            rep.diagonal_update(beta)
            want = rep.n + rep.n // 2
            if want > rep.cutoff:
                assert rep.set_cutoff(want) == 0
        succ, upd = g.single_rvb_sweep()
        for r, rep in enumerate(reps):
            assert succ[r] == rep.rvb_update(upd), f"{what}: RVB successes differ it={it} r={r}"
        assert_same(g, reps, f"{what} rvb it={it}")
        if cluster:
            g.single_cluster_step(flip_free=True)
            for rep in reps:
                rep.cluster_update(0.5)
                rep.flip_free_spins()
            assert_same(g, reps, f"{what} cluster it={it}")


def tables_flags(im, tg):
    return im.CFG_RVB_GLOBAL_TABLES | (im.CFG_GLOBAL_TABLES | im.CFG_NO_LDS_TABLES if tg else 0)


@pytest.mark.parametrize("tg", [False, True], ids=["lds_tables", "hbm_tables"])
@pytest.mark.parametrize("name,edges,gamma,h,beta,cutoff", RVB_CASES, ids=[c[0] for c in RVB_CASES])
def test_rvb_tables_in_hbm_forced_on_small_models(oracle, name, edges, gamma, h, beta, cutoff, tg):
    """The seven RVB models under CFG_RVB_GLOBAL_TABLES: alone (the LDS edge-table decode where the model takes it) and with the
    scan tables in HBM too (general bond records).  Standalone sweeps attempt by attempt, then whole timesteps with RVB and with
    RVB + heat-bath."""
    import isingmontecarlo_amd as im
    R = 4
    g, m, reps = make_pair(oracle, edges, gamma, h, cutoff, 8192, 1357, R, cfg_flags=tables_flags(im, tg))
    info = g.launch_info()
    assert info["global_tables"] == tg and not info["rvb_global_tables"], info
    rvb_sweeps_match(g, reps, 8, beta, name)
    info = g.launch_info()
    assert info["rvb_global_tables"] and not info["rvb_split"], info
    for flags in (im.FLAG_RVB, im.FLAG_RVB | im.FLAG_HEATBATH):
        run_both(g, reps, 12, beta, 2, flags)
        assert_same(g, reps, f"{name} timesteps flags={flags}")
    assert g.verify().all()
    assert g.launch_info()["rvb_global_tables"]


@pytest.mark.parametrize("tg", [False, True], ids=["lds_tables", "hbm_tables"])
@pytest.mark.parametrize("flags", [8, 8 | 1, 8 | 4], ids=["rvb", "rvb_loop", "rvb_heatbath"])
def test_rvb_tables_in_hbm_inside_fused_and_split_timesteps(oracle, flags, tg):
    """Whole timesteps whose RVB sweep needs a launch of its own: inside fused launches (CFG_FUSED_LAUNCH) and in front of a directed
    loop in the split form; sampling on, so the accumulators see the steps in order."""
    import isingmontecarlo_amd as im
    edges = lat.two_d_ferro(8)
    R, beta = 4, 3.0
    for fused in (False, True):
        cfg = tables_flags(im, tg) | (im.CFG_FUSED_LAUNCH if fused else 0)
        g, m, reps = make_pair(oracle, edges, 1.0, 0.3, 64, 8192, 2468, R, cfg_flags=cfg)
        run_both(g, reps, 15, beta, 3, flags)
        assert_same(g, reps, f"fused={fused} flags={flags}")
        assert_acc(g, reps)
        assert g.verify().all()
        assert g.launch_info()["rvb_global_tables"]


@pytest.mark.parametrize("no_pm", [False, True], ids=["pm_decode", "general_records"])
def test_rvb_tables_in_hbm_on_per_replica_couplings_with_a_field(oracle, no_pm):
    """configs[4] in small: 4^3 +-J, one realisation per replica, h = 0.1, scan tables in HBM (the +-J decode's mode, and the general
    records with CFG_NO_PM_DECODE).  The RVB sweep decodes through the general records either way."""
    import isingmontecarlo_amd as im
    l, R = 4, 5
    edges = lat.cubic_periodic(l)
    rng = np.random.default_rng(99)
    J = rng.choice([-1.0, 1.0], size=(R, len(edges)))
    cfg = im.CFG_GLOBAL_TABLES | im.CFG_RVB_GLOBAL_TABLES | (im.CFG_NO_PM_DECODE if no_pm else 0)
    g = im.QmcIsingGraph(edges, 1.0, 0.1, 64, 777, nreplicas=R, capacity=1 << 13, couplings=J, cfg_flags=cfg)
    assert g.launch_info()["global_tables"]
    e = [ab for ab, _ in edges]
    reps = [oracle.Replica(oracle.Model(g.nvars, e, list(J[r]), 1.0, 0.1), 1 << 13, 64, 777, r, None) for r in range(R)]
    g.run(25, 2.0)
    oracle.batch_timesteps(reps, 25, [2.0] * R)
    assert_same(g, reps, "cubic +-J, tables in HBM")
    for it in range(3):
        succ, upd = g.single_rvb_sweep()
        for r, rep in enumerate(reps):
            assert succ[r] == rep.rvb_update(upd), (it, r)
        assert_same(g, reps, f"cubic +-J rvb sweep {it}")
    assert g.launch_info()["rvb_global_tables"]
    for flags in (im.FLAG_RVB, im.FLAG_RVB | im.FLAG_HEATBATH):
        g.run(12, 2.0, flags=flags)
        oracle.batch_timesteps(reps, 12, [2.0] * R, 1, flags)
        assert_same(g, reps, f"cubic +-J timesteps flags={flags}")
    assert g.verify().all()


def test_rvb_tables_in_hbm_beyond_the_lds_constant_table(oracle):
    """The one-bond model at beta = 12000 holds more than 40960 constant ops: beyond LDS for the LDS form (which ends in ECAPACITY,
    test_gpu_dense_end.py), within the HBM table.  Sweeps and timesteps with RVB match the oracle."""
    import isingmontecarlo_amd as im
    edges = [((0, 1), 1.0)]
    R, beta = 2, 12000.0
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 2, 1 << 17, 808, R, cfg_flags=im.CFG_RVB_GLOBAL_TABLES)
    run_both(g, reps, 40, beta, 1, 0)
    assert_same(g, reps, "bond beta 12000")
    st = dense_stats(reps, len(edges), 2)
    assert min(st["S"]) - 32 > 40960, st
    for it in range(3):
        succ, upd = g.single_rvb_sweep()
        for r, rep in enumerate(reps):
            assert succ[r] == rep.rvb_update(upd), (it, r)
        assert_same(g, reps, f"bond beta 12000 rvb sweep {it}")
    run_both(g, reps, 4, beta, 1, im.FLAG_RVB)
    assert_same(g, reps, "bond beta 12000 timesteps with RVB")
    assert g.verify().all()
    assert g.launch_info()["rvb_global_tables"]


def test_rvb_tables_in_hbm_at_configs4_full_size(oracle):
    """BASELINE configs[4] at its lattice size: 32^3, per-replica +-J, Gamma = 1, h = 0.1, beta = 4, on the HBM-table path the engine
    picks by itself.  After 12 equilibrating timesteps: standalone RVB sweeps and whole timesteps with RVB, against the oracle.
    Cost, measured, almost all of it the oracle's (8-core box): the 12 timesteps under 1 s; a U = 512 sweep 6.7 s for the four
    replicas (U = 4096: 54 s, hence 512); the two timesteps with RVB — full sweeps of 16 384 attempts, one replica per thread —
    116-144 s.  The whole test: 95 s on an MI355X host."""
    import isingmontecarlo_amd as im
    l, R, beta, sweeps, U = 32, 4, 4.0, 12, 512
    edges = lat.cubic_periodic(l)
    nsite = l ** 3
    rng = np.random.default_rng(32768)
    J = rng.choice([-1.0, 1.0], size=(R, len(edges)))
    cap = 1 << 21
    g = im.QmcIsingGraph(edges, 1.0, 0.1, nsite, 2026, nreplicas=R, capacity=cap, couplings=J, cfg_flags=im.CFG_RVB_GLOBAL_TABLES)
    e = [ab for ab, _ in edges]
    reps = [oracle.Replica(oracle.Model(nsite, e, list(J[r]), 1.0, 0.1), cap, nsite, 2026, r, None) for r in range(R)]
    g.run(sweeps, beta)
    oracle.batch_timesteps(reps, sweeps, [beta] * R)
    assert_same(g, reps, "32^3 +-J")
    for it in range(2):
        succ, upd = g.single_rvb_sweep(updates_in_sweep=U)
        assert upd == U
        for r, rep in enumerate(reps):
            assert succ[r] == rep.rvb_update(U), (it, r)
        assert_same(g, reps, f"32^3 +-J rvb sweep {it}")
    g.run(2, beta, flags=im.FLAG_RVB)
    oracle.batch_timesteps(reps, 2, [beta] * R, 1, im.FLAG_RVB)
    assert_same(g, reps, "32^3 +-J timesteps with RVB")
    assert g.verify().all()
    info = g.launch_info()
    assert info["global_tables"] and info["rvb_global_tables"], info


def test_without_the_flag_models_with_tables_in_hbm_still_refuse_rvb(oracle):
    """CFG_RVB_GLOBAL_TABLES is the only switch: the same forced-HBM model without it still returns ENOTIMPL, and launch_info says
    that no RVB sweep kept its tables in HBM."""
    import isingmontecarlo_amd as im
    g, m, reps = make_pair(oracle, lat.two_d_periodic(4), 1.0, 0.0, 8, 8192, 4321, 4, cfg_flags=im.CFG_GLOBAL_TABLES | im.CFG_NO_LDS_TABLES)
    g.run(3, 2.0)
    with pytest.raises(im.IsingMcError) as ei:
        g.single_rvb_sweep()
    assert ei.value.code == -5 and "ISINGMC_CFG_RVB_GLOBAL_TABLES" in str(ei.value), str(ei.value)
    with pytest.raises(im.IsingMcError) as ei:
        g.run(1, 2.0, flags=im.FLAG_RVB)
    assert ei.value.code == -5
    assert not g.launch_info()["rvb_global_tables"]


def test_rvb_table_scratch_is_freed_with_the_batch():
    """The table scratch (allocated on the first RVB sweep with the flag: about 4 * capacity bytes per replica, 1 GiB here) goes with
    the batch: creating, sweeping and closing such a batch again and again leaves the device's free memory where it was."""
    import torch
    import isingmontecarlo_amd as im
    R, cap = 64, 1 << 22
    per_batch = R * 4 * cap

    def cycle():
        g = im.QmcIsingGraph(lat.two_d_ferro(8), 1.0, 0.0, 64, 97, nreplicas=R, capacity=cap, cfg_flags=im.CFG_RVB_GLOBAL_TABLES)
        g.run(3, 2.0)
        g.single_rvb_sweep()
        assert g.launch_info()["rvb_global_tables"]
        g.close()
        torch.cuda.synchronize()

    cycle()  # (first use: runtime and code-object set-up)
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(6):
        cycle()
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 >= free0 - 2 * per_batch, (free0, free1, per_batch)  # (a leak would be >= 6 * per_batch)
