"""RVB sweeps whose attempts outgrow the small growth areas and meet every cap of the working set, bit-exact against the oracle.

The cases come from _rvb_cases.py, where the oracle's statistics choose them (tests/test_rvb_working_set_cpu.py holds the conditions):
clusters of more than SSE_RVB_SLOT_CL members, boundary sets at SSE_RVB_SLOT_SET and one past it, deep inside the large areas, at
SSE_RVB_SETCAP and one past it, boundary bonds up to SSE_RVB_BONDCAP and past it, records on both sides of SSE_RVB_PROD_AHEAD, sweeps
whose regrown attempts lie in the regrow scan's last, partial group of 64, and a record buffer that grows between sweeps.  Every
growth and launch form runs them: the growth + main launches (main launch with 4, 8 and 16 waves), attempts grown one at a time, the
fused kernel, and the per-variable tables in HBM.

Past a large cap the sweep stops with ECAPACITY (code 7).  What it leaves behind, read from rvb_pass (the `GO_ERR` test in front of
rvb_attempt) and rvb_main_kernel (`if (gerr) break`, `if (stop) break`): the replica's attempts before the failing one are applied,
the failing one and everything behind it — the rest of the sweep and of the timestep — are not; the other replicas finish."""
import numpy as np
import pytest

import _rvb_cases as rc
from test_gpu_parity import make_pair, assert_same

pytestmark = pytest.mark.gpu

# name: cfg_flags, waves per replica, slots per lane (the geometries of test_rvb_update_matches_oracle), rvb_split, main-launch waves
FORMS = {
    "two_launch": (0, 0, 0, True, 4),
    "two_launch_w4": (0, 4, 2, True, 4),
    "two_launch_w8": (0, 8, 4, True, 8),
    "two_launch_w16": (0, 16, 4, True, 16),
    "serial_growth": (128, 0, 0, True, 4),       # ISINGMC_CFG_RVB_SERIAL_GROWTH
    "fused": (2048, 0, 0, False, None),          # ISINGMC_CFG_RVB_FUSED
    "global_tables": (4096, 0, 0, False, None),  # ISINGMC_CFG_RVB_GLOBAL_TABLES
}
LOUD_FORMS = ["two_launch", "serial_growth", "fused", "global_tables"]
FLAG_RVB = 8


def check_forms():
    import isingmontecarlo_amd as im
    assert (im.CFG_RVB_SERIAL_GROWTH, im.CFG_RVB_FUSED, im.CFG_RVB_GLOBAL_TABLES, im.FLAG_RVB) == (128, 2048, 4096, FLAG_RVB)


def pair_of(oracle, case, form):
    cfg, waves, k, _, _ = FORMS[form]
    return make_pair(oracle, case["edges"], case["gamma"], case["h"], case["cutoff"], case["cap"], case["seed"], case["R"], waves=waves, k=k,
                     cfg_flags=cfg, nvars=case["nvars"])


def device_step(g, step, beta):
    """The device's side of _rvb_cases.oracle_step: the per-replica results, or None."""
    kind = step[0]
    if kind == "cluster":
        return list(g.single_cluster_step(flip_free=False))
    if kind == "loop":
        return list(g.loop_update())
    if kind == "rvb":
        succ, upd = g.single_rvb_sweep(step[1])
        assert upd == rc.attempts_of(step, g.nvars)
        return list(succ)
    if kind == "diag":
        g.single_diagonal_step(beta)
    elif kind == "free":
        g.flip_free_spins()
    elif kind == "run":
        g.run(step[1], beta, sampling_freq=2, flags=step[2])
    else:
        assert kind == "step_rvb", step
        g.run(1, beta, sampling_freq=2, flags=FLAG_RVB)
    return None


def both_step(g, reps, step, beta, what):
    got, want = device_step(g, step, beta), rc.oracle_step(reps, step, beta)
    if step[0] != "step_rvb":  # (a whole timestep returns nothing on the device)
        assert (None if got is None else [int(x) for x in got]) == (None if want is None else [int(x) for x in want]), f"{what}: results differ"
    assert_same(g, reps, what)


def check_info(g, form):
    _, _, _, split, main_waves = FORMS[form]
    info = g.launch_info()
    assert info["rvb_split"] == split, info
    assert info["rvb_global_tables"] == (form == "global_tables"), info
    if split:
        assert info["rvb_main_waves"] == main_waves, info


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", [n for n in rc.PASSING if n not in rc.TIMESTEPS])
def test_working_set_inside_the_caps(oracle, name, form):
    """Every primitive of the case's program — diagonal step, RVB sweep, cluster step, free spins — compared as soon as it ran:
    successes and cluster counts, n, cutoff, epoch, states and op words."""
    check_forms()
    case = rc.BY_NAME[name]
    g, m, reps = pair_of(oracle, case, form)
    for si, step in enumerate(case["program"]):
        both_step(g, reps, step, case["beta"], f"{name} {form} step {si} {step}")
    assert g.verify().all()
    check_info(g, form)


@pytest.mark.parametrize("fused_launch", [False, True], ids=["split_launches", "fused_launch"])
@pytest.mark.parametrize("name", rc.TIMESTEPS)
def test_working_set_inside_whole_timesteps(oracle, name, fused_launch):
    """run(..., flags = FLAG_RVB) on the seeded lattice (a cluster of 18) and on the star of 129 leaves (hundreds of regrown
    attempts): the sweep as a launch of its own between the diagonal and the cluster launch, and inside the one-launch timestep."""
    import isingmontecarlo_amd as im
    case = rc.BY_NAME[name]
    steps = len(case["program"])
    g, m, reps = make_pair(oracle, case["edges"], case["gamma"], case["h"], case["cutoff"], case["cap"], case["seed"], case["R"],
                           cfg_flags=im.CFG_FUSED_LAUNCH if fused_launch else 0, nvars=case["nvars"])
    g.run(steps, case["beta"], sampling_freq=1, flags=FLAG_RVB)
    for rep in reps:
        rep.timesteps(steps, case["beta"], 1, FLAG_RVB)
    assert_same(g, reps, f"{name} timesteps")
    acc = g.accumulators()
    for r, rep in enumerate(reps):
        assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), (name, r)
    assert g.verify().all()
    assert g.launch_info()["split_launches"] == (not fused_launch)


@pytest.mark.parametrize("form", LOUD_FORMS)
@pytest.mark.parametrize("name", rc.LOUD)
def test_working_set_past_a_cap_stops_loudly(oracle, name, form):
    """Bit-exact up to the sweep the oracle names; that sweep raises ECAPACITY (code 7); behind it the failing replicas hold exactly
    their attempts before the first one past the cap, the others their whole sweep (and, in a whole timestep, what follows it)."""
    import isingmontecarlo_amd as im
    check_forms()
    case, an = rc.BY_NAME[name], rc.analyse(oracle, name)
    stop_step, bad, beta = an["sweeps"][an["first_bad"][1]][0], an["bad"], case["beta"]
    g, m, reps = pair_of(oracle, case, form)
    for si, step in enumerate(case["program"][:stop_step]):
        both_step(g, reps, step, beta, f"{name} {form} step {si} {step}")
    check_info(g, form)
    step = case["program"][stop_step]
    upd = rc.attempts_of(step, case["nvars"])
    with pytest.raises(im.IsingMcError) as ei:
        device_step(g, step, beta)
    assert ei.value.code == -3 and "(code 7)" in str(ei.value), str(ei.value)
    if step[0] == "step_rvb":
        rc.oracle_step(reps, ("diag",), beta)
    n, cut, st, ep = g.get_n(), g.get_cutoff(), g.state_ref(), g.get_epoch()
    for r, rep in enumerate(reps):
        rep.rvb_update(bad[r][0] if r in bad else upd)
        if step[0] == "step_rvb" and r not in bad:
            rep.cluster_update(0.5)
            rep.flip_free_spins()
        what = f"{name} {form} behind the stop, replica {r} ({'stopped at attempt %d' % bad[r][0] if r in bad else 'whole sweep'})"
        assert n[r] == rep.n and cut[r] == rep.cutoff, what
        assert np.array_equal(st[r], rep.state()), f"{what}: state differs"
        assert np.array_equal(g.export_ops(r), rep.ops()), f"{what}: op words differ"
        if r not in bad:
            assert ep[r] == rep.epoch, what
