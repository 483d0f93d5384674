"""The native tempering step against exact diagonalisation (ED) at GPU statistics: every slot of a ladder with swaps switched on
must sample its own temperature's (and its own Hamiltonian's) Gibbs ensemble.

The GPU counterpart of tests/test_tempering_ed_cpu.py, whose docstring has the reasoning, the statistics (z_t per slot, z_lean per
ladder, the chain as the independent unit), the gates (|z_t| < 4.5, |z_lean| < 3.5 for energy, |m|, m^2 and <sigma_x>), the
swap-rate condition (>= 0.3) and the set-up (one sweep then one tempering step, 300 warm-up steps, every replica at the fixed cutoff
of the coldest slot, which must not grow).  The rows, the ED and the statistics are imported from there.  Covered here: the decision
kernel (pt_decide_kernel with pt_accept, the accumulator rows that follow the labels), the host leg of isingmc_pt_step with
pt_bond_count_kernel and pt_relative_weight for per-slot Hamiltonians, and isingmc_pt_decide under the Python TemperingContainer.

Power.  The CPU module shows that six wrong rules reach |z| >= 6 at its statistics.  z grows with the square root of the samples,
and every row here that has a CPU twin runs at least 8 times the twin's chains x measured steps (asserted), so those rules stand
at |z| >= 17 here.  (The 1e-4 energy-shift check of the sweep module is not used: one ladder of six correlated slots does not
reach it, and errors of the swap rule bias at 1e-3 to 1e-2.)

Rows: chains x measured steps, wall time of the test on an MI355X (measured once), swap rate, largest |z_t|, largest |z_lean|.

  row                                          chains x steps  vs CPU twin  wall s  swap rate  max |z_t|  max |z_lean|
  device decisions, a_ring4_afm                   4096 x 2000      26.7       4.7     0.608      1.58       1.16
  device decisions, b_ring6_fm_long               4096 x 2000      10.0       5.0     0.427      1.85       1.23
  device decisions, villain_ladder (12 temps)     2048 x 2000        -        5.6     0.420      1.77       0.68
  device decisions, a_ring4_afm, loop             2048 x 2000      13.3       2.7     0.608      1.32       0.98
  device decisions, a_ring4_afm, rvb              2048 x 2000      13.3       5.2     0.608      1.30       1.00
  device decisions, a_ring4_afm, heatbath         2048 x 2000      13.3       2.6     0.608      2.80       1.27
  host decisions, b_ring6_fm_long                 2048 x 3300       8.3       5.4     0.427      1.49       0.44
  per-slot Hamiltonians, c_ring4_hams             2048 x 1300       8.7       4.2     0.517      2.36       1.61
  per-slot Hamiltonians, c_ring4_hams_common_beta 2048 x 1300        -        4.2     0.802      1.99       1.83
  per-slot Hamiltonians, ring6_hams               2048 x 1300        -        7.5     0.606      1.47       1.10
  Python container, a_ring4_afm                   2048 x 2000      13.3       2.9     0.608      2.87       1.49

The device rows started at 4096 chains x 4000 steps, where they passed as well (a_ring4_afm 8.6 s, max |z_t| 1.88, max |z_lean| 0.37;
b_ring6_fm_long 9.3 s, 1.57, 1.45; villain_ladder 20.6 s, 2.30, 0.66); they were cut to keep every test near 5 s.  A step costs about 1 ms
of wall time whatever the batch holds (one sweep call, which ends by reading the error flags back, and one decision launch), so the
wall time follows the steps, not the chains.  The whole module takes 51 s.
"""
import time

import numpy as np
import pytest

import test_tempering_ed_cpu as cpu
from test_gpu_ed_statistics import OBS, SYSTEMS, capacity_for, seed_of
from test_tempering_ed_cpu import WARMUP, check_ladder, exact_of, ladder_statistics, slot_arrays, slot_offset, start_cutoff

pytestmark = pytest.mark.gpu

FLAG_LOOP, FLAG_HEATBATH, FLAG_RVB = 1, 4, 8
POWER_RATIO = 8  # over the CPU twin's chains x measured steps

# row id -> (slots, CPU twin or None, chains, measured steps)
DEVICE_ROWS = {
    "a_ring4_afm": (cpu.ring4_afm, "a_ring4_afm", 4096, 2000),
    "b_ring6_fm_long": (cpu.ring6_fm_long, "b_ring6_fm_long", 4096, 2000),
    "villain_ladder": (cpu.villain_ladder, None, 2048, 2000),  # (12 temperatures, tests/test_tempering_ed_cpu.py:VILLAIN_TEMPERATURES)
}
RULE_ROWS = {"loop": FLAG_LOOP, "rvb": FLAG_RVB, "heatbath": FLAG_HEATBATH}  # on row (a)
QUARTER = (2048, 2000)  # a quarter of 4096 x 4000, where the device rows started (see the docstring)
HOST_ROW = ("b_ring6_fm_long", 2048, 3300)  # (2048 x 2000 would fall short of 8 times the CPU twin)
HAMS_ROWS = {
    "c_ring4_hams": (cpu.ring4_hams, "c_ring4_hams", 2048, 1300),
    "c_ring4_hams_common_beta": (cpu.ring4_hams_common_beta, None, 2048, 1300),
    "ring6_hams": (cpu.ring6_hams, None, 2048, 1300),
}


def assert_power(twin, K, steps):
    if twin is not None:
        _, ck, cs = cpu.ROWS[twin]
        assert K * steps >= POWER_RATIO * ck * cs, f"{K} x {steps} is less than {POWER_RATIO} times the CPU twin's {ck} x {cs}"


def make_graph(row, slots, K, capacity):
    """The batch of a ladder: replica t*K + k starts at slot t*K + k; per-slot Hamiltonians as rows per replica."""
    import isingmontecarlo_amd as im
    s0, R = slots[0], len(slots) * K
    if not cpu.differ(slots):
        edges = [((a, b), j) for a, b, j in s0["edges"]]
        return im.QmcIsingGraph(edges, s0["gamma"], s0["h"], s0["n"], seed_of(row), nreplicas=R, capacity=capacity, device=0)
    _, J, gam, h = slot_arrays(slots, K)
    edges = [((a, b), 0.0) for a, b, _ in s0["edges"]]
    return im.QmcIsingGraph(edges, s0["gamma"], s0["h"], s0["n"], seed_of(row), nreplicas=R, capacity=capacity, device=0,
                            couplings=J, transverse_r=gam, longitudinal_r=h)


def run_native(row, slots, K, steps, flags=0, decisions="device", warmup=WARMUP):
    """The ladder under NativeTemperingContainer on one rank: (z, lean, swap rate).  Asserts the decision path, verify(), that no
    cutoff grew and, with per-slot Hamiltonians, the offsets behind the labels; the sticky error flags raise from timesteps()."""
    import isingmontecarlo_amd as im
    T, exact = len(slots), exact_of(slots)
    cut = start_cutoff(slots, exact)
    betas = np.array([s["beta"] for s in slots])
    g = make_graph(row, slots, K, capacity_for(cut))
    try:
        tc = im.NativeTemperingContainer(g, betas, K, seed_of(row), flags=flags)
        if cpu.differ(slots):
            assert decisions == "host" and not tc.device_decisions  # per-slot Hamiltonians are decided on the host leg
        else:
            assert tc.device_decisions
            if decisions == "host":
                tc.set_device_decisions(False)
        g.set_cutoffs(np.full(g.nreplicas, cut, dtype=np.uint32))
        for _ in range(warmup):
            tc.timesteps(1)
            tc.tempering_step(count_swaps=False)
        g.reset_accumulators()
        swaps0 = tc.get_total_swaps()
        for _ in range(steps):
            tc.timesteps(1)
            tc.tempering_step(count_swaps=False)
        swaps = tc.get_total_swaps() - swaps0
        assert tc.device_decisions == (decisions == "device")
        acc = g.accumulators()
        assert g.verify().all(), "verify() failed after the measured steps"
        grew = np.flatnonzero(g.get_cutoff() != cut)
        assert grew.size == 0, f"cutoffs grew in {grew.size} replicas from {cut}: {g.get_cutoff()[grew[:4]]}"
        slot_of = np.asarray(tc.slot_of)
        assert sorted(slot_of.tolist()) == list(range(T * K)) and not np.array_equal(slot_of, np.arange(T * K))
        if cpu.differ(slots):
            want = np.array([slot_offset(s) for s in slots])[slot_of // K]
            assert np.abs(g.get_offsets() - want).max() < 1e-12, "the Hamiltonian rows did not follow the labels"
    finally:
        g.close()
    assert acc.shape == (T * K, 8) and (acc[:, 1] == steps).all()
    z, lean = ladder_statistics(acc, slots, exact, K)
    return z, lean, swaps / ((T - 1) * K * steps)


def run_row(what, row, slots, K, steps, **kw):
    t0 = time.time()
    z, lean, rate = run_native(row, slots, K, steps, **kw)
    wall = time.time() - t0
    check_ladder(f"{what}: {K} chains x {steps} steps, {wall:.1f} s", z, lean, rate)


def test_thermal_reproduces_the_stored_ed():
    """The ED computed in these tests is the one behind tests/golden/ed_tfim.json: at the betas that the ladders share with the
    stored points (their end points) thermal() gives the stored values."""
    shared = 0
    for make, name in ((cpu.ring6_fm_long, "ring6_fm_long"), (cpu.villain_ladder, "lat3x3_villain")):
        slots = make()
        exact = exact_of(slots)
        for res in SYSTEMS[name]["results"]:
            for s, ex in zip(slots, exact):
                if s["beta"] == res["beta"]:
                    shared += 1
                    for k in OBS:
                        assert ex[k] == pytest.approx(res[k], rel=1e-10, abs=1e-12), (name, res["beta"], k)
    assert shared == 3  # ring6_fm_long at beta = 2; lat3x3_villain at beta = 1 and 4


@pytest.mark.parametrize("row", list(DEVICE_ROWS))
def test_device_decisions_match_ed(row):
    make, twin, K, steps = DEVICE_ROWS[row]
    assert_power(twin, K, steps)
    run_row(f"device decisions, {row}", row, make(), K, steps)


@pytest.mark.parametrize("rule", list(RULE_ROWS))
def test_update_rules_under_tempering_match_ed(rule):
    K, steps = QUARTER
    assert_power("a_ring4_afm", K, steps)
    run_row(f"device decisions, a_ring4_afm, {rule}", f"a_ring4_afm|{rule}", cpu.ring4_afm(), K, steps, flags=RULE_ROWS[rule])


def test_host_decisions_match_ed():
    row, K, steps = HOST_ROW
    assert_power(row, K, steps)
    run_row(f"host decisions, {row}", f"{row}|host", cpu.ROWS[row][0](), K, steps, decisions="host")


@pytest.mark.parametrize("row", list(HAMS_ROWS))
def test_per_slot_hamiltonians_match_their_own_ed(row):
    make, twin, K, steps = HAMS_ROWS[row]
    assert_power(twin, K, steps)
    run_row(f"per-slot Hamiltonians, {row}", row, make(), K, steps, decisions="host")


def test_python_container_over_the_gpu_backend_matches_ed():
    """The label-swapping TemperingContainer (isingmc_pt_decide on gathered operator counts) over a QmcIsingGraph, row (a)."""
    import isingmontecarlo_amd as im
    row, (K, steps) = "a_ring4_afm|python", QUARTER
    assert_power("a_ring4_afm", K, steps)
    slots = cpu.ring4_afm()
    T, exact = len(slots), exact_of(slots)
    cut = start_cutoff(slots, exact)
    t0 = time.time()
    g = make_graph(row, slots, K, capacity_for(cut))
    try:
        tc = im.TemperingContainer(g, [s["beta"] for s in slots], K, seed_of(row))
        g.set_cutoffs(np.full(g.nreplicas, cut, dtype=np.uint32))
        for _ in range(WARMUP):
            tc.timesteps(1)
            tc.tempering_step()
        g.reset_accumulators()
        swaps0 = tc.get_total_swaps()
        for _ in range(steps):
            tc.timesteps(1)
            tc.tempering_step()
        swaps = tc.get_total_swaps() - swaps0
        acc = tc.slot_accumulators()
        assert tc.verify(), "verify() failed after the measured steps"
        grew = np.flatnonzero(g.get_cutoff() != cut)
        assert grew.size == 0, f"cutoffs grew in {grew.size} replicas from {cut}"
    finally:
        g.close()
    assert acc.shape == (T * K, 8) and (acc[:, 1] == steps).all()
    z, lean = ladder_statistics(acc, slots, exact, K)
    check_ladder(f"Python container, a_ring4_afm: {K} chains x {steps} steps, {time.time() - t0:.1f} s", z, lean, swaps / ((T - 1) * K * steps))
