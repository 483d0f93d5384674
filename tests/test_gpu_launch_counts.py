"""GPU test of the sweep driver's launch plan: for every kind of call, the launches it reports (last_kernel_ms), how they fall
into the diagonal bucket and the other one (last_pass_ms) and how many of them were RVB sweeps of their own (last_rvb_ms).  The
numbers are the table of DESIGN.md section 5.  One small model throughout: the results are pinned by the parity tests; this file
pins which launches produce them."""
import numpy as np
import pytest

import _lattices as lat
import isingmontecarlo_amd as im

pytestmark = pytest.mark.gpu

T = 20
R = 3
BETA = 1.0
RVB, LOOP, NO_CLUSTER = im.FLAG_RVB, im.FLAG_LOOP, im.FLAG_NO_CLUSTER
FUSED, RVB_G = im.CFG_FUSED_LAUNCH, im.CFG_RVB_GLOBAL_TABLES


def batch(cfg=0):
    """4x4 periodic lattice, uniform J, Gamma = 1"""
    return im.QmcIsingGraph(lat.two_d_ferro(4), 1.0, 0.0, 16, 2024, nreplicas=R, capacity=4096, cfg_flags=cfg)


def counts(g):
    """(launches, (diagonal launches, other launches), RVB launches) of the last call"""
    c = g.last_kernel_ms()[1], g.last_pass_ms()[1], g.last_rvb_ms()[1]
    print("counts", c)
    return c


# name -> (config flags, update flags, steps per launch or None, (launches, (diagonal, other), RVB))
TIMESTEPS = {
    "default": (0, 0, None, (2 * T, (T, T), 0)),
    "no_cluster": (0, NO_CLUSTER, None, (2 * T, (T, T), 0)),
    "rvb": (0, RVB, None, (3 * T, (T, 2 * T), T)),
    "rvb_loop": (0, RVB | LOOP, None, (2 * T, (T, T), 0)),
    "rvb_loop_tables_in_hbm": (RVB_G, RVB | LOOP, None, (3 * T, (T, 2 * T), T)),
    "fused": (FUSED, 0, None, (1, (0, 1), 0)),
    "fused_7_steps_per_launch": (FUSED, 0, 7, (3, (0, 3), 0)),
    "fused_rvb_tables_in_hbm": (FUSED | RVB_G, RVB, None, (3 * T, (0, 3 * T), 0)),
}


@pytest.mark.parametrize("name", list(TIMESTEPS))
def test_launches_of_timesteps(name):
    cfg, flags, spl, want = TIMESTEPS[name]
    g = batch(cfg)
    if spl is not None:
        g.set_steps_per_launch(spl)
    g.run(T, BETA, flags=flags)
    assert counts(g) == want
    assert g.verify().all()
    g.close()


def test_launches_of_fused_timesteps_end_on_sampled_steps_under_a_record():
    """7 steps per launch, but every launch ends on the next sampled step: six launches of 3 steps and one of the last 2.  The six
    recorded rows equal those of the split path."""
    rows = []
    for cfg, spl, want in ((FUSED, 7, (7, (0, 7), 0)), (0, None, (2 * T, (T, T), 0))):
        g = batch(cfg)
        if spl is not None:
            g.set_steps_per_launch(spl)
        g.attach_sample_record(T // 3)
        g.run(T, BETA, sampling_freq=3)
        assert counts(g) == want
        assert g.record_count() == 6
        rows.append(g.record_states())
        g.close()
    assert rows[0].shape == (6, R, 16)
    assert np.array_equal(rows[0], rows[1])


SINGLE = {
    "diagonal_update": lambda g: g.single_diagonal_step(BETA),
    "cluster_update": lambda g: g.single_cluster_step(flip_free=False),
    "loop_update": lambda g: g.loop_update(),
    "rvb_update": lambda g: g.single_rvb_sweep(),
    "flip_free_spins": lambda g: g.flip_free_spins(),
}


@pytest.mark.parametrize("name", list(SINGLE))
def test_launches_of_single_updates(name):
    """One launch each, in the other bucket: except that a lone diagonal update of a batch with split launches is that batch's
    diagonal launch (and nothing behind it), and counts as one."""
    g = batch()
    g.run(T, BETA)  # (an op-string to work on)
    SINGLE[name](g)
    assert counts(g) == (1, (1, 0) if name == "diagonal_update" else (0, 1), 0)
    assert g.verify().all()
    g.close()


def test_counts_and_pass_times_beyond_the_timed_steps():
    """300 split timesteps: events cover the first 256, the per-pass times are scaled up to the run; the counts are not estimates."""
    t = 300
    g = batch()
    g.run(T, BETA)  # (kernels loaded: the events of the first steps do not time the loader)
    g.run(t, BETA)
    assert counts(g) == (2 * t, (t, t), 0)
    total, (diag_ms, other_ms) = g.last_kernel_ms()[0], g.last_pass_ms()[0]
    print("ms", total, diag_ms, other_ms)
    assert diag_ms > 0 and other_ms > 0
    assert diag_ms + other_ms <= total
    g.close()
