"""The imaginary-time estimators on the HIP path against exact diagonalisation at GPU statistics: <O_g> from itime_average and the
Kubo susceptibility chi_g from both forms of itime_susceptibility (occupied slots, all slots), for the points and groups of
tests/golden/ed_itime.json (tests/golden/make_ed_itime.py).

Per point 4096 replicas run whole timesteps in one launch (CFG_FUSED_LAUNCH, as the primary rows of tests/test_gpu_ed_statistics.py)
at a fixed cutoff of 2 beta (offset - E) + 64 that must not grow; 300 warm-up sweeps, then timesteps_measure_itime takes 200 samples 5
sweeps apart.  z = (mean over replicas - exact) / (std over replicas / sqrt(R)).  Gates, as in that file: |z| < 4.5 per point and
|sum z| / sqrt(n) < 3.5 per estimator over its points."""
import json
import os

import numpy as np
import pytest

from test_gpu_ed_statistics import SYSTEMS, Z_AGGREGATE, Z_POINT, capacity_for, fixed_cutoff, offset_of, seed_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ed_itime.json")) as f:
    POINTS = json.load(f)
REPLICAS, WARMUP, SAMPLES, EVERY = 4096, 300, 200, 5
ESTIMATORS = (("average", "mean"), ("chi_occupied", "chi"), ("chi_all", "chi"))


def measure(point):
    import isingmontecarlo_amd as im
    case, beta = SYSTEMS[point["name"]], point["beta"]
    cut = fixed_cutoff(beta, offset_of(case), point["energy"])
    edges = [((a, b), j) for (a, b), j in zip(case["edges"], case["J"])]
    groups = [g["vars"] for g in point["groups"]]
    flips = np.array([1 - (len(g) & 1) for g in groups], dtype=np.uint8)  # products of +-1 spins
    g = im.QmcIsingGraph(edges, case["gamma"], case["h"], case["nvars"], seed_of("itime", point["name"], beta), nreplicas=REPLICAS,
                         capacity=capacity_for(cut), device=0, cfg_flags=im.CFG_FUSED_LAUNCH)
    try:
        cuts = np.full(REPLICAS, cut, dtype=np.uint32)
        g.set_cutoffs(cuts)
        g.run(WARMUP, beta)
        res = g.timesteps_measure_itime(SAMPLES * EVERY, beta, groups, sampling_freq=EVERY, flips=flips)
        assert g.verify().all()
        assert np.array_equal(g.get_cutoff(), cuts), "cutoffs grew"
    finally:
        g.close()
    rows = []
    for (est, key), x in zip(ESTIMATORS, res):
        for gi, grp in enumerate(point["groups"]):
            mu, se = float(x[:, gi].mean()), float(x[:, gi].std(ddof=1) / np.sqrt(REPLICAS))
            rows.append(dict(system=point["name"], beta=beta, estimator=est, vars=grp["vars"], mean=mu, se=se, exact=grp[key], z=(mu - grp[key]) / se))
    return rows


def test_estimators_match_ed():
    rows = [r for p in POINTS for r in measure(p)]
    bad, lean = [], {}
    for est, _ in ESTIMATORS:
        mine = [r for r in rows if r["estimator"] == est]
        z = np.array([r["z"] for r in mine])
        agg = float(z.sum() / np.sqrt(len(z)))
        print(f"\n{est}: {len(mine)} points, sum z / sqrt n = {agg:+.2f}")
        for r in mine:
            print(f"  {r['system']:>14} b={r['beta']:<4g} {str(r['vars']):<10} {r['mean']:+.6f} +- {r['se']:.6f} exact {r['exact']:+.6f} z={r['z']:+.2f}")
        bad += [(est, r["system"], r["vars"], round(r["z"], 2)) for r in mine if not abs(r["z"]) < Z_POINT]
        if not abs(agg) < Z_AGGREGATE:
            lean[est] = round(agg, 2)
    assert len(rows) == 3 * 10
    assert not bad, f"points beyond {Z_POINT} sigma of ED: {bad}"
    assert not lean, f"a lean shared by the points, |sum z| / sqrt(n) >= {Z_AGGREGATE}: {lean}"
