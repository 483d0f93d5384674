"""CPU tests of the imaginary-time folds: tests/_itime_reference.py (the yardstick of tests/test_gpu_itime.py) against the oracle's own
folds and counts and against imaginary_time_fold closures, and the estimators built on the folds (QmcIsingGraph._kubo; sum_all /
cutoff) against exact diagonalisation on oracle replicas (tests/golden/ed_itime.json, written by tests/golden/make_ed_itime.py)."""
import json
import os
import zlib

import numpy as np
import pytest

import _itime_reference as ref
import _lattices as lat

HERE = os.path.dirname(os.path.abspath(__file__))


def _tfim(oracle, edges, gamma, h, beta, cutoff, cap, seed, R, sweeps, flags=0):
    e, j = lat.split(edges)
    nvars = int(np.max(e)) + 1
    m = oracle.Model(nvars, e, j, gamma, h)
    reps = [oracle.Replica(m, cap, cutoff, seed, r, None) for r in range(R)]
    oracle.batch_timesteps(reps, sweeps, [beta] * R, 1, flags)
    return m, reps, ref.tfim_bond_vars(e, nvars, h), np.asarray(e)


def _xxz(oracle, sweeps):
    """The XXZ ring of test_generic_interactions_match_oracle: two-variable off-diagonal ops."""
    n, R, beta, cutoff, cap, seed = 7, 5, 1.5, 8, 1 << 12, 909
    ints = lat.xxz_ring_interactions(n)
    m = oracle.Model.generic(n, ints)
    reps = [oracle.Replica(m, cap, cutoff, seed, r, None) for r in range(R)]
    for rep in reps:
        rep.timesteps(sweeps, beta, 2, oracle.FLAG_LOOP | oracle.FLAG_NO_CLUSTER)
    return m, reps, ref.generic_bond_vars(ints), ints


class _HostGraph:
    """What QmcIsingGraph.imaginary_time_fold asks of a graph, served from an oracle replica (no device)."""

    def __init__(self, rep, nvars, edges=None, interactions=None):
        self._rep, self.nvars = rep, nvars
        self.edges = np.zeros((0, 2), dtype=np.uint32) if edges is None else np.asarray(edges, dtype=np.uint32).reshape(-1, 2)
        if interactions is not None:
            self.interactions = interactions

    def state_ref(self):
        return self._rep.state()[None, :]

    def export_ops(self, r):
        return self._rep.ops()


def _closure_fold(host, fold_fn, init):
    import isingmontecarlo_amd as im
    return im.QmcIsingGraph.imaginary_time_fold(host, fold_fn, init, r=0)


def _check_system(oracle, m, reps, bond_vars, hosts):
    nvars = m.nvars
    singles = [[v] for v in range(nvars)]
    pairs = [[v, (v + 1) % nvars] for v in range(nvars)]
    groups = singles + pairs + [list(range(nvars))]
    flips = np.array([0] * nvars + [1] * nvars + [1 - (nvars & 1)], dtype=np.uint8)  # products of +-1 spins
    sum_all, sum_occ = ref.fold_replicas(reps, bond_vars, groups, flips)
    counts = oracle.batch_bond_counts(oracle.pointers(reps), m.nbonds)
    offdiag = 0
    for r, rep in enumerate(reps):
        ops = rep.ops()
        # the single-variable sums add up to the oracle's fold of the magnetisation
        assert int(sum_all[r, :nvars].sum()) == rep.itime_magnetization()[0], r
        # bond counts
        assert np.array_equal(ref.bond_counts(ops, m.nbonds), counts[r]) and int(counts[r].sum()) == rep.n, r
        # closures through the package's host-side fold
        spin = lambda st, v: 2 * int(st[v]) - 1
        for g in (0, nvars - 1, nvars, 2 * nvars - 1, 2 * nvars):
            value = lambda st, g=g: int(np.prod([spin(st, v) for v in groups[g]]))
            assert _closure_fold(hosts[r], lambda acc, st: acc + value(st), 0) == int(sum_all[r, g]), (r, g)
        # ... and over the occupied slots: the closure counts slots itself
        def occupied(acc, st, ops=ops, g=nvars):
            p, tot = acc
            return p + 1, tot + (spin(st, groups[g][0]) * spin(st, groups[g][1]) if ops[p] else 0)
        assert _closure_fold(hosts[r], occupied, (0, 0))[1] == int(sum_occ[r, nvars]), r
        assert (np.abs(sum_all[r]) <= rep.cutoff).all() and (np.abs(sum_occ[r]) <= rep.n).all()
        offdiag += sum(1 for w in ops if w and (int(w) & 3) != ((int(w) >> 2) & 3))
    assert offdiag > 0  # (the folds saw observables change)
    return sum_all, sum_occ


def test_reference_fold_on_the_8x8_ferromagnet(oracle):
    m, reps, bv, e = _tfim(oracle, lat.two_d_ferro(8), 1.0, 0.0, 3.0, 64, 1 << 13, 99, 3, 25)
    _check_system(oracle, m, reps, bv, [_HostGraph(rep, m.nvars, e) for rep in reps])


def test_reference_fold_with_a_longitudinal_field(oracle):
    m, reps, bv, e = _tfim(oracle, lat.one_d_periodic(6, -1.0), 1.0, 0.3, 2.0, 6, 1 << 11, 2718, 4, 40)
    assert m.nbonds == 18 and len(bv) == 18
    sum_all, _ = _check_system(oracle, m, reps, bv, [_HostGraph(rep, m.nvars, e) for rep in reps])
    assert any(rep.bond_count(b) for rep in reps for b in range(12, 18))  # longitudinal ops are there


def test_reference_fold_on_two_variable_offdiagonal_ops(oracle):
    m, reps, bv, ints = _xxz(oracle, 60)
    two = sum(1 for rep in reps for w in rep.ops() if w and ((int(w) ^ (int(w) >> 2)) & 3) == 3)
    assert two > 0  # ops that flip both of their variables
    _check_system(oracle, m, reps, bv, [_HostGraph(rep, m.nvars, interactions=ints) for rep in reps])


# ---- the estimators against exact diagonalisation, on the oracle ----
with open(os.path.join(HERE, "golden", "ed_itime.json")) as f:
    ED_ITIME = json.load(f)
with open(os.path.join(HERE, "golden", "ed_tfim.json")) as f:
    ED_TFIM = {c["name"]: c for c in json.load(f)}
Z_POINT = 4.5
ED_REPLICAS, ED_WARMUP, ED_SAMPLES, ED_EVERY = 32, 200, 500, 2


def test_ed_file_is_what_its_generator_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ed_itime", os.path.join(HERE, "golden", "make_ed_itime.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert [(c["name"], c["beta"]) for c in ED_ITIME] == gen.POINTS
    for c in ED_ITIME:
        assert [g["vars"] for g in c["groups"]] == gen.GROUPS
        case = next(x for x in gen.CASES if x["name"] == c["name"])
        hmat, sz = gen.hamiltonian(case["n"], case["edges"], case["gamma"], case["h"])
        evals, evecs = np.linalg.eigh(hmat)
        for g in c["groups"]:
            mean, chi = gen.kubo(evals, evecs, np.prod(sz[g["vars"]], axis=0), c["beta"])
            assert mean == pytest.approx(g["mean"], abs=1e-10) and chi == pytest.approx(g["chi"], abs=1e-10)
            assert 0.0 < g["chi"] <= c["beta"] + 1e-12 and g["chi"] >= c["beta"] * g["mean"] ** 2 - 1e-12
        # a single spin without a transverse field would give chi = beta; here it is strictly less
        assert c["groups"][0]["chi"] < c["beta"]


@pytest.mark.parametrize("point", ED_ITIME, ids=[c["name"] for c in ED_ITIME])
def test_estimators_match_ed_on_the_oracle(oracle, point):
    """itime_average and both forms of itime_susceptibility, evaluated from the reference fold of oracle replicas, against the
    spectrum: |z| < 4.5 per group and estimator, z from the spread over independent replicas."""
    import isingmontecarlo_amd as im
    case, beta = ED_TFIM[point["name"]], point["beta"]
    offset = sum(abs(j) for j in case["J"]) + case["nvars"] * (case["gamma"] + abs(case["h"]))
    cutoff = int(2.0 * beta * (offset - point["energy"])) + 64  # never grows (tests/test_gpu_ed_statistics.py)
    m = oracle.Model(case["nvars"], case["edges"], case["J"], case["gamma"], case["h"])
    seed = zlib.crc32(f"itime|{point['name']}|{beta}".encode())
    reps = [oracle.Replica(m, cutoff, cutoff, seed, r, None) for r in range(ED_REPLICAS)]
    bv = ref.tfim_bond_vars(case["edges"], case["nvars"], case["h"])
    groups = [g["vars"] for g in point["groups"]]
    flips = np.array([1 - (len(g) & 1) for g in groups], dtype=np.uint8)
    betas = [beta] * ED_REPLICAS
    oracle.batch_timesteps(reps, ED_WARMUP, betas)
    acc = {k: np.zeros((ED_REPLICAS, len(groups))) for k in ("mean", "chi_occ", "chi_all")}
    for _ in range(ED_SAMPLES):
        oracle.batch_timesteps(reps, ED_EVERY, betas)
        sum_all, sum_occ = ref.fold_replicas(reps, bv, groups, flips)
        n = np.array([rep.n for rep in reps])
        acc["mean"] += sum_all / float(cutoff)
        acc["chi_occ"] += im.QmcIsingGraph._kubo(sum_occ, n, np.asarray(betas))
        acc["chi_all"] += im.QmcIsingGraph._kubo(sum_all, np.full(ED_REPLICAS, cutoff), np.asarray(betas))
    assert all(rep.cutoff == cutoff for rep in reps)
    bad = []
    for k, exact_key in (("mean", "mean"), ("chi_occ", "chi"), ("chi_all", "chi")):
        x = acc[k] / ED_SAMPLES
        for gi, g in enumerate(point["groups"]):
            mu, se = x[:, gi].mean(), x[:, gi].std(ddof=1) / np.sqrt(ED_REPLICAS)
            z = (mu - g[exact_key]) / se
            print(f"{point['name']} beta={beta} {k} {g['vars']}: {mu:.5f} +- {se:.5f} exact {g[exact_key]:.5f} z={z:+.2f}")
            if not abs(z) < Z_POINT:
                bad.append((k, g["vars"], round(float(z), 2)))
    assert not bad, bad


def test_kubo_estimator_forms():
    import isingmontecarlo_amd as im
    chi = im.QmcIsingGraph._kubo(np.array([[3, -3], [0, 0], [5, 1]]), np.array([3, 0, 5]), np.array([2.0, 2.0, 0.5]))
    assert chi[0, 0] == chi[0, 1] == pytest.approx(2.0 * (9 + 3) / 12)  # a constant observable: beta
    assert (chi[1] == 2.0).all()                                       # an empty string: beta
    assert chi[2, 0] == pytest.approx(0.5) and chi[2, 1] == pytest.approx(0.5 * 6 / 30)
