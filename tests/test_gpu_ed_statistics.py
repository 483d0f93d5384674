"""The HIP path against exact diagonalisation (ED) at GPU statistics: every update rule, the kernel paths and per-replica
Hamiltonians, with thousands of independent replicas per point.

The parity modules prove that the kernels restate the CPU oracle bit for bit; they cannot see an error of the sampler itself,
which the oracle and the kernels share.  Here the physics is checked directly: for the systems of tests/golden/ed_tfim.json,
per replica the energy, |m|, m^2 and <sigma_x> of the measured sweeps (accumulator columns 0, 1, 2, 3 and 6, turned into
observables exactly as tests/golden/ed_highstat.py does), z = (mean over replicas - exact) / (std over replicas / sqrt(R)).

Gates (fixed seeds: the test is deterministic):
  * every point and observable: |z| < 4.5;
  * every (rule, configuration, observable) over its points: |sum z| / sqrt(n) < 3.5 -- the test of a lean that all points
    share, which a per-point gate cannot see;
  * power, for the primary rules: shifting every exact energy by a relative 1e-4 moves the energy aggregate by at least 6,
    i.e. the statistics resolve a bias of 1e-4 of E.

Each system runs as one batch that holds all its temperatures (one beta per replica); the seed is a crc32 of the
(system, rule, configuration) id, so no two points share a random stream.  tests/golden/ed_highstat_gpu.py runs the primary
and isolating rows at higher statistics and keeps the record (tests/golden/ed_highstat_gpu.json).

Every replica starts at a cutoff of 2 beta (offset - E) + 64 = 2 <n> + 64, and the test asserts that it never grows.  Growth
needs n > 4/3 <n> + 43: far out of reach on the small points, about 7 std of n above the mean on the largest (lat3x3_fm at
beta = 4: <n> = 184.5, std ~ 15, cutoff 433), so the assertion is also a gate on the tail of n.  The reference grows the
cutoff after every step to max(cutoff, n + n/2) (qmc_ising.rs:786); each growth appends empty slots at the end of the
op-string, and the diagonal updates that follow fill them from the p = 0 state, a transient that holds the energy above its
equilibrium value.  The cutoff tracks the running maximum of n, so growth never quite stops: with the grown cutoff, 100 warm-up
and 1000 measured sweeps put the energy aggregate of every rule 4.7-8.6 high, 1e-4 to 1e-3 relative per point (CPU oracle and
HIP path alike; measured once, not recorded).  A fixed cutoff removes that transient; the warm-up then only has to equilibrate
the sampler itself.

Rules 0 and 1 of the primary rows run as whole timesteps in one launch (CFG_FUSED_LAUNCH), 2.2-2.4 times faster here than the
default geometry (trimmed diagonal kernel + dedicated cluster kernel, two launches per step; kernel time equals wall time, so
steps_per_launch gains nothing).  The parity tests show that every geometry computes the same op-strings bit for bit from the
same seeds, so these rows hold the default geometry's numbers; the kernel-path rows "default" run the default geometry itself.
RVB runs in the default geometry, where the fused launch is only 1.1 times faster.
"""
import json
import os
import time
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ed_tfim.json")) as f:
    # (the systems tagged "degenerate" -- no edges, isolated variables, duplicate edges, star, complete graph -- pin the CPU oracle in
    # tests/test_oracle_cpu.py for the parity tests of tests/test_gpu_shape_edges.py; the rows here keep the regular systems)
    ED = [c for c in json.load(f) if not c.get("degenerate")]
SYSTEMS = {c["name"]: c for c in ED}
OBS = ("energy", "abs_m", "m2", "sx")

FLAG_LOOP, FLAG_NO_CLUSTER, FLAG_HEATBATH, FLAG_RVB = 1, 2, 4, 8
RULES = {0: "metropolis+cluster", 1: "+loop", 8: "+rvb", 4: "heatbath+cluster", 5: "heatbath+loop+cluster",
         FLAG_LOOP | FLAG_NO_CLUSTER: "loop-only", FLAG_RVB | FLAG_NO_CLUSTER: "rvb-only"}
PRIMARY = [0, FLAG_LOOP, FLAG_RVB]
# (FLAG_LOOP | FLAG_NO_CLUSTER is not among them: without the cluster update the directed loop never makes a transverse op
# off-diagonal, test_loop_without_cluster_stays_in_the_classical_sector)
ISOLATING = [FLAG_HEATBATH, FLAG_HEATBATH | FLAG_LOOP, FLAG_RVB | FLAG_NO_CLUSTER]

REPLICAS = 4096  # per point (system, beta)
WARMUP, SWEEPS = 300, 8000
SWEEPS_OF = {FLAG_RVB: 12000}  # (without lat3x3_fm at beta = 4 the RVB row needs ~11000 sweeps for a power of 6)
ISOLATING_REPLICAS, ISOLATING_SWEEPS = 2048, 2000
Z_POINT, Z_AGGREGATE = 4.5, 3.5
POWER_SHIFT, POWER_MIN = 1e-4, 6.0


def uniform_j(case):
    """set_run_rvb needs couplings of one magnitude (qmc_ising.rs:435-447)."""
    return len({abs(j) for j in case["J"]}) == 1


def leaves_out(case, flags):
    """Why a rule is not run on a system (None: it is)."""
    if (flags & FLAG_RVB) and not uniform_j(case):
        return "RVB sweeps need couplings of one magnitude (qmc_ising.rs:435-447)"
    if (flags & FLAG_LOOP) and (flags & FLAG_NO_CLUSTER) and case["gamma"] != 0.0:
        return "not ergodic: a closed loop enters and leaves a one-site op through its two legs, so it never makes one off-diagonal"
    return None


def offset_of(case):
    """The energy offset of the transverse-field Ising model (sum |J| + N Gamma + N |h|: isingmc_get_offset)."""
    return sum(abs(j) for j in case["J"]) + case["nvars"] * (case["gamma"] + abs(case["h"]))


def fixed_cutoff(beta, offset, energy):
    """A cutoff the run never grows: 2 <n> + 64 with <n> = beta (offset - E) (the reference grows to n + n/2)."""
    return int(2.0 * beta * (offset - energy)) + 64


def capacity_for(cutoffs):
    """The op-string capacity of a batch: its largest cutoff, rounded up to a multiple of 256 slots."""
    return -(-int(np.max(cutoffs)) // 256) * 256


def seed_of(*parts):
    """Deterministic seed per (system, rule, configuration, ...): crc32 of the id."""
    return zlib.crc32("|".join(str(p) for p in parts).encode())


def observables(acc, beta, offset, gamma, nvars):
    """Per replica E, |m|, m^2 and <sigma_x> from accumulator rows (columns 0, 1, 2, 3, 6), as tests/golden/ed_highstat.py."""
    acc = np.asarray(acc, dtype=np.float64)
    return {"energy": -(acc[:, 0] / acc[:, 1]) / beta + offset, "abs_m": acc[:, 2] / acc[:, 1] / nvars,
            "m2": acc[:, 3] / acc[:, 1] / nvars ** 2, "sx": acc[:, 6] / acc[:, 1] / (beta * gamma * nvars) - 1.0}


def point(name, beta, obs, exact, **extra):
    """One (system, beta) point: mean, standard error over replicas, exact value and z per observable."""
    row = dict(system=name, beta=beta, R=len(obs["energy"]), **extra)
    for k in OBS:
        x = obs[k]
        mu, se = float(x.mean()), float(x.std(ddof=1) / np.sqrt(len(x)))
        row[k] = dict(mean=mu, se=se, exact=float(exact[k]), z=(mu - exact[k]) / se)
    return row


def run_batch(g, betas, flags, warmup, sweeps, cutoffs):
    """Fix the cutoffs, warm up, reset the accumulators, measure; at the end verify(), the sticky error flags (run() raises on
    any) and that no cutoff grew."""
    cutoffs = np.ascontiguousarray(np.broadcast_to(np.asarray(cutoffs, dtype=np.uint32), (g.nreplicas,)))
    g.set_cutoffs(cutoffs)
    g.run(warmup, betas, flags=flags)
    g.reset_accumulators()
    g.run(sweeps, betas, flags=flags)
    assert g.verify().all(), "verify() failed after the measured sweeps"
    grew = np.flatnonzero(g.get_cutoff() != cutoffs)
    assert grew.size == 0, f"cutoffs grew in {grew.size} replicas: {g.get_cutoff()[grew[:4]]} vs {cutoffs[grew[:4]]}"
    return g.accumulators()[:g.nreplicas]


def measure_system(case, flags, cfg=0, replicas=None, warmup=None, sweeps=None, seed=None):
    """All temperatures of one ED system in one batch on cuda:0; returns one point per beta."""
    import isingmontecarlo_amd as im
    replicas = REPLICAS if replicas is None else replicas
    warmup = WARMUP if warmup is None else warmup
    sweeps = SWEEPS_OF.get(flags, SWEEPS) if sweeps is None else sweeps
    seed = seed_of(case["name"], flags, cfg) if seed is None else seed
    betas = [r["beta"] for r in case["results"]]
    cuts = [fixed_cutoff(r["beta"], offset_of(case), r["energy"]) for r in case["results"]]
    edges = [((a, b), j) for (a, b), j in zip(case["edges"], case["J"])]
    t0 = time.time()
    g = im.QmcIsingGraph(edges, case["gamma"], case["h"], case["nvars"], seed, nreplicas=replicas * len(betas),
                         capacity=capacity_for(cuts), device=0, cfg_flags=cfg)
    try:
        assert g.get_offset() == pytest.approx(offset_of(case))
        bvec = np.repeat(np.asarray(betas, dtype=np.float64), replicas)
        acc = run_batch(g, bvec, flags, warmup, sweeps, np.repeat(cuts, replicas))
        offset, info = g.get_offset(), g.launch_info()
    finally:
        g.close()
    wall = time.time() - t0
    rows = []
    for k, res in enumerate(case["results"]):
        sl = slice(k * replicas, (k + 1) * replicas)
        obs = observables(acc[sl], res["beta"], offset, case["gamma"], case["nvars"])
        rows.append(point(case["name"], res["beta"], obs, res, flags=flags, cfg=cfg, seed=seed, sweeps=sweeps, cutoff=cuts[k],
                          wall_s=wall / len(betas)))
    return rows, info


def measure_rule(flags, cfg=0, systems=None, **kw):
    """Every applicable ED point under one rule and configuration: the points, and the ones left out with the reason."""
    rows, skipped = [], {}
    for case in ED if systems is None else [SYSTEMS[s] for s in systems]:
        why = leaves_out(case, flags)
        if why:
            skipped[case["name"]] = why
            continue
        if flags & FLAG_RVB:
            out = [r for r in case["results"] if (case["name"], r["beta"]) in RVB_LEFT_OUT]
            skipped.update({(case["name"], r["beta"]): RVB_LEFT_OUT[(case["name"], r["beta"])] for r in out})
            case = dict(case, results=[r for r in case["results"] if r not in out])
        rows += measure_system(case, flags, cfg, **kw)[0]
    return rows, skipped


def aggregate(rows):
    """Per observable over the points: n, sum z / sqrt(n), mean z; for the energy also the power against a relative bias
    POWER_SHIFT (how far sum z / sqrt(n) moves when every exact energy moves by POWER_SHIFT * |E|) and the median relative SE."""
    n = len(rows)
    out = {}
    for k in OBS:
        z = np.array([r[k]["z"] for r in rows])
        out[k] = dict(n=n, sum_z_over_sqrt_n=float(z.sum() / np.sqrt(n)), mean_z=float(z.mean()))
    shift = np.array([POWER_SHIFT * abs(r["energy"]["exact"]) / r["energy"]["se"] for r in rows])
    out["energy"]["power"] = float(shift.sum() / np.sqrt(n))
    out["energy"]["median_relative_se"] = float(np.median([r["energy"]["se"] / abs(r["energy"]["exact"]) for r in rows]))
    return out


def table(rows):
    return "\n".join(f"  {r['system']:>18} b={r['beta']:<6g} " + " ".join(f"{k}={r[k]['z']:+.2f}" for k in OBS) for r in rows)


def check(rows, what, power=False):
    """The per-point and aggregate gates (and the power check where asked); prints the z table either way."""
    assert rows, what
    agg = aggregate(rows)
    summary = " ".join(f"{k}:{agg[k]['sum_z_over_sqrt_n']:+.2f}" for k in OBS)
    print(f"\n{what}: {len(rows)} points, sum z/sqrt n {summary}, power {agg['energy']['power']:.2f}, "
          f"median rel. SE {agg['energy']['median_relative_se']:.2e}\n{table(rows)}")
    bad = [(r["system"], r["beta"], k, round(r[k]["z"], 2)) for r in rows for k in OBS if not abs(r[k]["z"]) < Z_POINT]
    assert not bad, f"{what}: points beyond {Z_POINT} sigma of ED: {bad}\n{table(rows)}"
    lean = {k: round(agg[k]["sum_z_over_sqrt_n"], 2) for k in OBS if not abs(agg[k]["sum_z_over_sqrt_n"]) < Z_AGGREGATE}
    assert not lean, f"{what}: a lean shared by the points, |sum z|/sqrt(n) >= {Z_AGGREGATE}: {lean}\n{table(rows)}"
    if power:
        assert agg["energy"]["power"] >= POWER_MIN, \
            f"{what}: statistics too thin to see a relative energy bias of {POWER_SHIFT}: power {agg['energy']['power']:.2f} < {POWER_MIN}"
    return agg


# lat3x3_fm at beta = 4 (3x3 ferromagnet, Gamma = 1, deep in the ordered phase) is left out of the RVB rows and has a test of
# its own, test_rvb_from_the_start_on_the_ordered_lattice.  From the test's start (empty op-string, 300 warm-up sweeps) RVB
# without the cluster update orders it slowly: |m| is 7.0, 4.0, 0.1 and 0.8 sigma below ED in the 2000-sweep blocks that begin
# after 300, 2300, 4300 and 6300 sweeps, and within 0.4 sigma after 20000 (2048 replicas per point); with the cluster update one
# replica of 8192 overshoots to n >= 293 (<n> = 184.5) within the first 25 sweeps and grows its fixed cutoff.
RVB_LEFT_OUT = {("lat3x3_fm", 4.0): "RVB from the test's start relaxes over thousands of sweeps here "
                                    "(test_rvb_from_the_start_on_the_ordered_lattice)"}


# ---- primary rules, with the power check: rules 0 and 1 as whole timesteps in one launch, RVB in the default geometry ----
def primary_cfg(flags):
    import isingmontecarlo_amd as im
    return 0 if flags & FLAG_RVB else im.CFG_FUSED_LAUNCH


@pytest.mark.parametrize("flags", PRIMARY, ids=[RULES[f] for f in PRIMARY])
def test_primary_rule_matches_ed(flags):
    rows, skipped = measure_rule(flags, primary_cfg(flags))
    assert len(rows) >= 16, (len(rows), skipped)
    check(rows, f"flags={flags} ({RULES[flags]})", power=True)


# ---- isolating rules: heat-bath diagonal updates, and the loop / RVB update without the cluster update ----
@pytest.mark.parametrize("flags", ISOLATING, ids=[RULES[f] for f in ISOLATING])
def test_isolating_rule_matches_ed(flags):
    rows, skipped = measure_rule(flags, replicas=ISOLATING_REPLICAS, sweeps=ISOLATING_SWEEPS)
    assert len(rows) >= 16, (len(rows), skipped)
    check(rows, f"flags={flags} ({RULES[flags]})")


@pytest.mark.parametrize("flags", [FLAG_RVB | FLAG_NO_CLUSTER, FLAG_RVB], ids=["rvb-only", "+rvb"])
@pytest.mark.xfail(strict=True, reason="RVB on lat3x3_fm at beta = 4 from an empty op-string: 300 warm-up sweeps are too short "
                                       "without the cluster update (|m| -7.0 sigma), and with it n overshoots and grows the cutoff")
def test_rvb_from_the_start_on_the_ordered_lattice(flags):
    """The point the RVB rows leave out, at the isolating row's statistics and seed (rvb-only), and the first 25 sweeps of the
    primary row's batch (+rvb).  Expected to fail while the cause stays a slow start; it passes if RVB reached equilibrium
    within the rows' warm-up."""
    case = SYSTEMS["lat3x3_fm"]
    if flags == FLAG_RVB:
        measure_system(case, flags, warmup=25, sweeps=1)  # (run_batch: the cutoffs must not grow)
    else:
        rows, _ = measure_system(case, flags, replicas=ISOLATING_REPLICAS, sweeps=ISOLATING_SWEEPS)
        check([r for r in rows if (r["system"], r["beta"]) in RVB_LEFT_OUT], "lat3x3_fm beta=4 rvb-only")


def test_loop_without_cluster_stays_in_the_classical_sector():
    """Why the directed loop has no row of its own: a one-site op has two legs, and a closed loop that passes it toggles both
    (it goes through) or neither (it bounces), so the op stays diagonal.  With the cluster update switched off, the transverse
    ops of a TFIM never turn off-diagonal and <sigma_x> is never sampled; with it, they do.  (Loop and cluster together are
    the primary rule FLAG_LOOP.)"""
    import isingmontecarlo_amd as im
    for name in ("single_bond", "ring8_fm", "ring6_fm_long"):
        case = SYSTEMS[name]
        assert leaves_out(case, FLAG_LOOP | FLAG_NO_CLUSTER)
        res = case["results"][0]
        cut = fixed_cutoff(res["beta"], offset_of(case), res["energy"])
        edges = [((a, b), j) for (a, b), j in zip(case["edges"], case["J"])]
        for flags, want_offdiag in ((FLAG_LOOP | FLAG_NO_CLUSTER, False), (FLAG_LOOP, True)):
            g = im.QmcIsingGraph(edges, case["gamma"], case["h"], case["nvars"], seed_of(name, flags, "sector"), nreplicas=256,
                                 capacity=capacity_for(cut), device=0)
            try:
                run_batch(g, res["beta"], flags, 50, 200, cut)
                _, off = g.count_diagonal_and_off()
                lens = g.loop_update()
            finally:
                g.close()
            assert lens.max() > 1, (name, flags)  # (the loops do run)
            assert (off.sum() > 0) == want_offdiag, (name, flags, off[:16])


# ---- kernel paths: the general kernels, fused launches, tables in HBM, the RVB variants; a subset of the points ----
PATH_SYSTEMS = ["lat3x3_villain", "ring6_fm_long"]  # frustrated +-J lattice, h != 0
PATH_REPLICAS, PATH_SWEEPS = 2048, 1000


def _cfgs():
    import isingmontecarlo_amd as im
    general = im.CFG_NO_FAST_DIAG | im.CFG_NO_LEAN_CLUSTER
    tables = im.CFG_GLOBAL_TABLES | im.CFG_NO_LDS_TABLES  # (tables in HBM need the general bond table)
    return {"default": (0, [0, 1]), "general": (general, [0, 1, 8]), "fused_launch": (im.CFG_FUSED_LAUNCH, [8]),
            "global_tables": (tables, [0, 1]), "global_tables_rvb": (tables | im.CFG_RVB_GLOBAL_TABLES, [8]),
            "rvb_fused": (im.CFG_RVB_FUSED, [8]), "rvb_global_tables": (im.CFG_RVB_GLOBAL_TABLES, [8])}


PATHS = [("default", 0), ("default", 1)] + [("general", f) for f in (0, 1, 8)] + [("fused_launch", 8)] + \
    [("global_tables", 0), ("global_tables", 1), ("global_tables_rvb", 8), ("rvb_fused", 8), ("rvb_global_tables", 8)]


@pytest.mark.parametrize("path,flags", PATHS, ids=[f"{p}-f{f}" for p, f in PATHS])
def test_kernel_path_matches_ed(path, flags):
    cfg = _cfgs()[path][0]
    rows, info = [], None
    for name in PATH_SYSTEMS:
        r, info = measure_system(SYSTEMS[name], flags, cfg, replicas=PATH_REPLICAS, sweeps=PATH_SWEEPS)
        rows += r
        # the configuration reached the kernels it names
        if path == "default":
            assert info["split_launches"] and info["fast_diagonal"], info
        elif path == "general":
            assert not info["fast_diagonal"] and not info["lean_cluster"], info
        elif path == "fused_launch":
            assert not info["split_launches"], info
        elif path.startswith("global_tables"):
            assert info["global_tables"], info
        elif path == "rvb_fused":
            assert not info["rvb_split"], info
        if path in ("global_tables_rvb", "rvb_global_tables"):
            assert info["rvb_global_tables"], info
    check(rows, f"{path} flags={flags}")


# ---- per-replica Hamiltonians: two Hamiltonians on one ring graph in one batch, each group against its own ED ----
@pytest.mark.parametrize("flags", [0, FLAG_LOOP, FLAG_RVB], ids=[RULES[f] for f in (0, FLAG_LOOP, FLAG_RVB)])
def test_per_replica_hamiltonians_match_their_own_ed(flags):
    import isingmontecarlo_amd as im
    a, b = SYSTEMS["ring6_fm_long"], SYSTEMS["ring6_afm_neglong"]
    assert a["edges"] == b["edges"] and a["nvars"] == b["nvars"]
    groups = [(c, res) for c in (a, b) for res in c["results"]]  # (system, beta) per group of replicas
    rp = 2048
    R = rp * len(groups)
    J = np.concatenate([np.tile(np.asarray(c["J"], dtype=np.float64), (rp, 1)) for c, _ in groups])
    gam = np.repeat([c["gamma"] for c, _ in groups], rp).astype(np.float64)
    h = np.repeat([c["h"] for c, _ in groups], rp).astype(np.float64)
    betas = np.repeat([res["beta"] for _, res in groups], rp).astype(np.float64)
    cuts = np.repeat([fixed_cutoff(res["beta"], offset_of(c), res["energy"]) for c, res in groups], rp)
    edges = [((u, v), 0.0) for u, v in a["edges"]]
    g = im.QmcIsingGraph(edges, 1.0, 0.0, a["nvars"], seed_of("per_replica_ring6", flags), nreplicas=R, capacity=capacity_for(cuts),
                         device=0, couplings=J, transverse_r=gam, longitudinal_r=h)
    try:
        acc = run_batch(g, betas, flags, WARMUP, PATH_SWEEPS, cuts)
        offsets = g.get_offsets()
    finally:
        g.close()
    rows = []
    for k, (c, res) in enumerate(groups):
        sl = slice(k * rp, (k + 1) * rp)
        assert np.all(offsets[sl] == pytest.approx(offset_of(c)))
        obs = observables(acc[sl], res["beta"], offsets[sl][0], c["gamma"], c["nvars"])
        rows.append(point(c["name"], res["beta"], obs, res, flags=flags))
    check(rows, f"per-replica Hamiltonians flags={flags}")


# ---- the dense end: few sites, very long operator strings; ED in the test (at most 2^4 states here) ----
def _ed_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ed_golden", os.path.join(HERE, "golden", "make_ed_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DENSE = [  # name, sites, edges (a, b, J), gamma, h, beta: two cases of tests/test_gpu_dense_end.py
    ("ring4_afm_b500", 4, [(i, (i + 1) % 4, 1.0) for i in range(4)], 1.0, 0.0, 500.0),
    ("bond_b800", 2, [(0, 1, 1.0)], 1.0, 0.0, 800.0),
]
DENSE_REPLICAS, DENSE_WARMUP, DENSE_SWEEPS = 2048, 100, 400


@pytest.mark.parametrize("flags", [0, FLAG_LOOP], ids=[RULES[f] for f in (0, FLAG_LOOP)])
def test_dense_end_matches_ed(flags):
    import isingmontecarlo_amd as im
    rows = []
    for name, n, edges, gamma, h, beta in DENSE:
        assert n <= 8
        exact = _ed_module().thermal(n, edges, gamma, h, beta)
        offset = sum(abs(j) for _, _, j in edges) + n * (gamma + abs(h))
        cut = fixed_cutoff(beta, offset, exact["energy"])
        g = im.QmcIsingGraph([((u, v), j) for u, v, j in edges], gamma, h, n, seed_of(name, flags), nreplicas=DENSE_REPLICAS,
                             capacity=capacity_for(cut), device=0)
        try:
            acc = run_batch(g, beta, flags, DENSE_WARMUP, DENSE_SWEEPS, cut)
            info = g.launch_info()
            assert g.get_offset() == pytest.approx(offset)
        finally:
            g.close()
        # the plan sent these replicas to the general cluster kernel (the dedicated one's flip bits do not fit)
        assert not info["lean_cluster"], info
        rows.append(point(name, beta, observables(acc, beta, offset, gamma, n), exact, flags=flags))
    check(rows, f"dense end flags={flags}")
