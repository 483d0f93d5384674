#!/usr/bin/env python3
"""RVB sweeps with their per-variable tables in HBM (ISINGMC_CFG_RVB_GLOBAL_TABLES): two readings, written to --out as one JSON object.

1. BASELINE configs[4]: 32^3 periodic cubic +-J (one realisation per replica), Gamma = 1, h = 0.1, beta = 4, 512 replicas.  Its scan tables
   live in HBM, so RVB sweeps exist there only with the flag.  After --equilibrate timesteps without RVB (cutoff growth, thermalisation) and
   one untimed sweep: ms per standalone RVB sweep ((N+1)/2 attempts per replica, isingmc_rvb_update), median of --sweeps; then verify().
2. A/B at BASELINE configs[2]: 32x32 TFIM, J = -1, Gamma = 1, beta = 16, 1024 replicas.  The same equilibrated batch (same seed) through the
   default RVB form (tables in LDS) and through CFG_RVB_GLOBAL_TABLES; the two must end bit-identical.

usage: python tools/bench_rvb_global.py [--out profiles/r04_rvb_global.json]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # (initialised before the library: see tests/conftest.py)
import _lattices as lat
import isingmontecarlo_amd as im

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r04_rvb_global.json"))
ap.add_argument("--sweeps", type=int, default=5, help="timed RVB sweeps per reading (the median is reported)")
ap.add_argument("--equilibrate", type=int, default=40)
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--skip-cubic", action="store_true")
ap.add_argument("--skip-ab", action="store_true")
a = ap.parse_args()
torch.cuda.is_available()


def sweep(g, errors):
    """One standalone RVB sweep.  A replica whose attempt outgrows the fixed RVB working set (512 sub-variables, 192 candidates per set,
    288 boundary bonds, 80 windows: ECAPACITY, code 7) ends its sweep there; that is recorded, the flag cleared, and the reading goes on."""
    try:
        s, upd = g.single_rvb_sweep()
        return int(s.sum()), upd
    except im.IsingMcError as e:
        if e.code != -3:
            raise
        errors.append(str(e))
        g.clear_errors()
        return None, (g.nvars + 1) // 2


def time_sweeps(g, n, errors):
    """ms of each of n standalone RVB sweeps (wall clock around the blocking call) and the library's own kernel time."""
    wall, kern, succ = [], [], []
    for _ in range(n):
        t0 = time.perf_counter()
        s, upd = sweep(g, errors)
        wall.append(1e3 * (time.perf_counter() - t0))
        kern.append(float(g.last_kernel_ms()[0]))
        succ.append(s)
    return wall, kern, succ, upd


def reading(g, what, n):
    errors = []
    sweep(g, errors)  # untimed: allocates the table scratch on the first sweep with the flag
    wall, kern, succ, upd = time_sweeps(g, n, errors)
    ok = bool(g.verify().all())
    info = g.launch_info()
    return {"what": what, "ms_per_rvb_sweep_median": statistics.median(kern), "ms_kernel": kern, "ms_wall": wall,
            "attempts_per_replica": upd, "successes_per_sweep": succ, "verify": ok, "capacity_errors": errors,
            "rvb_global_tables": info["rvb_global_tables"], "rvb_split": info["rvb_split"], "global_tables": info["global_tables"]}


out = {"tool": "tools/bench_rvb_global.py", "device": torch.cuda.get_device_name(0), "sweeps": a.sweeps, "equilibrate": a.equilibrate}


def save():  # after every reading: a later failure keeps what was measured
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)

if not a.skip_cubic:
    L, R, beta = 32, 512, 4.0
    edges = lat.cubic_periodic(L)
    nsite = L ** 3
    J = np.random.default_rng(a.seed + 7919).choice([-1.0, 1.0], size=(R, len(edges)))
    n_est = beta * (len(edges) * 1.3 + nsite * 1.2)
    cap = 1 << int(np.ceil(np.log2(2.0 * n_est + 4 * nsite)))  # (bench.py --pmj3d 32: 2^21)
    g = im.QmcIsingGraph(edges, 1.0, 0.1, nsite, a.seed, nreplicas=R, capacity=cap, couplings=J, cfg_flags=im.CFG_RVB_GLOBAL_TABLES)
    t0 = time.perf_counter()
    for _ in range(0, a.equilibrate, 10):
        g.run(10, beta, flags=im.FLAG_PREP)
    t_eq = time.perf_counter() - t0
    r = reading(g, f"configs[4]: {L}^3 +-J Gamma=1 h=0.1 beta={beta}, {R} replicas, capacity {cap}", a.sweeps)
    r.update(equilibrate_s=t_eq, n_mean=float(g.get_n().mean()), cutoff_max=int(g.get_cutoff().max()),
             rvb_table_bytes_per_replica=4 * (((nsite + 1) + nsite + (nsite + 1) // 2 + (len(edges) + 1) // 2 + cap + 15) & ~15))
    out["configs4"] = r
    save()
    print(json.dumps({"configs4_ms_per_rvb_sweep": r["ms_per_rvb_sweep_median"], "verify": r["verify"]}), flush=True)
    del g

if not a.skip_ab:
    L, R, beta = 32, 1024, 16.0
    edges = lat.two_d_ferro(L)
    n_est = beta * (3 * L * L + 2.2 * L * L)
    cap = 1 << int(np.ceil(np.log2(2.0 * n_est + 4 * L * L)))  # (bench.py: 2^18)
    ab = {}
    states = {}
    for name, cfg in (("lds_tables", 0), ("hbm_tables", im.CFG_RVB_GLOBAL_TABLES)):
        g = im.QmcIsingGraph(edges, 1.0, 0.0, L * L, a.seed, nreplicas=R, capacity=cap, cfg_flags=cfg)
        for _ in range(0, a.equilibrate, 10):
            g.run(10, beta, flags=im.FLAG_PREP)
        ab[name] = reading(g, f"configs[2]: {L}x{L} J=-1 Gamma=1 beta={beta}, {R} replicas, {name}", a.sweeps)
        states[name] = [g.state_ref().copy(), g.get_n().copy()] + [g.export_ops(r) for r in range(0, R, 97)]
        del g
    same = all(np.array_equal(x, y) for x, y in zip(states["lds_tables"], states["hbm_tables"]))
    ab["identical_results"] = bool(same)
    ab["hbm_over_lds"] = ab["hbm_tables"]["ms_per_rvb_sweep_median"] / ab["lds_tables"]["ms_per_rvb_sweep_median"]
    out["configs2_ab"] = ab
    save()
    print(json.dumps({"configs2_lds_ms": ab["lds_tables"]["ms_per_rvb_sweep_median"], "configs2_hbm_ms": ab["hbm_tables"]["ms_per_rvb_sweep_median"],
                      "identical": same}), flush=True)

print("wrote", a.out)
