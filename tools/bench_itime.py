#!/usr/bin/env python3
"""What the imaginary-time folds cost at the headline model (bench.py's configs[1]: 32x32 ferromagnet, Gamma = 1, beta = 16, 1024
replicas, directed loops on, equilibrated as bench.py does): isingmc_itime_groups for the 3072 site + bond groups, isingmc_bond_counts,
and a timestep of the same batch, in one process.

Two GPU steps, each a child process under its own `timeout` (this parent never opens the GPU; a step that fails ends the run):
  measure   host clock around the blocking calls (they end in a stream synchronise): medians over --reps rounds in which the three
            alternate, after a warm-up of each; ms per timestep also from the library's device events (last_kernel_ms)
  trace     the same calls, twice each, under `rocprofv3 --kernel-trace`: the kernel's own time without the copies around it
The lower bound of a fold is one read of the strings: 4 B per slot over the HBM peak of bench.py.

usage: python tools/bench_itime.py [--out profiles/r14_itime.json]
"""
import argparse, csv, glob, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_itime.json"))
ap.add_argument("--L", type=int, default=32)
ap.add_argument("--replicas", type=int, default=1024)
ap.add_argument("--beta", type=float, default=16.0)
ap.add_argument("--equilibrate", type=int, default=80)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20, help="timesteps per timed run")
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--limit", type=int, default=240, help="seconds each GPU step may take")
ap.add_argument("--no-trace", action="store_true")
ap.add_argument("--step", choices=["measure", "trace"], default=None, help="(internal) run one GPU step in this process")
a = ap.parse_args()
HBM_PEAK_GBS = 8000.0  # bench.py
KERNEL = "itime_kernel"


def child(step, extra=()):
    cmd = ["timeout", "-k", "10", str(a.limit)] + list(extra) + [sys.executable, os.path.abspath(__file__), "--step", step, "--out", a.out]
    for k in ("L", "replicas", "equilibrate", "reps", "steps", "seed"):
        cmd += ["--" + k, str(getattr(a, k))]
    cmd += ["--beta", str(a.beta)]
    print("+", " ".join(cmd), flush=True)
    rc = subprocess.call(cmd)
    if rc != 0:
        raise SystemExit(f"bench_itime: step {step} ended with status {rc}; nothing more is run")


if a.step is None:
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    child("measure")
    if not a.no_trace:
        tdir = tempfile.mkdtemp(prefix="itime_trace_")  # (the trace itself is not kept: two numbers come out of it)
        child("trace", ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tdir, "--"])
        out = json.load(open(a.out))
        files = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
        rows = sorted((r for f in files for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows if KERNEL in r["Kernel_Name"]]
        assert len(ms) == 4, (files, len(ms))  # groups, groups, counts, counts
        out["kernel_ms_rocprofv3"] = {"itime_groups": ms[1], "bond_counts": ms[3], "source": "rocprofv3 --kernel-trace, a run of its own; second of two calls each"}
        out["ratios"]["fold_kernel_over_bound"] = ms[1] / out["bound_ms_4B_per_slot"]
        out["ratios"]["fold_kernel_over_timestep"] = ms[1] / out["timestep_ms"]["device_events"]
        out["ratios"]["bond_counts_kernel_over_bound"] = ms[3] / out["bound_ms_4B_per_slot"]
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(json.load(open(a.out))))
    sys.exit(0)

import numpy as np
import torch  # (initialised before the library: see tests/conftest.py)
import _lattices as lat
import isingmontecarlo_amd as im
from isingmontecarlo_amd.autocorrelations import bond_groups, variable_groups

if not torch.cuda.is_available():
    raise SystemExit("bench_itime.py needs a HIP device (no CPU fallback)")
L, R, beta, flags = a.L, a.replicas, a.beta, im.FLAG_LOOP
edges = lat.two_d_ferro(L)
n_est = beta * (3 * L * L + 2.2 * L * L)
cap = 1 << int(np.ceil(np.log2(2.0 * n_est + 4 * L * L)))
g = im.QmcIsingGraph(edges, 1.0, 0.0, L * L, a.seed, nreplicas=R, capacity=cap)
for _ in range(0, a.equilibrate, 10):
    g.run(min(10, a.equilibrate), beta, flags=flags)
vg, vf = variable_groups(g.nvars)
bg, bf = bond_groups(g)
groups, flips = vg + bg, np.concatenate([vf, bf])

if a.step == "trace":
    for _ in range(2):
        g.itime_groups(groups, flips)
    for _ in range(2):
        g.bond_counts()
    sys.exit(0)


def timed(fn):
    torch.cuda.synchronize(); g.synchronize()
    t0 = time.perf_counter()
    r = fn()
    g.synchronize(); torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


g.run(a.steps, beta, flags=flags); g.itime_groups(groups, flips); g.bond_counts()  # warm-up of the shapes
ms = {"timestep": [], "timestep_events": [], "itime_groups": [], "bond_counts": []}
for _ in range(a.reps):  # the three alternate inside a round
    ms["timestep"].append(timed(lambda: g.run(a.steps, beta, flags=flags))[0] / a.steps)
    ms["timestep_events"].append(g.last_kernel_ms()[0] / a.steps)
    ms["itime_groups"].append(timed(lambda: g.itime_groups(groups, flips))[0])
    ms["bond_counts"].append(timed(lambda: g.bond_counts())[0])
slots = int(g.get_cutoff().astype(np.int64).sum())
sum_all, sum_occ = g.itime_groups(groups, flips)
counts = g.bond_counts()
assert np.array_equal(counts.sum(axis=1), g.get_n()) and (np.abs(sum_all) <= g.get_cutoff()[:, None]).all()
bound_ms = 4.0 * slots / (HBM_PEAK_GBS * 1e9) * 1e3
med = {k: statistics.median(v) for k, v in ms.items()}
res = {"model": f"{L}x{L} ferromagnet Gamma=1 beta={beta}, {R} replicas, FLAG_LOOP (bench.py configs[1])", "groups": len(groups),
       "group_variables": int(sum(len(x) for x in groups)), "bonds": int(g.num_bonds()), "slots_all_replicas": slots,
       "mean_cutoff": slots / R, "mean_n": float(g.get_n().mean()), "reps": a.reps,
       "timestep_ms": {"host_clock": med["timestep"], "device_events": med["timestep_events"], "all": ms["timestep"]},
       "itime_groups_call_ms": {"median": med["itime_groups"], "all": ms["itime_groups"],
                                "note": "whole call: groups up, kernel, 2 x R x G x 8 bytes down into pageable memory"},
       "bond_counts_call_ms": {"median": med["bond_counts"], "all": ms["bond_counts"]},
       "bound_ms_4B_per_slot": bound_ms, "hbm_peak_GBps": HBM_PEAK_GBS,
       "ratios": {"fold_call_over_timestep": med["itime_groups"] / med["timestep_events"], "fold_call_over_bound": med["itime_groups"] / bound_ms,
                  "bond_counts_call_over_timestep": med["bond_counts"] / med["timestep_events"]}}
json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res), flush=True)
