#!/usr/bin/env python3
"""What classical parallel tempering costs on the device: the 64 x 64 periodic lattice with the benches' Villain couplings of
tools/bench_classical.py, R = 1024 replicas as 32 chains of 32 temperatures (beta |J| = 0.2 .. 1.0), spin steps with nspin = N.

For steps = 1 and 10 per round, after a warm-up, five alternating repeats of
  tempering_run(rounds, steps)            rounds x (steps launch, tempering launch), device events around the whole run
  timesteps(rounds * steps)               the same number of steps in one launch on a plain batch: the code path without tempering
  rounds x timesteps(steps)               the same steps in as many launches as the tempering run uses (sum of the launches' events)
and the tempering launch alone (tempering_run(rounds, 0)), the swap acceptance per pair, and the wall-clock time of a tempering run
against the loop it replaces (timesteps + get_energy per sample, one synchronisation and one host copy each).
Writes profiles/classical_pt_bench.json.

    python tools/bench_classical_pt.py [--rounds 50] [--repeats 5] [--out profiles/classical_pt_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classical_pt_bench.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.is_available()
    import isingmontecarlo_amd as im
    import isingmontecarlo_amd.classical as cl
    import _lattices as lat

    L, chains, ntemps, seed = 64, 32, 32, 2024
    N, R = L * L, chains * ntemps
    edges, biases = lat.two_d_periodic(L), [0.0] * N
    ladder = np.linspace(0.2, 1.0, ntemps)
    by_slot = np.tile(ladder, chains)
    pt, plain = im.GraphState(edges, biases, seed, nreplicas=R), im.GraphState(edges, biases, seed, nreplicas=R)
    pt.attach_tempering(ladder)
    kw = dict(nspinupdates=N, kinds=cl.KINDS_SPIN)
    pt.tempering_run(a.warmup, 1, record=False, **kw)
    plain.timesteps(a.warmup, by_slot, **kw)

    ms = {s: {"tempering_run": [], "timesteps_one_launch": [], "timesteps_per_round": []} for s in (1, 10)}
    alone = []
    for _ in range(a.repeats):
        for steps in (1, 10):  # alternating
            pt.tempering_run(a.rounds, steps, record=True, **kw)
            ms[steps]["tempering_run"].append(pt.last_kernel_ms())
            plain.timesteps(a.rounds * steps, by_slot, **kw)
            ms[steps]["timesteps_one_launch"].append(plain.last_kernel_ms())
            total = 0.0
            for _ in range(a.rounds):
                plain.timesteps(steps, by_slot, **kw)
                total += plain.last_kernel_ms()
            ms[steps]["timesteps_per_round"].append(total)
        pt.tempering_run(a.rounds, 0, record=True)
        alone.append(pt.last_kernel_ms() / a.rounds)

    # the wall clock of a recorded series: one call against the loop it replaces
    t0 = time.perf_counter()
    pt.tempering_run(a.rounds, 1, record=True, **kw)
    wall_run = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(a.rounds):
        plain.timesteps(1, by_slot, **kw)
        plain.get_energy()
    wall_loop = time.perf_counter() - t0

    att, acc = pt.swap_counts()
    med = {s: {k: float(np.median(v)) for k, v in d.items()} for s, d in ms.items()}
    step_ms = med[10]["timesteps_one_launch"] / (a.rounds * 10)
    out = {"lattice": f"{L}x{L} periodic, Villain couplings", "replicas": R, "chains": chains, "temperatures": ntemps,
           "beta_abs_J": [float(ladder[0]), float(ladder[-1])], "nspin": N, "rounds_per_call": a.rounds, "repeats": a.repeats,
           "event_ms": {f"steps_{s}": {k: [float(x) for x in v] for k, v in d.items()} for s, d in ms.items()},
           "median_ms": {f"steps_{s}": d for s, d in med.items()},
           "tempering_run_over_timesteps_one_launch": {f"steps_{s}": med[s]["tempering_run"] / med[s]["timesteps_one_launch"] for s in med},
           "tempering_run_over_timesteps_per_round": {f"steps_{s}": med[s]["tempering_run"] / med[s]["timesteps_per_round"] for s in med},
           "tempering_launch_alone_ms": [float(x) for x in alone], "tempering_launch_alone_median_ms": float(np.median(alone)),
           "one_step_ms": step_ms, "tempering_launch_over_one_step": float(np.median(alone)) / step_ms,
           "wall_s": {"tempering_run_recorded": wall_run, "timesteps_and_get_energy_loop": wall_loop},
           "swap_acceptance_per_pair": [float(x) for x in acc.sum(axis=0) / att.sum(axis=0)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
