#!/usr/bin/env python3
"""What the isoenergetic cluster moves between copies cost on the device, on two workloads of R = 1024 replicas as 16 groups x 2 copies
x 32 temperatures (beta |J| = 0.2 .. 1.0), spin steps with nspin = N, 50 rounds per call, device events around the whole call:
  villain   the 64 x 64 periodic lattice with the benches' Villain couplings (the workload of tools/bench_classical_overlap.py)
  pmj       the 64 x 64 periodic lattice with couplings +-1 drawn once (one realisation for the batch)
Cluster moves run at every temperature of the ladder.

Three kinds of GPU step, each a child process under its own `timeout` (this parent never opens the GPU; a step that fails ends the run):
  cluster   on one handle per workload, for steps = 1 and 10, five alternating repeats after a warm-up of
              tempering_run(rounds, steps, cluster_moves=True)   rounds x (steps launch, cluster-move launch, tempering launch)
              tempering_run(rounds, steps)                       the same rounds without the moves
            and, for the cluster-move launch alone, tempering_run(rounds, 0, cluster_moves=True) against tempering_run(rounds, 0);
            the mean cluster size per temperature comes from the counts of all those rounds
  plain     tempering_run(rounds, steps) through the C ABI of a given library file, five calls after a warm-up: with --parent-lib
            (a library built from the parent commit) the existing path of this commit's library and the parent's are timed in
            alternating processes, --processes each; the two spreads over the repeats must overlap
  decorrelate  (with --decorrelate; a record, not a gate) on the pmj lattice at the coldest temperature, the rounds the spin-overlap
            series needs to decorrelate (integrated autocorrelation time of Q, summed to the first non-positive lag, averaged over the
            groups), with and without the moves, over --series-rounds rounds of one step after as many of thermalisation
Writes profiles/classical_icm_bench.json.

    python tools/bench_classical_icm.py [--parent-lib PATH] [--decorrelate] [--rounds 50] [--repeats 5] [--out profiles/classical_icm_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

L, GROUPS, COPIES, NTEMPS, SEED = 64, 16, 2, 32, 2024
N, R = L * L, GROUPS * COPIES * NTEMPS
STEPS = (1, 10)
WORKLOADS = ("villain", "pmj")


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "all": [float(x) for x in xs]}


def lattice(workload):
    import _lattices as lat
    if workload == "villain":
        return lat.two_d_periodic(L)
    signs = np.random.default_rng(SEED).integers(0, 2, (L, L, 2)) * 2.0 - 1.0
    return lat.two_d_periodic(L, lambda i, j, d: float(signs[i, j, d]))


def handle(workload):
    import torch
    torch.cuda.is_available()
    import isingmontecarlo_amd as im
    g = im.GraphState(lattice(workload), [0.0] * N, SEED, nreplicas=R)
    g.attach_tempering(np.linspace(0.2, 1.0, NTEMPS))
    g.attach_overlaps(COPIES)
    g.attach_cluster_moves()
    return g


def cluster(a):
    import isingmontecarlo_amd.classical as cl
    g = handle(a.workload)
    kw = dict(nspinupdates=N, kinds=cl.KINDS_SPIN, record=False)
    g.tempering_run(a.warmup, 1, **kw)
    g.tempering_run(a.warmup, 1, cluster_moves=True, **kw)
    g.reset_cluster_moves()
    ms = {s: {"with_moves": [], "without": []} for s in STEPS}
    alone = {"with_moves": [], "without": []}
    for _ in range(a.repeats):
        for steps in STEPS:  # alternating
            g.tempering_run(a.rounds, steps, cluster_moves=True, **kw)
            ms[steps]["with_moves"].append(g.last_kernel_ms() / a.rounds)
            g.tempering_run(a.rounds, steps, **kw)
            ms[steps]["without"].append(g.last_kernel_ms() / a.rounds)
        g.tempering_run(a.rounds, 0, cluster_moves=True, record=False)
        alone["with_moves"].append(g.last_kernel_ms() / a.rounds)
        g.tempering_run(a.rounds, 0, record=False)
        alone["without"].append(g.last_kernel_ms() / a.rounds)
    counts = g.cluster_move_counts()
    rounds = a.repeats * (len(STEPS) + 1) * a.rounds
    assert ((counts["moves"] + counts["empty"]) == rounds).all()
    moves, size_sum = counts["moves"].sum(axis=(0, 1)).astype(np.float64), counts["size_sum"].sum(axis=(0, 1)).astype(np.float64)
    med = {s: {k: float(np.median(v)) for k, v in d.items()} for s, d in ms.items()}
    return {"event_ms_per_round": {f"steps_{s}": {k: spread(v) for k, v in d.items()} for s, d in ms.items()},
            "with_over_without": {f"steps_{s}": med[s]["with_moves"] / med[s]["without"] for s in STEPS},
            "added_ms_per_round": {f"steps_{s}": med[s]["with_moves"] - med[s]["without"] for s in STEPS},
            "steps_0_ms_per_round": {k: spread(v) for k, v in alone.items()},
            "cluster_launch_alone_ms": float(np.median(alone["with_moves"]) - np.median(alone["without"])),
            "items_per_launch": GROUPS * (COPIES // 2) * NTEMPS, "launch_plan": g.cluster_move_plan(),
            "mean_cluster_size_by_temperature": [float(x) for x in size_sum / np.maximum(moves, 1.0)],
            "empty_items": int(counts["empty"].sum())}


def tau_int(x):
    """The integrated autocorrelation time of the series x [rounds], 1/2 + the sum of the normalised autocorrelation up to the first
    non-positive lag, in rounds."""
    x = np.asarray(x, dtype=np.float64) - np.mean(x)
    var = float(np.dot(x, x)) / len(x)
    if var == 0.0:
        return 0.5
    tau = 0.5
    for lag in range(1, len(x) // 2):
        rho = float(np.dot(x[:-lag], x[lag:])) / (len(x) - lag) / var
        if rho <= 0.0:
            break
        tau += rho
    return tau


def decorrelate(a):
    import isingmontecarlo_amd.classical as cl
    out = {}
    for key, on in (("with_moves", True), ("without", False)):
        g = handle("pmj")
        kw = dict(nspinupdates=N, kinds=cl.KINDS_SPIN, cluster_moves=on)
        g.tempering_run(a.series_rounds, 1, record=False, **kw)
        q = g.tempering_run(a.series_rounds, 1, overlaps=True, **kw)["overlap"][:, :, 0, NTEMPS - 1]  # [rounds][G] at the coldest temperature
        taus = [tau_int(q[:, i]) for i in range(GROUPS)]
        out[key] = {"tau_int_rounds": spread(taus), "mean_abs_q": float(np.abs(q).mean() / N)}
        g.close()
    out["series_rounds"] = a.series_rounds
    return out


def plain(a):
    """tempering_run through the C ABI of the library file a.lib: only symbols that the parent commit has as well."""
    import torch
    torch.cuda.is_available()
    import isingmontecarlo_amd as im
    import isingmontecarlo_amd.classical as cl

    lib = C.CDLL(os.path.abspath(a.lib))
    names = ("isingmc_classical_create", "isingmc_classical_destroy", "isingmc_classical_pt_attach", "isingmc_classical_pt_run", "isingmc_classical_last_kernel_ms",
             "isingmc_classical_get_state")
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = im.SYMBOLS[name]
    ed, js, hs = cl._model(lattice(a.workload), [0.0] * N)
    ladder = np.ascontiguousarray(np.linspace(0.2, 1.0, NTEMPS))
    h = C.c_void_p()
    assert lib.isingmc_classical_create(C.byref(cl._config(ed, js, hs, SEED, R)), C.byref(h)) == 0
    assert lib.isingmc_classical_pt_attach(h, NTEMPS, im._ptr(ladder, C.c_double)) == 0
    energy, mag, ms = np.zeros((a.rounds, R)), np.zeros((a.rounds, R), dtype=np.int32), C.c_float(0)

    def run(rounds, steps):
        assert lib.isingmc_classical_pt_run(h, rounds, steps, N, cl.NONE, cl.NONE, cl.KINDS_SPIN, im._ptr(energy, C.c_double), im._ptr(mag, C.c_int32)) == 0
        assert lib.isingmc_classical_last_kernel_ms(h, C.byref(ms)) == 0
        return ms.value / rounds

    run(min(a.warmup, a.rounds), 1)
    out = {f"steps_{s}": [] for s in STEPS}
    for _ in range(a.repeats):
        for s in STEPS:
            out[f"steps_{s}"].append(run(a.rounds, s))
    state = np.zeros((R, N), dtype=np.uint8)
    assert lib.isingmc_classical_get_state(h, 0xFFFFFFFF, im._ptr(state, C.c_uint8)) == 0
    lib.isingmc_classical_destroy(h)
    return {"event_ms_per_round": out, "state_checksum": int(np.packbits(state).astype(np.uint64).sum()), "energy_checksum": float(energy.sum())}


def child(a, step, extra=()):
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(a.rounds), "--warmup", str(a.warmup),
           "--repeats", str(a.repeats), "--series-rounds", str(a.series_rounds)] + list(extra)
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise SystemExit(f"bench_classical_icm: step {step} ended with status {p.returncode}; nothing more is run")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--processes", type=int, default=3, help="processes per library in the comparison with the parent commit")
    ap.add_argument("--parent-lib", default=None, help="libisingmc_hip.so built from the parent commit")
    ap.add_argument("--decorrelate", action="store_true", help="also record the decorrelation of the spin overlap at the coldest temperature")
    ap.add_argument("--series-rounds", type=int, default=4000)
    ap.add_argument("--limit", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classical_icm_bench.json"))
    ap.add_argument("--step", choices=["cluster", "plain", "decorrelate"], default=None, help="(internal) run one GPU step in this process")
    ap.add_argument("--workload", choices=WORKLOADS, default="villain", help="(internal) the lattice of a cluster or plain step")
    ap.add_argument("--lib", default=None, help="(internal) the library file of a plain step")
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps({"cluster": cluster, "plain": plain, "decorrelate": decorrelate}[a.step](a)))
        return
    out = {"lattices": {"villain": f"{L}x{L} periodic, Villain couplings", "pmj": f"{L}x{L} periodic, couplings +-1 drawn once"}, "replicas": R, "groups": GROUPS,
           "copies": COPIES, "temperatures": NTEMPS, "beta_abs_J": [0.2, 1.0], "window": [0, NTEMPS], "nspin": N, "rounds_per_call": a.rounds, "repeats": a.repeats}
    out["cluster_moves"] = {w: child(a, "cluster", ["--workload", w]) for w in WORKLOADS}
    if a.parent_lib:
        from isingmontecarlo_amd import _build
        libs = {"parent": a.parent_lib, "this": _build.LIB}
        runs = {k: [] for k in libs}
        for _ in range(a.processes):
            for k, path in libs.items():  # alternating processes
                runs[k].append(child(a, "plain", ["--lib", path]))
        cmp = {}
        for s in STEPS:
            key = f"steps_{s}"
            cmp[key] = {k: spread([x for r in v for x in r["event_ms_per_round"][key]]) for k, v in runs.items()}
            cmp[key]["this_minus_parent_median"] = cmp[key]["this"]["median"] - cmp[key]["parent"]["median"]
            cmp[key]["spreads_overlap"] = cmp[key]["this"]["min"] <= cmp[key]["parent"]["max"] and cmp[key]["parent"]["min"] <= cmp[key]["this"]["max"]
        cmp["equal_results"] = len({(r["state_checksum"], r["energy_checksum"]) for v in runs.values() for r in v}) == 1
        out["existing_path_against_parent"] = cmp
    else:
        out["existing_path_against_parent"] = "not measured: no --parent-lib given"
    out["decorrelation_at_the_coldest_temperature"] = child(a, "decorrelate") if a.decorrelate else "not measured: no --decorrelate given"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    if a.parent_lib and not all(out["existing_path_against_parent"][f"steps_{s}"]["spreads_overlap"] for s in STEPS):
        raise SystemExit("bench_classical_icm: the plain run of this library and the parent's do not overlap in their spreads")


if __name__ == "__main__":
    main()
