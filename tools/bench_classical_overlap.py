#!/usr/bin/env python3
"""What measuring the overlaps between copies costs on the device: the 64 x 64 periodic lattice with the benches' Villain couplings
of tools/bench_classical_pt.py, R = 1024 replicas as 16 groups x 2 copies x 32 temperatures (beta |J| = 0.2 .. 1.0), spin steps with
nspin = N, 50 rounds per call, device events around the whole call.

Two kinds of GPU step, each a child process under its own `timeout` (this parent never opens the GPU; a step that fails ends the run):
  measure   on one handle, for steps = 1 and 10, five alternating repeats after a warm-up of
              tempering_run(rounds, steps, overlaps=True)    rounds x (steps launch, overlap launch, tempering launch)
              tempering_run(rounds, steps)                   the same rounds without the measurement
            and, for the overlap launch alone, tempering_run(rounds, 0, overlaps=True) against tempering_run(rounds, 0);
            the histograms are checked against the recorded series on the way
  plain     tempering_run(rounds, steps) through the C ABI of a given library file, five calls after a warm-up: with --parent-lib
            (a library built from the parent commit) the existing path of this commit's library and the parent's are timed in
            alternating processes, --processes each
Writes profiles/classical_overlap_bench.json.

    python tools/bench_classical_overlap.py [--parent-lib PATH] [--rounds 50] [--repeats 5] [--out profiles/classical_overlap_bench.json]
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


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "all": [float(x) for x in xs]}


def measure(a):
    import torch
    torch.cuda.is_available()
    import isingmontecarlo_amd as im
    import isingmontecarlo_amd.classical as cl
    import _lattices as lat

    edges, ladder = lat.two_d_periodic(L), np.linspace(0.2, 1.0, NTEMPS)
    g = im.GraphState(edges, [0.0] * N, SEED, nreplicas=R)
    g.attach_tempering(ladder)
    g.attach_overlaps(COPIES)
    kw = dict(nspinupdates=N, kinds=cl.KINDS_SPIN)
    g.tempering_run(a.warmup, 1, record=False, **kw)
    g.tempering_run(a.warmup, 1, record=False, overlaps=True, **kw)
    g.reset_overlaps()
    ms = {s: {"with_overlaps": [], "without": []} for s in STEPS}
    alone = {"with_overlaps": [], "without": []}
    series = []
    for _ in range(a.repeats):
        for steps in STEPS:  # alternating
            series.append(g.tempering_run(a.rounds, steps, overlaps=True, **kw)["overlap"])
            ms[steps]["with_overlaps"].append(g.last_kernel_ms())
            g.tempering_run(a.rounds, steps, **kw)
            ms[steps]["without"].append(g.last_kernel_ms())
        series.append(g.tempering_run(a.rounds, 0, overlaps=True)["overlap"])
        alone["with_overlaps"].append(g.last_kernel_ms() / a.rounds)
        g.tempering_run(a.rounds, 0)
        alone["without"].append(g.last_kernel_ms() / a.rounds)
    hq, hl = g.overlap_histograms()
    nq = (N - np.concatenate(series).astype(np.int64)) // 2  # every measured round is in a series: the histogram is their bincount
    assert (hq.sum(axis=3) == len(nq)).all() and (hl.sum(axis=3) == len(nq)).all()
    assert all(np.array_equal(hq[i, 0, t], np.bincount(nq[:, i, 0, t], minlength=N + 1)) for i in range(GROUPS) for t in (0, NTEMPS - 1))
    med = {s: {k: float(np.median(v)) for k, v in d.items()} for s, d in ms.items()}
    launch = float(np.median(alone["with_overlaps"]) - np.median(alone["without"]))
    m = g.overlap_moments()
    return {"event_ms_per_call": {f"steps_{s}": {k: spread(v) for k, v in d.items()} for s, d in ms.items()},
            "with_over_without": {f"steps_{s}": med[s]["with_overlaps"] / med[s]["without"] for s in STEPS},
            "added_ms_per_round": {f"steps_{s}": (med[s]["with_overlaps"] - med[s]["without"]) / a.rounds for s in STEPS},
            "steps_0_ms_per_round": {k: spread(v) for k, v in alone.items()},
            "overlap_launch_alone_ms": launch, "items_per_launch": GROUPS * NTEMPS,
            "overlap_launch_bytes_read": GROUPS * NTEMPS * (2 * N // 8 + 4 * 2 * N),  # two states and the edge list per item
            "q2_coldest_and_hottest": [float(m["q2"][:, -1].mean()), float(m["q2"][:, 0].mean())]}


def plain(a):
    """tempering_run through the C ABI of the library file a.lib: only symbols that the parent commit has as well."""
    import torch
    torch.cuda.is_available()
    import isingmontecarlo_amd as im
    import isingmontecarlo_amd.classical as cl
    import _lattices as lat

    lib = C.CDLL(os.path.abspath(a.lib))
    names = ("isingmc_classical_create", "isingmc_classical_destroy", "isingmc_classical_pt_attach", "isingmc_classical_pt_run", "isingmc_classical_last_kernel_ms",
             "isingmc_classical_get_state")
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = im.SYMBOLS[name]
    ed, js, hs = cl._model(lat.two_d_periodic(L), [0.0] * N)
    ladder = np.ascontiguousarray(np.linspace(0.2, 1.0, NTEMPS))
    h = C.c_void_p()
    assert lib.isingmc_classical_create(C.byref(cl._config(ed, js, hs, SEED, R)), C.byref(h)) == 0
    assert lib.isingmc_classical_pt_attach(h, NTEMPS, im._ptr(ladder, C.c_double)) == 0
    energy, mag, ms = np.zeros((a.rounds, R)), np.zeros((a.rounds, R), dtype=np.int32), C.c_float(0)

    def run(rounds, steps):
        assert lib.isingmc_classical_pt_run(h, rounds, steps, N, cl.NONE, cl.NONE, cl.KINDS_SPIN, im._ptr(energy, C.c_double), im._ptr(mag, C.c_int32)) == 0
        assert lib.isingmc_classical_last_kernel_ms(h, C.byref(ms)) == 0
        return ms.value

    run(min(a.warmup, a.rounds), 1)
    out = {f"steps_{s}": [] for s in STEPS}
    for _ in range(a.repeats):
        for s in STEPS:
            out[f"steps_{s}"].append(run(a.rounds, s))
    state = np.zeros((R, N), dtype=np.uint8)
    assert lib.isingmc_classical_get_state(h, 0xFFFFFFFF, im._ptr(state, C.c_uint8)) == 0
    lib.isingmc_classical_destroy(h)
    return {"event_ms_per_call": out, "state_checksum": int(np.packbits(state).astype(np.uint64).sum()), "energy_checksum": float(energy.sum())}


def child(a, step, extra=()):
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(a.rounds), "--warmup", str(a.warmup),
           "--repeats", str(a.repeats)] + list(extra)
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise SystemExit(f"bench_classical_overlap: step {step} ended with status {p.returncode}; nothing more is run")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--processes", type=int, default=3, help="processes per library in the comparison with the parent commit")
    ap.add_argument("--parent-lib", default=None, help="libisingmc_hip.so built from the parent commit")
    ap.add_argument("--limit", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classical_overlap_bench.json"))
    ap.add_argument("--step", choices=["measure", "plain"], default=None, help="(internal) run one GPU step in this process")
    ap.add_argument("--lib", default=None, help="(internal) the library file of a plain step")
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps(measure(a) if a.step == "measure" else plain(a)))
        return
    out = {"lattice": f"{L}x{L} periodic, Villain couplings", "replicas": R, "groups": GROUPS, "copies": COPIES, "temperatures": NTEMPS, "beta_abs_J": [0.2, 1.0],
           "nspin": N, "rounds_per_call": a.rounds, "repeats": a.repeats}
    out["measuring"] = child(a, "measure")
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
            cmp[key] = {k: spread([x for r in v for x in r["event_ms_per_call"][key]]) for k, v in runs.items()}
            cmp[key]["this_minus_parent_median"] = cmp[key]["this"]["median"] - cmp[key]["parent"]["median"]
            cmp[key]["parent_spread"] = cmp[key]["parent"]["max"] - cmp[key]["parent"]["min"]
        cmp["equal_results"] = len({(r["state_checksum"], r["energy_checksum"]) for v in runs.values() for r in v}) == 1
        out["existing_path_against_parent"] = cmp
    else:
        out["existing_path_against_parent"] = "not measured: no --parent-lib given"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
