#!/usr/bin/env python3
"""Classical Monte Carlo throughput: spin-move attempts per second on a 64 x 64 periodic lattice (the benches' Villain couplings),
R = 1024 replicas, beta |J| = 0.44, spin steps only with nspin = N.

Three numbers: the batched kernel (64 moves of a step side by side per wave), its ISINGMC_CLASSICAL_CFG_SERIAL_MOVES variant (one move at
a time per wave) and isingmc_classical_host_steps on one CPU core; and the share of lanes committed per batch round of the batched
kernel, counted by replaying a replica's rounds from its moves.  The two device variants are timed alternately, with device events
(isingmc_classical_last_kernel_ms), after a warm-up; their final states must be equal.  Writes profiles/classical_bench.json.

    python tools/bench_classical.py [--steps 200] [--repeats 5] [--out profiles/classical_bench.json]

--per-replica times the same workload with R = 1024 independent +-J sign realisations of the lattice's bonds (GraphState(couplings=...))
instead: the planned launch (2 waves per workgroup, the coupling codes in LDS), the launch with the codes kept in global memory
(CFG_GLOBAL_CODES: 4 waves per workgroup) and the shared-coupling batch of the same session, alternately; every replica of the first
two must end in the same state, and replica 0 in the state of the host's sequential rule.  Writes
profiles/classical_per_replica_bench.json.
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


def committed_share(edges, nvars, before, after_fn, nmoves, words):
    """Replay one step of one replica: the share of active lanes that a round of the batched kernel commits, and rounds per batch.
    words[i] = (site word, uniform word) of move i; before = the state; after_fn(v, state) -> accepted?"""
    nbrs = [[] for _ in range(nvars)]
    for (a, b), _ in edges:
        nbrs[a].append(b); nbrs[b].append(a)
    state = before.copy()
    active = committed = rounds = batches = 0
    for base in range(0, nmoves, 64):
        nb = min(64, nmoves - base)
        sites = [(int(words[base + l][0]) * nvars) >> 32 for l in range(nb)]
        p = 0
        batches += 1
        while p < nb:
            acc = [after_fn(sites[l], state, words[base + l][1]) for l in range(p, nb)]
            stamp = {}
            for l in range(p, nb):
                if acc[l - p]:
                    stamp.setdefault(sites[l], l)
            d = nb
            for l in range(p + 1, nb):
                if any(stamp.get(u, 99) < l for u in [sites[l]] + nbrs[sites[l]]):
                    d = l
                    break
            for l in range(p, d):
                if acc[l - p]:
                    state[sites[l]] ^= 1
            active += nb - p; committed += d - p; rounds += 1
            p = d
    return committed / active, rounds / batches, state


def per_replica(a, im, cl, edges, biases, L, R, beta, seed):
    """The 64 x 64 workload on R independent +-J realisations: kernel ms per call of the planned launch, of the launch with the codes in
    global memory and of the shared-coupling batch, timed alternately."""
    N = L * L
    cj = np.ascontiguousarray(np.random.default_rng(seed).choice([-1.0, 1.0], (R, len(edges))))
    graphs = {"shared": im.GraphState(edges, biases, seed, nreplicas=R),
              "per_replica": im.GraphState(edges, biases, seed, nreplicas=R, couplings=cj),
              "per_replica_global_codes": im.GraphState(edges, biases, seed, nreplicas=R, couplings=cj, cfg_flags=cl.CFG_GLOBAL_CODES)}
    plans = {k: g.launch_plan() for k, g in graphs.items()}
    assert plans["per_replica"]["waves"] == 2 and plans["per_replica"]["in_lds"] & 64, plans
    assert plans["per_replica_global_codes"]["waves"] == 4 and not plans["per_replica_global_codes"]["in_lds"] & 64, plans
    start = graphs["per_replica"].state_ref()[:1]
    for g in graphs.values():
        g.timesteps(a.warmup, beta, nspinupdates=N, kinds=cl.KINDS_SPIN)
    ms = {k: [] for k in graphs}
    for _ in range(a.repeats):
        for k, g in graphs.items():  # alternating
            g.timesteps(a.steps, beta, nspinupdates=N, kinds=cl.KINDS_SPIN)
            ms[k].append(g.last_kernel_ms())
    assert np.array_equal(graphs["per_replica"].state_ref(), graphs["per_replica_global_codes"].state_ref()), "the two launches must agree"
    host = cl.host_steps(edges, biases, seed, start, 0, a.warmup + a.host_steps, beta, nspinupdates=N, kinds=cl.KINDS_SPIN, couplings=cj[:1])
    check = im.GraphState(edges, biases, seed, nreplicas=1, couplings=cj[:1])
    check.timesteps(a.warmup + a.host_steps, beta, nspinupdates=N, kinds=cl.KINDS_SPIN)
    assert np.array_equal(check.state_ref(), host[0]), "replica 0 must follow the sequential rule"
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"lattice": f"{L}x{L} periodic, independent +-J signs per replica", "replicas": R, "beta_abs_J": beta, "nspin": N, "steps_per_call": a.steps,
            "repeats": a.repeats, "kernel_ms": {k: [float(x) for x in v] for k, v in ms.items()}, "kernel_ms_median": med,
            "kernel_ms_spread": {k: [float(min(v)), float(max(v))] for k, v in ms.items()},
            "over_shared": {k: med[k] / med["shared"] for k in ("per_replica", "per_replica_global_codes")}, "plans": plans}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=4)
    ap.add_argument("--per-replica", action="store_true", help="time per-replica +-J couplings against the shared-coupling batch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "classical_per_replica_bench.json" if a.per_replica else "classical_bench.json")
    import torch
    torch.cuda.is_available()
    import isingmontecarlo_amd as im
    import isingmontecarlo_amd.classical as cl
    import _lattices as lat
    import _classical_reference as CR

    L, R, beta, seed = 64, 1024, 0.44, 2024
    N = L * L
    edges, biases = lat.two_d_periodic(L), [0.0] * N
    if a.per_replica:
        out = per_replica(a, im, cl, edges, biases, L, R, beta, seed)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    graphs = {"batched": im.GraphState(edges, biases, seed, nreplicas=R), "serial": im.GraphState(edges, biases, seed, nreplicas=R, cfg_flags=cl.CFG_SERIAL_MOVES)}
    for g in graphs.values():
        g.timesteps(a.warmup, beta, nspinupdates=N, kinds=cl.KINDS_SPIN)
    ms = {k: [] for k in graphs}
    for _ in range(a.repeats):
        for k, g in graphs.items():  # alternating
            g.timesteps(a.steps, beta, nspinupdates=N, kinds=cl.KINDS_SPIN)
            ms[k].append(g.last_kernel_ms())
    assert np.array_equal(graphs["batched"].state_ref(), graphs["serial"].state_ref()), "the two variants must agree"
    attempts = float(R) * a.steps * N
    rate = {k: attempts / (np.median(v) * 1e-3) for k, v in ms.items()}

    # one CPU core: the sequential rule
    st = graphs["batched"].state_ref()[:8]
    t0 = time.perf_counter()
    cl.host_steps(edges, biases, seed, st, graphs["batched"].get_epoch()[:8], a.host_steps, beta, nspinupdates=N, kinds=cl.KINDS_SPIN)
    host_rate = 8.0 * a.host_steps * N / (time.perf_counter() - t0)

    # the committed-lane share: replay the next step of replica 0 (the device state after the step checks the replay)
    g = graphs["batched"]
    before, epoch = g.state_ref()[0].copy(), int(g.get_epoch()[0])
    words = CR.philox_np(seed, np.arange(1, N + 1, dtype=np.uint64), epoch, 0, CR.TAG_CLASSICAL)[:, :2]
    jrow = [[] for _ in range(N)]
    for (x, y), j in edges:
        jrow[x].append((y, j)); jrow[y].append((x, j))
    for r in jrow:
        r.sort(key=lambda t: t[0])

    def accept(v, state, uword):
        de = 0.0
        for u, j in jrow[v]:
            de += -2.0 * j * (1.0 if state[v] == state[u] else -1.0)
        return de <= 0.0 or float(uword) / 4294967296.0 < np.exp(-beta * de)
    share, rounds, after = committed_share(edges, N, before, accept, N, words)
    g.timesteps(1, beta, nspinupdates=N, kinds=cl.KINDS_SPIN)
    assert np.array_equal(g.state_ref()[0], after), "the replay of the rounds must end in the device's state"
    c = g.counters()
    out = {"lattice": f"{L}x{L} periodic, Villain couplings", "replicas": R, "beta_abs_J": beta, "nspin": N, "steps_per_call": a.steps, "repeats": a.repeats,
           "kernel_ms": {k: [float(x) for x in v] for k, v in ms.items()},
           "spin_attempts_per_second": {"batched": rate["batched"], "serial_moves": rate["serial"], "host_one_core": host_rate},
           "batched_over_serial": rate["batched"] / rate["serial"], "batched_over_host_core": rate["batched"] / host_rate,
           "acceptance": float(c[:, 1].sum() / c[:, 0].sum()),
           "committed_lane_share_per_round": share, "rounds_per_batch": rounds,
           "plan": cl.plan(edges, biases)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
