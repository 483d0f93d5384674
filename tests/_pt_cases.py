"""The tempering parity cases of tests/test_gpu_tempering_edges.py, as plain (JSON-able) dicts, and their references.  The CPU
suite (test_tempering_cpu.py) runs every reference alone and checks that it swaps where the case claims to look; the GPU tests
compare against the same, cached, references.  Test infrastructure only."""
import functools
import json

import numpy as np

import _lattices as lat
import _oracle as O
import _pt_reference as ptref

LOOP, HEATBATH, RVB = O.FLAG_LOOP, O.FLAG_HEATBATH, O.FLAG_RVB


def case(name, model, betas, K, seed, cap, cutoff, steps, sweeps, flags=0, step0=0, gamma=1.0, h=0.0, hams=None, world=1):
    return dict(name=name, model=list(model), betas=[float(b) for b in betas], K=K, seed=seed, capacity=cap, cutoff=cutoff, steps=steps,
                sweeps=sweeps, flags=flags, step0=step0, gamma=gamma, h=h, hams=hams, world=world)


def edges_of(c):
    kind = c["model"][0]
    if kind == "ring":
        return lat.one_d_periodic(int(c["model"][1]), float(c["model"][2]))
    assert kind == "ferro2d"
    return lat.two_d_ferro(int(c["model"][1]))


def nvars_of(c):
    return int(c["model"][1]) if c["model"][0] == "ring" else int(c["model"][1]) ** 2


def slot_hamiltonians(c):
    """(J[T*K][E], gamma[T*K], h[T*K]) of a case with per-slot Hamiltonians, row t*K + k; None without."""
    if not c["hams"]:
        return None
    T, K = len(c["betas"]), c["K"]
    j0 = np.array([j for _, j in edges_of(c)])
    t, k = np.divmod(np.arange(T * K), K)
    J = j0[None, :] * (1.0 + 0.03 * t + 0.01 * k)[:, None]
    return J, 0.9 + 0.03 * t, 0.20 - 0.01 * t


# ---- layouts: 6-site ferromagnetic ring, strings of a few slots: only the (T, K) shape of the decision kernel matters ----
RING6 = ("ring", 6, -1.0)
LAYOUTS = [
    case("T1_K4", RING6, [1.0], 4, 9101, 1024, 16, 6, 2),                               # the step only counts
    case("T2_K1", RING6, np.linspace(1.0, 1.2, 2), 1, 9102, 1024, 16, 12, 2),
    case("T3_K1", RING6, np.linspace(1.0, 1.4, 3), 1, 9103, 1024, 16, 12, 2),             # odd T: the last pair belongs to set b only
    case("T5_K3", RING6, np.linspace(0.8, 1.6, 5), 3, 9104, 2048, 16, 12, 2),
    case("T2_K65", RING6, np.linspace(1.0, 1.2, 2), 65, 9105, 1024, 16, 6, 2),            # two waves, the second nearly empty
    case("T2_K300", RING6, np.linspace(1.0, 1.2, 2), 300, 9106, 1024, 16, 6, 2),          # the stride loop runs twice
]
# ---- more than one state word, strings of several 256-slot chunks ----
LONG = [
    case("ring65", ("ring", 65, -1.0), np.linspace(3.0, 4.0, 4), 3, 9201, 4096, 65, 10, 2),
    case("ferro16x16", ("ferro2d", 16), np.linspace(1.905, 2.1, 6), 2, 9202, 16384, 256, 8, 2),
]
# ---- every update rule (the geometries are the GPU test's business: they do not change the reference) ----
RULE_FLAGS = [0, LOOP, HEATBATH, HEATBATH | LOOP, RVB, RVB | LOOP]
RULES = [case(f"ferro8x8_flags{f}", ("ferro2d", 8), np.linspace(0.8, 1.2, 4), 2, 9300 + f, 4096, 64, 6, 2, flags=f) for f in RULE_FLAGS]
# ---- the step counter crosses 2^32: Philox counter word 3 changes on the way ----
STEP32 = case("T5_K3_step_2p32", RING6, np.linspace(0.8, 1.6, 5), 3, 9104, 2048, 16, 6, 2, step0=2 ** 32 - 3)
# ---- per-slot Hamiltonians, two chains: 40-site ring, J, Gamma and h differ between the slots ----
HAMS = [case(f"ring40_hams_flags{f}", ("ring", 40, -1.0), np.linspace(1.6, 2.4, 6), 2, 9400, 4096, 40, 12, 3, flags=f, hams=True)
        for f in (0, LOOP, HEATBATH, RVB)]
# ---- mode toggle / checkpoint (three legs of 4 steps; the reference is one run of 12) ----
TOGGLE = case("T5_K3_toggle", RING6, np.linspace(0.8, 1.6, 5), 3, 9501, 2048, 16, 12, 2)
# ---- two ranks, three temperatures each ----
TWO_RANKS = [
    dict(case("ferro16x16_two_ranks", ("ferro2d", 16), np.linspace(1.905, 2.1, 6), 2, 9202, 16384, 256, 8, 2, world=2)),
    dict(case("ring40_hams_two_ranks", ("ring", 40, -1.0), np.linspace(1.6, 2.4, 6), 2, 9400, 4096, 40, 12, 3, hams=True, world=2)),
]
ALL_CASES = LAYOUTS + LONG + RULES + [STEP32] + HAMS + [TOGGLE] + TWO_RANKS
BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


@functools.lru_cache(maxsize=None)
def _reference(key, nsteps):
    c = json.loads(key)
    e, j = lat.split(edges_of(c))
    hams = None
    if c["hams"]:
        J, gam, h = slot_hamiltonians(c)
        hams = ptref.SlotHamiltonians(nvars_of(c), e, J, gam, h)
    model = None if hams else O.Model(nvars_of(c), e, j, c["gamma"], c["h"])
    return ptref.reference_pt(model, c["betas"], c["K"], c["seed"], c["capacity"], c["cutoff"], nsteps, c["sweeps"], flags=c["flags"],
                              step0=c["step0"], hams=hams), hams


def reference(c, nsteps=None):
    """(PtReference, SlotHamiltonians or None) of a case, computed once per session and shared: callers must not change it.  Cases
    that differ only in name or world share one run."""
    key = {k: v for k, v in c.items() if k not in ("name", "world")}
    return _reference(json.dumps(key, sort_keys=True), c["steps"] if nsteps is None else int(nsteps))


def check_preconditions(c):
    """A case proves nothing if its reference never swaps where the case claims to look."""
    ref, _ = reference(c)
    T = len(c["betas"])
    assert len(ref.pair_accepts) == T - 1 and int(ref.pair_accepts.sum()) == ref.swaps
    assert (ref.pair_accepts >= 1).all(), f"{c['name']}: a pair of neighbouring temperatures never swaps: {ref.pair_accepts.tolist()}"
    if T == 1:
        assert ref.swaps == 0
    if c["world"] == 2:
        assert ref.pair_accepts[T // 2 - 1] >= 3, f"{c['name']}: the pair across the rank boundary swaps {ref.pair_accepts[T // 2 - 1]} times"
    if c["hams"]:
        assert ref.swaps < ref.attempts, f"{c['name']}: every attempt is accepted: the weights decide nothing"
    for chain in ref.by_slot:
        assert all(r.verify() for r in chain)
    return ref
