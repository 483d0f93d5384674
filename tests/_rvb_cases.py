"""The RVB sweep's working set: cases that reach the regrowth path and every cap of the growth areas, chosen on the CPU.

Every attempt is grown in a small area first (SSE_RVB_SLOT_CL members, SSE_RVB_SLOT_SET candidates per boundary set, in registers);
one that outgrows it is grown again in a large area in LDS (SSE_RVB_MAXCL, SSE_RVB_SETCAP), and the probability pass and the
mutation track at most SSE_RVB_BONDCAP boundary bonds.  Past a large cap the sweep stops with ECAPACITY (code 7).  The oracle has
no caps; its statistics (Replica.rvb_update(..., stats=True)) say which attempt meets which of them, so a case here is a model, a
seed, a program of steps, the branch it is there for and the least number of attempts that must reach it.  analyse() replays a
case in the oracle; tests/test_rvb_working_set_cpu.py holds the conditions, tests/test_gpu_rvb_working_set.py runs the device.

The constants are parsed out of the kernel headers, never retyped."""
import os
import re

import numpy as np

import _lattices as lat

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "isingmontecarlo_amd", "csrc")


def _defines(path, found):
    """#define NAME <integer expression of earlier names> of one header -> found[NAME]."""
    with open(path) as f:
        for name, expr in re.findall(r"^\s*#\s*define\s+([A-Z][A-Z0-9_]*)[ \t]+([^/\n]+?)[ \t]*(?://.*|/\*.*)?$", f.read(), re.M):
            expr = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uU]?[lL]{0,2}\b", r"\1", expr)
            if not re.fullmatch(r"[\sA-Z0-9_a-fxX+\-*/()<>|&]+", expr):
                continue
            try:
                found[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(found)))
            except Exception:
                pass
    return found


K = _defines(os.path.join(_CSRC, "sse_rvb_split.hip.h"), _defines(os.path.join(_CSRC, "sse_rvb.hip.h"), {}))
_FMT = _defines(os.path.join(os.path.dirname(_CSRC), "..", "include", "sse_format.h"), {})
SSE_TAG_RVB = _FMT["SSE_TAG_RVB"]
SMALL = dict(cl=K["SSE_RVB_SLOT_CL"], set=K["SSE_RVB_SLOT_SET"], sub=K["SSE_RVB_SLOT_SUB"], win=K["SSE_RVB_SLOT_WIN"])
LARGE = dict(cl=K["SSE_RVB_MAXCL"], set=K["SSE_RVB_SETCAP"], sub=K["SSE_RVB_MAXSUB"], win=K["SSE_RVB_MAXWIN"])
BONDCAP, AHEAD, STRIDE = K["SSE_RVB_BONDCAP"], K["SSE_RVB_PROD_AHEAD"], K["SSE_RVB_PROD_STRIDE"]
GROUP = 64  # attempts per group of the regrow scan (rvb_grow_kernel)


# ---- draws ----
def cluster_size(oracle, seed, epoch, replica, attempt):
    """csize of an attempt: draw 1 of rvb_draw (counter (1, epoch_lo, replica, tag << 24 | attempt), key = the seed's halves):
    trailing ones of its first 64 bits, plus one (rvb.rs:1190-1192)."""
    import ctypes as C
    ctr = (C.c_uint32 * 4)(1, epoch & 0xFFFFFFFF, replica, (SSE_TAG_RVB << 24) | (attempt & 0xFFFFFF))
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = (C.c_uint32 * 4)()
    oracle.lib().ora_philox4x32_10(ctr, key, out)
    bits = out[0] | (out[1] << 32)
    csize = 1
    while (bits & 1) and csize <= 64:
        csize += 1
        bits >>= 1
    return csize


def find_seed(oracle, R, attempts, epoch, at_least=17, first=1, last=4000):
    """The first seed in [first, last) whose sweep at `epoch` (R replicas x attempts) draws a cluster size >= at_least, or None."""
    for seed in range(first, last):
        for r in range(R):
            for a in range(attempts):
                if cluster_size(oracle, seed, epoch, r, a) >= at_least:
                    return seed
    return None


# ---- records of the two-launch form (sse_rvb_split.hip.h: "record of one attempt in HBM") ----
def record_words(nsub, ntog, nwin, nadj):
    """Words of an attempt's record behind its bond map: (lists, lists + edges).  lists = header + toggles, sub-variables and
    windows, two words each; the edges add sadj[nsub + 1] and adjb[nadj]."""
    lists = 8 + 2 * int(ntog) + 2 * int(nsub) + 2 * int(nwin)
    return lists, lists + int(nsub) + 1 + int(nadj)


def edges_listed(row):
    """rvb_store_product: the edges are listed when the whole record stays within the part that is fetched ahead."""
    return record_words(row["nsub"], row["ntog"], row["nwin"], row["nadj"])[1] <= AHEAD


def whole_record(row):
    """rvb_main_kernel: `words > small`, the record is fetched whole over both fetched-ahead parts."""
    return record_words(row["nsub"], row["ntog"], row["nwin"], row["nadj"])[0] > AHEAD


# ---- what an attempt's statistics mean for the device ----
def regrown(row):
    """Outgrows a small area: one member, candidate, sub-variable candidate or window more than it holds."""
    return bool(row["ncl"] > SMALL["cl"] or row["bf"] > SMALL["set"] or row["bn"] > SMALL["set"] or row["ncand"] > SMALL["sub"]
                or row["nwin"] > SMALL["win"])


def loud_cap(row):
    """The large cap an attempt exceeds (the first in the order the kernels meet them), or None."""
    if row["bf"] > LARGE["set"]:
        return "bf"
    if row["bn"] > LARGE["set"]:
        return "bn"
    if row["ncl"] > LARGE["cl"]:
        return "cl"
    if row["ncand"] > LARGE["sub"]:
        return "sub"
    if row["nwin"] > LARGE["win"]:
        return "win"
    if row["bonds_prob"] > BONDCAP or row["bonds_mut"] > BONDCAP:
        return "bonds"
    return None


# ---- programs: lists of steps that the oracle and the device run side by side ----
# ("diag",) diagonal step at the case's beta; ("rvb", attempts or None) one standalone sweep; ("cluster",) cluster step without the
# free spins; ("free",) free spins; ("loop",) directed loop; ("run", timesteps, flags) whole timesteps, sampling every second one;
# ("step_rvb",) one whole timestep with FLAG_RVB
def sweeps_program(its, attempts=None):
    """`its` times: diagonal step, RVB sweep, cluster step, free spins (the order of test_rvb_update_matches_oracle)."""
    return [s for _ in range(its) for s in (("diag",), ("rvb", attempts), ("cluster",), ("free",))]


def shape_edges_primitives(its):
    """check_primitives of test_gpu_shape_edges.py: diagonal, cluster, free spins, directed loop, RVB sweep."""
    return [s for _ in range(its) for s in (("diag",), ("cluster",), ("free",), ("loop",), ("rvb", None))]


def shape_edges_run_model(its, steps):
    """run_model of test_gpu_shape_edges.py: the primitives, `steps` timesteps each without flags, with the directed loop and with
    the heat bath, then `steps` timesteps with RVB sweeps."""
    return shape_edges_primitives(its) + [("run", steps, f) for f in (0, 1, 4)] + [("step_rvb",)] * steps


def oracle_step(reps, step, beta, stats=False):
    """One step on every replica; returns the per-replica results (cluster counts, loop lengths, RVB successes — with stats=True
    RVB gives [(successes, rows)]), or None."""
    kind = step[0]
    if kind == "diag":
        for rep in reps:
            rep.diagonal_update(beta)
            want = rep.n + rep.n // 2
            if want > rep.cutoff:
                assert rep.set_cutoff(want) == 0
        return None
    if kind == "cluster":
        return [rep.cluster_update(0.5) for rep in reps]
    if kind == "free":
        for rep in reps:
            rep.flip_free_spins()
        return None
    if kind == "loop":
        return [rep.loop_update() for rep in reps]
    if kind == "run":
        for rep in reps:
            rep.timesteps(step[1], beta, 2, step[2])
        return None
    if kind == "step_rvb":  # ora_timestep with FLAG_RVB, taken apart for the sweep's statistics: diagonal, RVB, cluster, free spins
        oracle_step(reps, ("diag",), beta)
        res = oracle_step(reps, ("rvb", None), beta, stats)
        oracle_step(reps, ("cluster",), beta)
        oracle_step(reps, ("free",), beta)
        return res
    assert kind == "rvb", step
    return [rep.rvb_update(attempts_of(step, rep.model.nvars), stats=stats) for rep in reps]


def attempts_of(step, nvars):
    return (nvars + 1) // 2 if step[0] == "step_rvb" or step[1] is None else step[1]


def two_hubs(leaves, j_bridge):
    """Hubs 0 and 1 with `leaves` leaves each (J = 1) and a bridge variable 2 tied to both by j_bridge: from a leaf a cluster walks to
    its hub and, by weight, over the bridge to the other hub."""
    e = [((0, 2), j_bridge), ((1, 2), j_bridge)]
    e += [((0, 3 + i), 1.0) for i in range(leaves)]
    e += [((1, 3 + leaves + i), 1.0) for i in range(leaves)]
    return e


def _case(name, edges, nvars, beta, seed, program, branch, at_least, R=3, gamma=1.0, h=0.0, cutoff=None, cap=None, loud=None):
    return dict(name=name, edges=edges, nvars=nvars, gamma=gamma, h=h, beta=beta, seed=seed, R=R, program=program, branch=branch,
                at_least=at_least, cutoff=nvars if cutoff is None else cutoff, cap=8192 if cap is None else cap, loud=loud)


# branch: a predicate name of BRANCHES over (row, attempt, attempts of its sweep); at_least: attempts (over all replicas and sweeps) that
# must satisfy it — conditions, set well below what the oracle counts for these seeds (the census of DESIGN.md), and recomputed by
# tests/test_rvb_working_set_cpu.py.  loud: the cap the sweep must stop at (None: the case stays inside every large cap).
def _in_tail(a, u):
    """Attempt a lies in the last, partial group of 64 that the regrow scan of rvb_grow_kernel looks at."""
    return u % GROUP != 0 and a >= (u // GROUP) * GROUP


BRANCHES = {
    "regrown": lambda r, a, u: regrown(r),
    "regrown_cl": lambda r, a, u: r["ncl"] > SMALL["cl"],
    "regrown_bf": lambda r, a, u: r["bf"] > SMALL["set"],
    "regrown_bn": lambda r, a, u: r["bn"] > SMALL["set"],
    "bn_at_small_cap": lambda r, a, u: r["bn"] == SMALL["set"],
    "bn_one_past_small_cap": lambda r, a, u: r["bn"] == SMALL["set"] + 1,
    "bf_deep": lambda r, a, u: r["bf"] > SMALL["set"] + 32,          # adjacency lists longer than a wave, sets of two and three rounds
    "bn_deep": lambda r, a, u: r["bn"] > 2 * SMALL["set"],
    "bn_at_large_cap": lambda r, a, u: r["bn"] == LARGE["set"],
    "bonds_near_cap": lambda r, a, u: BONDCAP - 48 <= r["bonds_prob"] <= BONDCAP,
    "bonds_at_cap": lambda r, a, u: r["bonds_prob"] == BONDCAP,
    "edges_listed": lambda r, a, u: edges_listed(r),
    "edges_not_listed": lambda r, a, u: not edges_listed(r),
    "whole_record": lambda r, a, u: whole_record(r),
    "regrown_in_tail": lambda r, a, u: regrown(r) and _in_tail(a, u),
    "loud": lambda r, a, u: loud_cap(r) is not None,
}

LATTICE_SEED = 1305   # find_seed(R = 4, 8 attempts, epoch 1): the first seed with a draw >= SSE_RVB_SLOT_CL + 1
TAIL_ATTEMPTS = (1, 63, 64, 65, 129)


def make_cases():
    c = []
    # a cluster of more than SSE_RVB_SLOT_CL members: the seed is searched (find_seed; the CPU test repeats the search)
    c.append(_case("ferro8x8_csize18", lat.two_d_ferro(8), 64, 3.0, LATTICE_SEED, sweeps_program(2, 8), "regrown_cl", 1, R=4))
    c.append(_case("ferro8x8_timesteps", lat.two_d_ferro(8), 64, 3.0, LATTICE_SEED, [("step_rvb",)] * 3, "regrown_cl", 1, R=4))
    # bn at the small cap and one past it (beta = 0: no ops, every leaf is a candidate of bn once the centre is a member)
    c.append(_case("star65_bn64", lat.star(65), 65, 0.0, 4242, sweeps_program(2), "bn_at_small_cap", 2))
    c.append(_case("star66_bn65", lat.star(66), 66, 0.0, 4242, sweeps_program(2), "bn_one_past_small_cap", 2))
    # deep inside the large areas
    c.append(_case("star130_b1.5", lat.star(130), 130, 1.5, 4242, sweeps_program(3), "bf_deep", 20))
    c.append(_case("star130_timesteps", lat.star(130), 130, 1.5, 4242, [("step_rvb",)] * 3, "regrown_bf", 20))
    c.append(_case("star194_b0.2", lat.star(194), 194, 0.2, 4242, sweeps_program(2), "bn_deep", 50))
    # bn at the large cap, and one past it: sweeps of 24 attempts, so that whole sweeps come before the one that stops and some
    # replicas get through it
    c.append(_case("star193_bn192", lat.star(193), 193, 0.0, 4242, sweeps_program(2), "bn_at_large_cap", 2))
    c.append(_case("star194_bn193", lat.star(194), 194, 0.0, 5, sweeps_program(4, 24), "loud", 1, R=4, loud="bn"))
    # bf past the large cap: the sequence of test_star_with_rvb_sweeps (test_gpu_shape_edges.py run_model: same seed, same steps)
    c.append(_case("star70_bf", lat.star(70, -1.0), 70, 1.5, 6200, shape_edges_run_model(3, 12), "loud", 1, cap=4096, loud="bf"))
    # boundary bonds up to SSE_RVB_BONDCAP: a cluster of k whole variables of K_n has k (n - k) of them (seeds searched in the oracle)
    c.append(_case("k34_bonds", lat.complete(34), 34, 0.5, 6, sweeps_program(3), "bonds_near_cap", 1, R=4, cap=16384))
    c.append(_case("k36_bonds288", lat.complete(36), 36, 0.5, 47, sweeps_program(3), "bonds_at_cap", 1, R=4, cap=16384))
    c.append(_case("k38_bonds", lat.complete(38), 38, 0.5, 8, sweeps_program(3), "bonds_near_cap", 1, R=4, cap=16384))
    c.append(_case("k40_bonds", lat.complete(40), 40, 0.5, 14, sweeps_program(3), "loud", 1, R=4, cap=16384, loud="bonds"))
    # records of the two-launch form on both sides of SSE_RVB_PROD_AHEAD: with and without the edges at the sub-variables
    c.append(_case("k24_edges_listed", lat.complete(24), 24, 0.5, 4242, sweeps_program(2), "edges_listed", 20))
    c.append(_case("k25_edges_not_listed", lat.complete(25), 25, 0.5, 4242, sweeps_program(2), "edges_not_listed", 20))
    # a record that the main launch fetches whole (more than SSE_RVB_PROD_AHEAD words of lists, about 316 sub-variables) inside all three
    # caps: both hubs of two_hubs are members, as segments of imaginary time that do not overlap, so that all 316 leaves are
    # sub-variables (about half of them in either boundary set) while the boundary bonds are one hub's at a time.  One attempt in
    # 1500 on this model, next to 1 in 15 that exceeds a cap: sweeps of 12 attempts, seed searched in the oracle.
    c.append(_case("hubs2x158_whole_record", two_hubs(158, -300.0), 319, 0.8, 1622, [("run", 1, 0)] + sweeps_program(2, 12), "whole_record", 1,
                   R=2, cap=1 << 15))
    # attempt counts around the regrow scan's groups of 64, regrown attempts in the last, partial group; and the record buffer, sized
    # by the first sweep that needs it, growing for a longer sweep and serving a shorter one again
    tail = [s for u in TAIL_ATTEMPTS for s in (("diag",), ("rvb", u))] + [("cluster",), ("free",)]
    c.append(_case("star130_group_tails", lat.star(130), 130, 1.5, 10, tail, "regrown_in_tail", 8, R=4))  # (seed: the last attempt of every sweep is regrown in two replicas or more)
    buf = [("diag",), ("rvb", 4), ("diag",), ("rvb", 200), ("diag",), ("rvb", 4), ("cluster",), ("free",)]
    c.append(_case("star130_record_buffer", lat.star(130), 130, 1.5, 4242, buf, "regrown", 50))
    return c


CASES = make_cases()
BY_NAME = {c["name"]: c for c in CASES}
PASSING = [c["name"] for c in CASES if c["loud"] is None]
LOUD = [c["name"] for c in CASES if c["loud"] is not None]
TIMESTEPS = [c["name"] for c in CASES if all(s[0] == "step_rvb" for s in c["program"])]


def make_oracle_pair(oracle, case, R=None):
    e, j = lat.split(case["edges"])
    m = oracle.Model(case["nvars"], e, j, case["gamma"], case["h"])
    reps = [oracle.Replica(m, case["cap"], case["cutoff"], case["seed"], r, None) for r in range(case["R"] if R is None else R)]
    return m, reps


_ANALYSIS = {}


def analyse(oracle, name):
    """Replays a case in the oracle.  Returns dict(sweeps=[(step index, rows [R][attempts] as structured arrays)], first_bad=None or
    (replica, sweep number, attempt, cap) of the earliest sweep that exceeds a large cap — earliest sweep first, then the lowest
    replica —, bad={replica: (attempt, cap)} for every replica that exceeds one in that sweep).  The replay stops behind that sweep:
    the device stops there."""
    if name in _ANALYSIS:
        return _ANALYSIS[name]
    case = BY_NAME[name]
    m, reps = make_oracle_pair(oracle, case)
    sweeps, first_bad, bad = [], None, {}
    dt = np.dtype([(k, np.uint32) for k in oracle.RVB_STATS])
    for si, step in enumerate(case["program"]):
        res = oracle_step(reps, step, case["beta"], stats=True)
        if step[0] not in ("rvb", "step_rvb"):
            continue
        rows = [np.ascontiguousarray(st).view(dt).reshape(-1) for _, st in res]
        sweeps.append((si, rows))
        for r, rr in enumerate(rows):
            for a, row in enumerate(rr):
                cap = loud_cap(row)
                if cap is not None:
                    bad[r] = (a, cap)
                    break
        if bad:
            r0 = min(bad)
            first_bad = (r0, len(sweeps) - 1, bad[r0][0], bad[r0][1])
            break
    out = dict(sweeps=sweeps, first_bad=first_bad, bad=bad)
    _ANALYSIS[name] = out
    return out


def all_rows(an):
    """Every attempt's row of an analysis, as (sweep number, replica, attempt, attempts of the sweep, row); in the sweep that stops,
    the rows up to and including each replica's first attempt past a cap (what lies behind never runs on the device)."""
    for sn, (_, rows) in enumerate(an["sweeps"]):
        last = an["first_bad"] is not None and sn == len(an["sweeps"]) - 1
        for r, rr in enumerate(rows):
            stop = an["bad"][r][0] + 1 if (last and r in an["bad"]) else len(rr)
            for a in range(stop):
                yield sn, r, a, len(rr), rr[a]


def census(oracle, name):
    """What the oracle counts for a case: attempts, those that reach the case's branch, those grown again, the largest cluster,
    boundary sets and boundary-bond set, records with their edges listed / fetched whole, and where the sweep stops."""
    an, case = analyse(oracle, name), BY_NAME[name]
    rows = list(all_rows(an))
    hit = BRANCHES[case["branch"]]
    peak = lambda k: max(int(row[k]) for *_, row in rows)
    return dict(attempts=len(rows), branch=sum(1 for _, _, a, u, row in rows if hit(row, a, u)),
                regrown=sum(1 for *_, row in rows if regrown(row) and loud_cap(row) is None),
                ncl=peak("ncl"), bf=peak("bf"), bn=peak("bn"), bonds=max(peak("bonds_prob"), peak("bonds_mut")),
                listed=sum(1 for *_, row in rows if edges_listed(row)), whole=sum(1 for *_, row in rows if whole_record(row)),
                first_bad=an["first_bad"])


# where the loud cases stop in the oracle: (replica, sweep number, attempt) of the earliest sweep with an attempt past a large cap
STOPS_AT = {"star194_bn193": (1, 2, 21), "star70_bf": (0, 7, 1), "k40_bonds": (0, 2, 9)}


def census_row(oracle, name):
    """The case's row of the census table of DESIGN.md ("RVB working set")."""
    cs, case = census(oracle, name), BY_NAME[name]
    stop = "—" if cs["first_bad"] is None else "replica {}, sweep {}, attempt {}: {}".format(*cs["first_bad"])
    return (f"| `{name}` | {case['branch']} | {cs['attempts']} | {cs['branch']} (≥ {case['at_least']}) | {cs['regrown']} | "
            f"{cs['ncl']} / {cs['bf']} / {cs['bn']} / {cs['bonds']} | {cs['listed']} / {cs['whole']} | {stop} |")
