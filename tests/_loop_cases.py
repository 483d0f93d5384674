"""Cases of the directed-loop suite (tests/test_loop_cases_cpu.py, tests/test_gpu_loop_edges.py) and the features they must reach.

loop_pass (csrc/sse_loop.hip.h) searches the op-string in tiles of T = 4 * 64 * W slots (W waves, four loads per thread) and takes
its speculative first-tile loads when the cutoff M exceeds 2 T; the start vertex is looked for in one chunk of CH slots
(isingmc_plan_geometry), in sub-tiles of T slots.  features() names what a walk of the CPU oracle exercised of all that, from the
oracle's trace (Replica.loop_update_trace); every case lists the features it claims, and both test files assert them (each at least
MIN_COUNT times over the case's replicas and loops) before anything is compared, so a change of growth rule, chunk grid or seed
cannot quietly empty a case.  Seeds, betas and loop counts were chosen with the oracle alone.

Two ways to drive a case:
  prim  g.loop_update() loop by loop.  A lone loop runs in the general kernel (sweep_kernel) at the batch's wave count.
  step  whole timesteps, one per call, with FLAG_LOOP | FLAG_NO_CLUSTER and no sampling: diagonal pass, cutoff growth, loop, free
        spins.  On a TFIM batch at the default geometry the first two and the loop run in the trimmed kernel (sse_fast.hip.h), which
        no primitive reaches; the oracle replays the timestep pass by pass and traces its loop.
Two kinds of strings:
  natural  warmed up with whole timesteps on both sides;
  placed   one-variable ops on constant one-variable bonds (four equal weights: walks move freely in both directions) at the exact
           slots that give the distances T, T + 1, M and 1 across p = 0, on an all-zero state.  prim: diagonal ops (in = out = 0), a
           valid string by construction.  step: off-diagonal pairs (0 -> 1, 1 -> 0) and beta = 1e-6, because the diagonal pass in
           front of the loop removes every diagonal op and inserts none at that beta, and leaves off-diagonal ops alone (single ops
           on a variable cannot be placed that way: the trimmed kernel meets d = M on natural strings only)."""
from collections import Counter, namedtuple

import numpy as np

import _lattices as lat

FLAG_LOOP, FLAG_NO_CLUSTER = 1, 2
CFG_NO_LDS_TABLES = 1
MIN_COUNT = 3
STEP_BETA_PLACED = 1e-6

FEATURES = ("far_search_2", "far_search_3", "tile_last_lane", "tile_first_lane", "self_found", "self_in_tail_tile", "wrap_fwd", "wrap_bwd",
            "wrap_var_31_32", "near_wrap_fwd", "near_wrap_bwd", "spec_on", "spec_off", "refill_1", "refill_2", "revisit", "two_var_rel1",
            "hop_visited", "start_subtile_k", "start_chunk_k", "start_first_of_chunk", "start_last_of_chunk", "start_behind_empty_chunk",
            "closed_at_vertex", "closed_on_arrival")
FAR, SPEC = ("far_search_2", "far_search_3"), ("spec_on", "spec_off")
START = tuple(f for f in FEATURES if f.startswith("start_"))
# hop_visited: the TFIM has no off-diagonal two-variable op (qmc_ising.rs:863-888), so no TFIM case, the trimmed kernel's included, can
# reach it; everything else is owed on generic W = 1, generic W = 4 and the trimmed kernel, FAR + SPEC + START on generic W = 16 too
OWED = {"generic_w1": FEATURES, "generic_w4": FEATURES, "trimmed": tuple(f for f in FEATURES if f != "hop_visited"), "generic_w16": FAR + SPEC + START}

P, ESIDE, EREL, XSIDE, XREL, VAR, DIST, FORWARD, WRAPPED, CLOSED, WORD = range(11)  # _oracle.LOOP_TRACE


def tile(W):
    return 256 * W


def chunk_size(cap):
    """CH of isingmc_plan_geometry (asserted against it on the GPU side): capacity / 128 chunks, rounded up to 256 slots."""
    return -(-(-(-cap // 128)) // 256) * 256


def features(trace, start, M, W, CH, ops=None):
    """What one walk exercised: Counter of feature -> occurrences.  trace, start: Replica.loop_update_trace (the whole walk: callers
    give it room); M the cutoff; W the waves of the launch; CH the chunk size; ops the string before the walk (only for
    start_behind_empty_chunk).  An empty trace (n = 0) has no feature."""
    f = Counter()
    if len(trace) == 0:
        return f
    T = tile(W)
    t = np.asarray(trace, dtype=np.int64)
    s = t[t[:, CLOSED] != 1]  # the vertices behind which a search ran
    d, fwd, wr = s[:, DIST], s[:, FORWARD] == 1, s[:, WRAPPED] == 1
    assert ((d >= 1) & (d <= M)).all()
    f["far_search_2"] = int(((d > T) & (d <= 2 * T)).sum())
    f["far_search_3"] = int((d > 2 * T).sum())
    f["tile_last_lane"] = int((d == T).sum())
    f["tile_first_lane"] = int((d == T + 1).sum())
    f["self_found"] = int((d == M).sum())
    f["self_in_tail_tile"] = int((d == M).sum()) if M % T in (1, 64) else 0
    f["wrap_fwd"] = int((wr & fwd).sum())
    f["wrap_bwd"] = int((wr & ~fwd).sum())
    f["wrap_var_31_32"] = int((wr & ((s[:, VAR] == 31) | (s[:, VAR] == 32))).sum())
    f["near_wrap_fwd"] = int((wr & fwd & (d == 1) & (s[:, P] == M - 1)).sum())
    f["near_wrap_bwd"] = int((wr & ~fwd & (d == 1) & (s[:, P] == 0)).sum())
    f["spec_on" if M > 2 * T else "spec_off"] = len(s)
    f["refill_1"] = int(len(t) > 64)
    f["refill_2"] = int(len(t) > 128)
    seen = set()
    for p in t[:, P]:
        f["revisit"] += int(p) in seen
        seen.add(int(p))
    f["two_var_rel1"] = int((t[:, EREL] == 1).sum())
    f["hop_visited"] = int((((t[:, WORD] & 3) ^ ((t[:, WORD] >> 2) & 3)) == 3).sum())
    p0 = start[1]
    assert p0 == t[0, P]
    f["start_subtile_k"] = int(p0 % CH >= T)
    f["start_chunk_k"] = int(p0 >= CH)
    f["start_first_of_chunk"] = int(p0 >= CH and p0 % CH == 0)
    f["start_last_of_chunk"] = int(p0 % CH == CH - 1)
    if ops is not None and p0 >= CH:
        o = np.asarray(ops[:(p0 // CH) * CH]).reshape(-1, CH)
        f["start_behind_empty_chunk"] = int(((o != 0).sum(axis=1) == 0).any())
    f["closed_at_vertex"] = int(t[-1, CLOSED] == 1)
    f["closed_on_arrival"] = int(t[-1, CLOSED] == 2)
    return +f


# ---- models: (kind, size).  const_bond(v): the constant one-variable bond of variable v ----
def model_parts(model):
    """(nvars, generic interactions or None, edges, gamma, const_bond)"""
    kind, n = model
    if kind == "xxz":      # lat.xxz_ring_interactions: bonds 0 .. n-1 two-variable with hopping, n + v the hx bond of v
        return n, lat.xxz_ring_interactions(n), None, 0.0, lambda v: n + v
    if kind == "weak_ring":  # TFIM ring, J = -0.05, Gamma = 1 (uniform |J|: the trimmed kernel's class): transverse bond of v = E + v
        return n, None, lat.one_d_periodic(n, -0.05), 1.0, lambda v: n + v
    if kind == "edge_free":  # TFIM without edges: only transverse bonds
        return n, None, [], 1.0, lambda v: v
    raise ValueError(kind)


def op_word(bond, i, o):
    return ((bond + 1) << 4) | i | (o << 2)


def placed_string(layout, M, T, CH, const_bond, offdiag):
    """The placed op-string of a layout: {variable: slots}.  offdiag: pairs (0 -> 1), (1 -> 0) instead of diagonal ops; variables
    with a single op are left out then."""
    s = 5
    if layout == "dist":  # needs M in {2 T, 2 T + 1}
        assert M in (2 * T, 2 * T + 1)
        on = {3: [s, s + T],          # d = T forward, M - T backward
              7: [s + 4, s + T + 5],  # d = T + 1 forward, M - T - 1 backward
              31: [100],              # d = M
              11: [T + 77],           # d = M
              32: [0, M - 1]}         # d = 1 across p = 0 in both directions, d = M - 1 the long way
    elif layout == "start":  # ops at 0, T - 1, T, CH - 1, CH and M - 1, chunk 2 empty
        assert CH >= 2 * T and 3 * CH < M <= 4 * CH
        on = {5: [0, T - 1], 6: [T, CH - 1], 33: [CH, M - 1]}
    else:
        raise ValueError(layout)
    words = np.zeros(M, dtype=np.uint32)
    for v, slots in on.items():
        if offdiag and len(slots) % 2:
            continue
        for i, p in enumerate(slots):
            assert words[p] == 0
            words[p] = op_word(const_bond(v), i & 1, (i & 1) ^ 1) if offdiag else op_word(const_bond(v), 0, 0)
    return words


Case = namedtuple("Case", "name model waves cfg cap cutoff0 beta seed R warm loops mode layout group claims fast")
_N = FEATURES  # (shorthand below)
NAT_LONG = ("wrap_fwd", "wrap_bwd", "refill_1", "refill_2", "revisit", "two_var_rel1", "hop_visited", "closed_at_vertex", "closed_on_arrival")
PLACED_DIST = ("tile_last_lane", "tile_first_lane", "self_found", "wrap_fwd", "wrap_bwd", "wrap_var_31_32", "near_wrap_fwd", "near_wrap_bwd",
        "far_search_2", "closed_at_vertex", "closed_on_arrival", "revisit")
PLACED_DIST_OFF = tuple(f for f in PLACED_DIST if f != "self_found")


def _placed(kind, model, waves, cfg, group, mode="prim", seed=31, R=8, loops=10, fast=False):
    """The three placed strings of a geometry: dist at M = 2 T and 2 T + 1, start at M = 3 CH + 7."""
    W = waves or 4
    T = tile(W)
    cap = 128 * 2 * T  # the smallest capacity whose chunk holds two sub-tiles: CH = 2 T
    CH = 2 * T
    off = mode == "step"
    beta = STEP_BETA_PLACED if off else 0.0
    d = PLACED_DIST_OFF if off else PLACED_DIST
    return [
        Case(f"{kind}_dist_2T", model, waves, cfg, cap, 2 * T, beta, seed, R, 0, loops, mode, "dist", group, d + ("spec_off",), fast),
        Case(f"{kind}_dist_2T1", model, waves, cfg, cap, 2 * T + 1, beta, seed + 1, R, 0, loops, mode, "dist", group,
             d + ("spec_on",) + (() if off else ("self_in_tail_tile",)), fast),
        Case(f"{kind}_start", model, waves, cfg, cap, 3 * CH + 7, beta, seed + 2, R, 0, loops, mode, "start", group,
             START + ("far_search_3", "spec_on"), fast),
    ]


XXZ70, XXZ40, WEAK40 = ("xxz", 70), ("xxz", 40), ("weak_ring", 40)
CASES = (
    # ---- natural strings, generic model: XXZ ring of 70 sites on each side of M = 2 T; sparse rings for the far searches ----
    [Case("xxz70_w1_below", XXZ70, 1, 0, 1 << 16, 8, 2.5, 11, 8, 30, 30, "prim", None, "generic_w1", NAT_LONG + ("spec_off",), False),
     Case("xxz70_w1_above", XXZ70, 1, 0, 1 << 16, 8, 3.5, 12, 3, 30, 12, "prim", None, "generic_w1", NAT_LONG + ("spec_on", "start_chunk_k"), False),
     Case("xxz70_w4_below", XXZ70, 4, 0, 1 << 18, 8, 10.0, 13, 3, 30, 10, "prim", None, "generic_w4", NAT_LONG + ("spec_off",), False),
     Case("xxz70_w4_above", XXZ70, 4, 0, 1 << 18, 8, 14.0, 14, 3, 30, 10, "prim", None, "generic_w4", NAT_LONG + ("spec_on", "start_chunk_k"), False),
     Case("xxz70_w16_below", XXZ70, 16, 0, 1 << 20, 8, 40.0, 15, 3, 30, 6, "prim", None, "generic_w16", NAT_LONG + ("spec_off",), False),
     Case("xxz70_w16_above", XXZ70, 16, 0, 1 << 20, 8, 60.0, 16, 3, 30, 6, "prim", None, "generic_w16", NAT_LONG + ("spec_on",), False),
     Case("xxz70_default", XXZ70, 0, 0, 1 << 18, 8, 14.0, 17, 3, 30, 10, "prim", None, "generic_w4", NAT_LONG + ("spec_on",), False),
     Case("xxz700_w1_sparse", ("xxz", 700), 1, 0, 1 << 16, 700, 0.3, 21, 4, 20, 10, "prim", None, "generic_w1", FAR + ("self_found", "spec_on", "start_subtile_k"), False),
     Case("xxz2500_w4_sparse", ("xxz", 2500), 4, 0, 1 << 18, 2500, 0.3, 22, 4, 20, 10, "prim", None, "generic_w4", FAR + ("self_found", "spec_on", "start_subtile_k"), False),
     Case("xxz2500_w16_sparse", ("xxz", 2500), 16, 0, 1 << 20, 20000, 0.3, 23, 4, 20, 10, "prim", None, "generic_w16", FAR + ("self_found", "spec_on", "start_subtile_k"), False)]
    # (a ring of 9000 sites does not get 16 waves: their per-variable tables do not fit in LDS and the plan falls back to 4; 2500
    # sites are the most that do, so the W = 16 string is made sparse by a cutoff of 20000 instead of by more sites)
    # ---- placed strings, generic model (N = 40 > 32) ----
    + _placed("xxz40_w1", XXZ40, 1, 0, "generic_w1") + _placed("xxz40_w4", XXZ40, 4, 0, "generic_w4") + _placed("xxz40_w16", XXZ40, 16, 0, "generic_w16")
    # ---- TFIM: the general kernel with the edge table in LDS (default geometry and 8 waves) and without it ----
    + _placed("tfim_w4_cl", WEAK40, 0, 0, "tfim_w4_cl", fast=True) + _placed("tfim_w8_cl", WEAK40, 8, 0, "tfim_w8_cl")
    + _placed("tfim_w4_nolds", WEAK40, 4, CFG_NO_LDS_TABLES, "tfim_w4_nolds")
    + [Case("weak40_w8_cl", WEAK40, 8, 0, 1 << 18, 8, 40.0, 41, 8, 30, 24, "prim", None, "tfim_w8_cl", ("wrap_fwd", "wrap_bwd", "refill_1", "refill_2", "revisit", "two_var_rel1", "spec_off"), False),
       Case("weak40_w1_nolds", WEAK40, 1, CFG_NO_LDS_TABLES, 1 << 16, 8, 40.0, 42, 8, 30, 12, "prim", None, "tfim_w1_nolds", ("wrap_fwd", "wrap_bwd", "refill_1", "refill_2", "revisit", "two_var_rel1", "spec_on"), False)]
    # ---- the trimmed kernel: whole timesteps on TFIM batches at the default geometry ----
    + [Case("weak40_fast_below", WEAK40, 0, 0, 1 << 18, 8, 28.0, 51, 8, 30, 24, "step", None, "trimmed", ("wrap_fwd", "wrap_bwd", "refill_1", "revisit", "two_var_rel1", "spec_off", "closed_at_vertex"), True),
       Case("weak40_fast_above", WEAK40, 0, 0, 1 << 18, 8, 40.0, 52, 8, 30, 24, "step", None, "trimmed", ("wrap_fwd", "wrap_bwd", "refill_1", "refill_2", "revisit", "two_var_rel1", "spec_on", "start_chunk_k", "closed_at_vertex"), True),
       Case("edgefree3000_fast", ("edge_free", 3000), 0, 0, 1 << 18, 8, 0.7, 53, 4, 20, 10, "step", None, "trimmed", FAR + ("self_found", "spec_on", "start_subtile_k", "start_chunk_k"), True),
       Case("edgefree1200_fast_tail", ("edge_free", 1200), 0, 0, 1 << 18, 2049, 0.5, 54, 4, 20, 10, "step", None, "trimmed", FAR + ("self_found", "self_in_tail_tile", "spec_on"), True)]
    + _placed("tfim_fast", WEAK40, 0, 0, "trimmed", mode="step", R=24, loops=2, fast=True)
)
CASE_IDS = [c.name for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)
# whole timesteps inside run() with FLAG_LOOP and 7 steps per launch: (model, waves, capacity, beta, seed, flags)
RUN_CASES = [("xxz70_run", XXZ70, 0, 1 << 18, 10.0, 61, FLAG_LOOP | FLAG_NO_CLUSTER), ("weak40_run", WEAK40, 0, 1 << 18, 40.0, 62, FLAG_LOOP)]


def launch_waves(case):
    return case.waves or 4  # (asserted from launch_info() on the GPU side)


# ---- the oracle's side of a case: shared by the CPU test (features, twins) and the GPU test (reference) ----
def oracle_model(oracle, model):
    nvars, ints, edges, gamma, _ = model_parts(model)
    if ints is not None:
        return oracle.Model.generic(nvars, ints)
    e, j = lat.split(edges)
    return oracle.Model(nvars, e, j, gamma, 0.0)


def warm_flags(case):
    return FLAG_LOOP | FLAG_NO_CLUSTER


def oracle_replicas(oracle, case):
    """The case's replicas, warmed up (natural) or loaded with the placed string: (model, replicas)."""
    m = oracle_model(oracle, case.model)
    state = None if case.layout is None else np.zeros(m.nvars, dtype=np.uint8)
    reps = [oracle.Replica(m, case.cap, case.cutoff0, case.seed, r, state) for r in range(case.R)]
    if case.layout is None:
        oracle.batch_timesteps(reps, case.warm, [case.beta] * case.R, 1, warm_flags(case))
    else:
        words = placed_words(case)
        for rep in reps:
            rep.set_ops(words)
    return m, reps


def placed_words(case):
    T = tile(launch_waves(case))
    return placed_string(case.layout, case.cutoff0, T, chunk_size(case.cap), model_parts(case.model)[4], case.mode == "step")


def oracle_round(case, reps):
    """One loop (prim) or one timestep (step) of every replica: (walk lengths, features summed over the replicas)."""
    W, CH = launch_waves(case), chunk_size(case.cap)
    lens, feats = [], Counter()
    for rep in reps:
        if case.mode == "step":  # ora_timestep with FLAG_LOOP | FLAG_NO_CLUSTER, pass by pass
            rep.diagonal_update(case.beta)
            want = rep.n + rep.n // 2
            if want > rep.cutoff:
                assert rep.set_cutoff(want) == 0
        ops = rep.ops()
        M = rep.cutoff
        length, trace, start = rep.loop_update_trace()
        assert length == len(trace), "the trace buffer is shorter than the walk"
        if case.mode == "step":
            rep.flip_free_spins()
        lens.append(length)
        feats.update(features(trace, start, M, W, CH, ops))
    return lens, feats


# One batch in which replica 0 is fresh (no op, cutoff as it was) while the others walk far: (case, rounds).  In at least MIN_COUNT
# rounds another replica walks more than 64 vertices in the same launch.
MIXED = Case("xxz70_w4_mixed", XXZ70, 4, 0, 1 << 18, 8, 14.0, 71, 4, 30, 10, "prim", None, "generic_w4", ("refill_1",), False)


def empty_first_replica(reps):
    reps[0].set_ops(np.zeros(reps[0].cutoff, dtype=np.uint32))
