"""GPU parity at the sizes where the host code switches kernels and layouts, and on degenerate graphs and strings.

Everything is bit-exact against the CPU oracle (operator words, n, cutoff, epoch, states, accumulators [:7], cluster counts, loop
lengths, RVB successes); the oracle itself is pinned to exact diagonalisation on the degenerate topologies in test_oracle_cpu.py.

The size ladders put one model on each side of every gate of isingmc_create / run():
  * trimmed diagonal kernel           N <= 4096                 45x91 = 4095, 64x64 = 4096 | 17x241 = 4097; chains 4095, 4096 | 4097
  * dedicated cluster kernel          N <= 4095                 ... 4095 | 4096
      its 16-bit ids                  16 N + 384 <= 65535       chains 4071 | 4072 (hot end: next to no cuts)
  * two-launch RVB bond map           Nb <= 8192                chains 4096 (Nb = 8192) | 4097 (Nb = 8194)
  * compact edge table in LDS         E <= 12288                64x96 (E = 12288) | 65x95 (E = 12350); chains 12288 | 12289
      next to the per-variable tables 4.3125 N + 288 + 4096 <= 40960 words of a 160 KB LDS: chains 8480 | 8481 (uniform |J|)
  * per-variable tables in HBM        3.3125 N + 288 + 4096 <= 40960 words: chains 11041 | 11042
  * 16-bit union-find ids in LDS      W N + cuts <= 65535       16 waves: chains 4071 | 4072; 4 waves: beyond the HBM-table switch
Which path a size takes is the engine's business: only the documented implications are asserted, and that every bit of
launch_info() takes both values somewhere on the ladder."""
import numpy as np
import pytest

import _lattices as lat
from _lattices import chain, uni_chain, LADDER, LADDER_IDS
from test_gpu_parity import make_pair, assert_same

pytestmark = pytest.mark.gpu

FLAG_LOOP, FLAG_HEATBATH, FLAG_RVB = 1, 4, 8
# RVB sweeps keep a table of the constant ops in the LDS behind the per-variable tables and refuse (ECAPACITY, code 6) when it
# does not fit: the ladder runs them with the tables in LDS up to the bond-map gate (4097) and through
# ISINGMC_CFG_RVB_GLOBAL_TABLES, the documented way for larger models, beyond it
RVB_LDS_MAX_VARS = 4097


def rung_parameters(nvars):
    """(beta, timesteps per flag set, capacity, attempts of a single RVB sweep, timesteps with RVB sweeps): a string of a few N
    slots at every size (n ~ beta (offset - E0) <= 5 beta N on the rectangles, 2.5 beta N on the chains), a handful of sweeps on
    the largest rungs.  An RVB sweep is (N + 1) / 2 attempts of O(n) each in the oracle (1 s per replica at N = 8480): beyond
    2047 variables the single sweeps make 64 attempts, and whole timesteps with RVB sweeps stop behind the bond-map gate (4097)."""
    beta = 2.0 if nvars <= 129 else (1.0 if nvars <= 2047 else 0.5)
    steps = 12 if nvars <= 129 else (8 if nvars <= 1025 else 4)
    rvb_attempts = None if nvars <= 2047 else 64
    rvb_steps = steps if nvars <= 1025 else (2 if nvars <= 2047 else (1 if nvars <= 4097 else 0))
    return beta, steps, 24 * nvars + 256, rvb_attempts, rvb_steps


def diagonal_step(g, reps, beta):
    g.single_diagonal_step(beta)
    for rep in reps:
        rep.diagonal_update(beta)
        want = rep.n + rep.n // 2
        if want > rep.cutoff:
            assert rep.set_cutoff(want) == 0


def check_primitives(g, reps, beta, iterations, what, rvb, rvb_attempts=None):
    """diagonal, cluster, free spins, directed loop and (rvb) an RVB sweep of rvb_attempts attempts (None: the sweep's own
    (N + 1) / 2), each compared as soon as it ran."""
    for it in range(iterations):
        diagonal_step(g, reps, beta)
        assert_same(g, reps, f"{what} diag it={it}")
        nc = g.single_cluster_step(flip_free=False)
        for r, rep in enumerate(reps):
            assert nc[r] == rep.cluster_update(0.5), f"{what}: cluster count differs it={it} r={r}"
        assert_same(g, reps, f"{what} cluster it={it}")
        g.flip_free_spins()
        for rep in reps:
            rep.flip_free_spins()
        assert_same(g, reps, f"{what} free it={it}")
        lens = g.loop_update()
        for r, rep in enumerate(reps):
            assert lens[r] == rep.loop_update(), f"{what}: loop length differs it={it} r={r}"
        assert_same(g, reps, f"{what} loop it={it}")
        if rvb:
            succ, upd = g.single_rvb_sweep(rvb_attempts)
            for r, rep in enumerate(reps):
                assert succ[r] == rep.rvb_update(upd), f"{what}: RVB successes differ it={it} r={r}"
            assert_same(g, reps, f"{what} rvb it={it}")


def check_timesteps(oracle, g, reps, beta, steps, flag_sets, what, freq=2):
    for flags in flag_sets:
        g.run(steps, beta, sampling_freq=freq, flags=flags)
        oracle.batch_timesteps(reps, steps, [beta] * len(reps), freq, flags)
        assert_same(g, reps, f"{what} timesteps flags={flags}")
        acc = g.accumulators()
        for r, rep in enumerate(reps):
            assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), f"{what} flags={flags}: accumulators differ r={r}: {acc[r]} vs {rep.accumulators()}"


def check_observables(g, m, reps, nedges, what):
    """The folds and counters that run popcounts over whole state words (they see a stray tail bit at once) and the per-bond
    counts, at both ends of every bond kind."""
    s1, s2, sa = g.itime_magnetization()
    d, o = g.count_diagonal_and_off()
    n = g.get_n()
    for r, rep in enumerate(reps):
        assert (int(s1[r]), int(s2[r]), int(sa[r])) == rep.itime_magnetization(), f"{what}: imaginary-time magnetisation differs r={r}"
        w = rep.ops()
        occ = w[w != 0]
        nd = int(((occ & 3) == ((occ >> 2) & 3)).sum())
        assert (int(d[r]), int(o[r])) == (nd, len(occ) - nd), f"{what}: diagonal / off-diagonal counts differ r={r}"
        assert int(d[r]) + int(o[r]) == n[r]
    assert g.num_bonds() == m.nbonds
    N, Nb = g.nvars, m.nbonds
    bonds = range(Nb) if Nb <= 40 else sorted({0, nedges // 2, max(nedges, 1) - 1, nedges, nedges + N // 2, nedges + N - 1, Nb - N, Nb - 1})
    for r in {0, len(reps) - 1}:
        for b in bonds:
            assert g.get_bond_count(b, r) == reps[r].bond_count(b), f"{what}: count of bond {b} differs r={r}"


def run_model(oracle, edges, nvars, gamma, h, beta, steps, cap, seed, R, what, cutoff=None, waves=0, k=0, cfgf=0, iterations=2,
              rvb_attempts=None, rvb_steps=None, with_rvb=True):
    import isingmontecarlo_amd as im
    g, m, reps = make_pair(oracle, edges, gamma, h, nvars if cutoff is None else cutoff, cap, seed, R, waves=waves, k=k, cfg_flags=cfgf, nvars=nvars)
    assert g.nvars == nvars
    assert_same(g, reps, f"{what} init")
    tg = g.launch_info()["global_tables"]
    rvb = with_rvb and not tg and nvars <= RVB_LDS_MAX_VARS
    check_primitives(g, reps, beta, iterations, what, rvb, rvb_attempts)
    check_timesteps(oracle, g, reps, beta, steps, [0, FLAG_LOOP, FLAG_HEATBATH], what)
    if rvb and (rvb_steps is None or rvb_steps):
        check_timesteps(oracle, g, reps, beta, steps if rvb_steps is None else rvb_steps, [FLAG_RVB], what)
    check_observables(g, m, reps, len(edges), what)
    assert g.verify().all(), what
    assert all(rep.verify() for rep in reps), what
    if tg:  # tables in HBM: the RVB sweep refuses loudly (it needs ISINGMC_CFG_RVB_GLOBAL_TABLES), it never runs something else
        with pytest.raises(im.IsingMcError) as ei:
            g.run(1, beta, flags=FLAG_RVB)
        assert ei.value.code == -5
    if not rvb and with_rvb:
        g.close()
        g, m, reps = make_pair(oracle, edges, gamma, h, nvars if cutoff is None else cutoff, cap, seed, R, waves=waves, k=k,
                               cfg_flags=cfgf | im.CFG_RVB_GLOBAL_TABLES, nvars=nvars)
        for it in range(2):
            diagonal_step(g, reps, beta)
            succ, upd = g.single_rvb_sweep(rvb_attempts)
            for r, rep in enumerate(reps):
                assert succ[r] == rep.rvb_update(upd), f"{what}: RVB successes (tables in HBM) differ it={it} r={r}"
            assert_same(g, reps, f"{what} rvb with its tables in HBM it={it}")
            nc = g.single_cluster_step(flip_free=True)
            for r, rep in enumerate(reps):
                assert nc[r] == rep.cluster_update(0.5)
                rep.flip_free_spins()
            assert_same(g, reps, f"{what} cluster behind it it={it}")
        assert g.launch_info()["rvb_global_tables"] and g.verify().all(), what


@pytest.mark.parametrize("name,edges,nvars,h", LADDER, ids=LADDER_IDS)
def test_size_ladder(oracle, name, edges, nvars, h):
    beta, steps, cap, rvb_attempts, rvb_steps = rung_parameters(nvars)
    run_model(oracle, edges, nvars, 1.0, h, beta, steps, cap, 8100 + nvars, 3, name, rvb_attempts=rvb_attempts, rvb_steps=rvb_steps)


def test_every_gate_is_straddled():
    """Every rung is created at the default geometry and runs one timestep (and 64 attempts of an RVB sweep up to 4097
    variables); over the ladder each dispatch bit of launch_info() is seen set and clear, and the documented implications hold on
    every rung."""
    import isingmontecarlo_amd as im
    seen = {k: set() for k in ("fast_diagonal", "lean_cluster", "lds_edge_table", "global_tables", "rvb_split")}
    for name, edges, nvars, h in LADDER:
        g = im.QmcIsingGraph(edges, 1.0, h, nvars, 17, nreplicas=2, capacity=8 * nvars + 64, nvars=nvars)
        g.run(1, 0.25)
        if not g.launch_info()["global_tables"] and nvars <= RVB_LDS_MAX_VARS:
            g.single_rvb_sweep(64)
        info = g.launch_info()
        uniform = len({abs(j) for _, j in edges}) <= 1
        if info["fast_diagonal"]:
            assert nvars <= 4096 and uniform, (name, info)
        if info["lean_cluster"]:
            assert nvars <= 4095, (name, info)
        if info["lds_edge_table"]:
            assert len(edges) <= 12288, (name, info)
        assert g.verify().all(), name
        for k in seen:
            seen[k].add(info[k])
        g.close()
    assert all(v == {False, True} for v in seen.values()), seen


def test_plan_batch_agrees_with_the_batch_created():
    """isingmc_plan_batch, given the LDS bytes this device reports, against launch_info() of the batch isingmc_create makes from
    the same config: on both sides of the gates that move the edge table and then the per-variable tables out of LDS (chains),
    and on the 64 x 64 lattice."""
    import torch
    import isingmontecarlo_amd as im
    import _plan_cases as pc
    lds_bytes = torch.cuda.get_device_properties(0).shared_memory_per_block
    models = [(f"chain{n}", chain(n, uni_chain), n) for n in (4096, 4097, 8480, 8481, 11041, 11042, 12289)] + [("rect64x64", lat.two_d_ferro(64), 4096)]
    seen = set()
    for name, edges, nvars in models:
        case = dict(nreplicas=1, capacity=4096, cutoff=64)
        cfg, keep = pc.config_of(im, case, dict(edges=edges, nvars=nvars, transverse=1.0, longitudinal=0.0))
        rc, out = pc.plan_batch(im, cfg, lds_bytes)
        assert rc == 0, name
        p = dict(zip(pc.SLOTS, out))
        g = im.QmcIsingGraph(edges, 1.0, 0.0, 64, 17, nreplicas=1, capacity=4096, nvars=nvars)
        info = g.launch_info()
        g.close()
        hbm = p["mode"] in (pc.MODE_GLOBAL_TABLES, pc.MODE_PM_GLOBAL_TABLES)
        got = (p["W"], p["K"], p["nwords"], p["mode"] == pc.MODE_LDS_EDGES, hbm, bool(p["fast_diag"]), (4 * p["lds_words_diag"] + 7) & ~7)
        want = (info["waves_per_replica"], info["slots_per_lane"], info["state_words"], info["lds_edge_table"],
                info["global_tables"], info["fast_diagonal"], info["lds_bytes_diagonal"])
        assert got == want, (name, got, want)
        assert ((4 * p["lds_words"] + 7) & ~7, p["lds_ufcap"]) == (info["lds_bytes"], info["lds_uf_ids"]), name
        seen.add((info["lds_edge_table"], info["global_tables"]))
    assert seen == {(True, False), (False, False), (False, True)}, seen


@pytest.mark.parametrize("n", [33, 65, 129])
def test_sample_record_and_bit_series_at_odd_sizes(oracle, n):
    """The sample record's rows against the oracle and the bit-series kernel against numpy, on groups that hold variable N - 1
    (the last bit in use of the last state word)."""
    R, T, beta = 3, 40, 1.5
    edges = chain(n, uni_chain)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.2, n, 16 * n, 4400 + n, R)
    g.attach_sample_record(T)
    g.run(T, beta, sampling_freq=1)
    rows = g.record_states()
    assert rows.shape == (T, R, n)
    for t in range(T):
        for r, rep in enumerate(reps):
            rep.timesteps(1, beta, 1, 0)
            assert np.array_equal(rows[t, r], rep.state()), f"row {t} of replica {r}"
    assert_same(g, reps, f"chain{n} recorded run")
    groups = [[n - 1], [0, n - 1], [n - 2, n - 1, 31, 32], list(range(n))]
    flips = [0, 1, 0, 1]
    series = g.record_series(groups, flips)
    assert series.shape == (R, len(groups), (T + 31) // 32)
    for r in range(R):
        for k, (grp, fl) in enumerate(zip(groups, flips)):
            par = (rows[:, r, grp].sum(axis=1) & 1) ^ fl
            want = np.zeros((T + 31) // 32, dtype=np.uint32)
            for t in range(T):
                want[t >> 5] |= np.uint32(int(par[t]) << (t & 31))
            assert np.array_equal(series[r, k], want), (r, k)


def _isolated():
    # 70 variables, edges on nine of them: isolated variables in every state word, the highest index among them
    return [((0, 1), 1.0), ((1, 2), -1.0), ((2, 33), 1.0), ((33, 34), 1.0), ((34, 63), -1.0), ((63, 64), 1.0), ((64, 65), 1.0), ((65, 0), -1.0), ((5, 40), 1.0)]


def _duplicates():
    # same sign, opposite sign and reversed orientation between one pair each, inside a ring of 6
    return lat.one_d_periodic(6, 1.0) + [((0, 1), 1.0), ((2, 3), -1.0), ((4, 3), 1.0), ((0, 1), 1.0)]


# (name, edges, nvars, h)
DEGENERATE = [
    ("noedges1", [], 1, 0.0),
    ("noedges5", [], 5, 0.0),
    ("noedges40_long", [], 40, 0.3),
    ("isolated70", _isolated(), 70, 0.0),
    ("isolated70_long", _isolated(), 70, -0.2),
    ("duplicates6", _duplicates(), 6, 0.0),
    ("duplicates6_mixed", [(ab, j * (1.0 + 0.5 * (i % 2))) for i, (ab, j) in enumerate(_duplicates())], 6, 0.1),
    ("star70_without_rvb", lat.star(70, -1.0), 70, 0.0),   # degree 69 at the centre (RVB sweeps: test_star_with_rvb_sweeps)
    ("k12", lat.complete(12, 1.0), 12, 0.0),
]


@pytest.mark.parametrize("waves,k,cfgf", [(0, 0, 0), (8, 2, 0), (0, 0, 1)], ids=["default", "w8k2", "no_lds_tables"])
@pytest.mark.parametrize("name,edges,nvars,h", DEGENERATE, ids=[c[0] for c in DEGENERATE])
def test_degenerate_graphs(oracle, name, edges, nvars, h, waves, k, cfgf):
    run_model(oracle, edges, nvars, 1.0, h, 1.5, 12, 4096, 6200, 3, name, waves=waves, k=k, cfgf=cfgf, iterations=3,
              with_rvb=not name.endswith("_without_rvb"))


class RvbWorkingSetCap(Exception):
    """ECAPACITY, code 7: an RVB attempt outgrew the fixed working set of the kernels (csrc/sse_rvb.hip.h)."""


@pytest.mark.xfail(strict=True, raises=RvbWorkingSetCap,
                   reason="RVB attempts keep their cluster, boundary sets and time windows in fixed LDS arrays (SSE_RVB_SETCAP 192 candidates, "
                          "SSE_RVB_BONDCAP 288 bonds, SSE_RVB_MAXWIN 80 windows, ...); around the centre of a star of degree 69 an attempt "
                          "outgrows them and the sweep stops with ECAPACITY (code 7) where the reference and the oracle carry on. "
                          "Loud, never wrong; lifting the caps changes the LDS layout of every RVB kernel (DESIGN.md: out of scope so far).")
@pytest.mark.parametrize("waves,k,cfgf", [(0, 0, 0), (8, 2, 0), (0, 0, 1)], ids=["default", "w8k2", "no_lds_tables"])
def test_star_with_rvb_sweeps(oracle, waves, k, cfgf):
    """The star of test_degenerate_graphs with RVB sweeps among the primitives and in whole timesteps (same seed, same steps)."""
    import isingmontecarlo_amd as im
    try:
        run_model(oracle, lat.star(70, -1.0), 70, 1.0, 0.0, 1.5, 12, 4096, 6200, 3, "star70", waves=waves, k=k, cfgf=cfgf, iterations=3)
    except im.IsingMcError as e:
        if e.code == -3 and "(code 7)" in str(e):
            raise RvbWorkingSetCap(str(e)) from e
        raise


@pytest.mark.parametrize("flags", [0, FLAG_LOOP, FLAG_RVB, FLAG_LOOP | FLAG_RVB])
@pytest.mark.parametrize("beta", [0.0, 2.0])
@pytest.mark.parametrize("cutoff0", [0, 1, 2, 3])
def test_empty_and_near_empty_strings(oracle, cutoff0, beta, flags):
    """Strings of 0 .. 3 slots on a 7-site ring: zero-trip loops and `% cutoff`.  The oracle keeps a string of cutoff 0 empty and
    one of cutoff 1 at cutoff 1 (n + n / 2 never exceeds it), and at beta = 0 nothing is ever inserted."""
    edges = lat.one_d_periodic(7)
    R = 3
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, cutoff0, 256, 3300 + cutoff0, R)
    assert_same(g, reps, "init")
    for it in range(2):  # single primitives on the (near-)empty string first
        diagonal_step(g, reps, beta)
        assert_same(g, reps, f"diag it={it}")
        nc = g.single_cluster_step(flip_free=True)
        for r, rep in enumerate(reps):
            assert nc[r] == rep.cluster_update(0.5)
            rep.flip_free_spins()
        lens = g.loop_update()
        for r, rep in enumerate(reps):
            assert lens[r] == rep.loop_update()
        succ, upd = g.single_rvb_sweep()
        for r, rep in enumerate(reps):
            assert succ[r] == rep.rvb_update(upd)
        assert_same(g, reps, f"primitives it={it}")
    check_timesteps(oracle, g, reps, beta, 40, [flags], f"cutoff0={cutoff0} beta={beta}", freq=3)
    n, cut = g.get_n(), g.get_cutoff()
    if cutoff0 == 0 or beta == 0.0:
        assert (n == 0).all() and (cut == cutoff0).all(), (n, cut)
    if cutoff0 == 1:
        assert (cut == 1).all() and (n <= 1).all(), (n, cut)
    check_observables(g, m, reps, len(edges), f"cutoff0={cutoff0} beta={beta} flags={flags}")
    assert g.verify().all()


@pytest.mark.parametrize("R", [1, 63, 65, 257])
def test_replica_counts_around_the_verify_blocks(oracle, R):
    """verify() launches (R + 63) / 64 blocks of 64 threads; the per-replica getters and setters at the last index."""
    edges = lat.two_d_periodic(3)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.1, 9, 1024, 5100 + R, R)
    g.run(12, 1.5, sampling_freq=2)
    oracle.batch_timesteps(reps, 12, [1.5] * R, 2, 0)
    assert_same(g, reps, f"R={R}")
    ok = g.verify()
    assert ok.shape == (R,) and ok.all()
    acc = g.accumulators()
    assert np.array_equal(acc[R - 1, :7], reps[R - 1].accumulators()[:7])
    last = R - 1
    assert [g.get_bond_count(b, last) for b in range(m.nbonds)] == [reps[last].bond_count(b) for b in range(m.nbonds)]
    assert np.array_equal(g.export_ops(last), reps[last].ops())
    # set_state / state_ref round trip with r = all, then the last replica alone; the saved states go back and verify() still holds
    saved = g.state_ref()
    rng = np.random.default_rng(R)
    pattern = rng.integers(0, 2, size=(R, 9), dtype=np.uint8)
    g.set_state(pattern)
    assert np.array_equal(g.state_ref(), pattern)
    g.set_state(1 - pattern[last], r=last)
    pattern[last] = 1 - pattern[last]
    assert np.array_equal(g.state_ref(), pattern)
    g.set_state(saved)
    assert np.array_equal(g.state_ref(), saved) and g.verify().all()
    g.set_cutoff(int(g.get_cutoff()[last]) + 5, r=last)
    assert reps[last].set_cutoff(reps[last].cutoff + 5) == 0
    g.run(5, 1.5)
    oracle.batch_timesteps(reps, 5, [1.5] * R)
    assert_same(g, reps, f"R={R} after the round trip")
    assert g.verify().all()


# (capacity, ring size, beta, steps): found with the oracle alone (seed 7700 + capacity, 4 replicas): after `steps` timesteps at `beta`
# the largest cutoff of the batch stands within 3 slots of the prime capacity and no replica has asked for more
PRIME_CAPACITIES = [
    (97, 16, 0.945, 60),
    (8191, 1000, 1.668, 21),
]


@pytest.mark.parametrize("cap,ring,beta,steps", PRIME_CAPACITIES, ids=[f"cap{c[0]}" for c in PRIME_CAPACITIES])
def test_prime_capacities_fill_up_and_then_fail_loudly(oracle, cap, ring, beta, steps):
    import isingmontecarlo_amd as im
    R = 4
    edges = lat.one_d_periodic(ring, -1.0)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, ring, cap, 7700 + cap, R)
    g.run(steps, beta, sampling_freq=1)
    for rep in reps:
        rep.timesteps(steps, beta, 1, 0)
    assert_same(g, reps, f"capacity {cap}")
    cut = g.get_cutoff()
    assert cap - 3 <= cut.max() <= cap, cut
    assert g.verify().all()
    # one more step at three times beta: every replica's n + n / 2 passes the capacity (the oracle says so too)
    assert all(rep.timestep(3.0 * beta, 0) != 0 for rep in reps)
    with pytest.raises(im.IsingMcError) as ei:
        g.run(1, 3.0 * beta)
    assert ei.value.code == -3


def _random_model(rng):
    """Random connected graph of 41 .. 700 variables, as test_gpu_parity._random_model draws them below 40."""
    n = int(rng.integers(41, 701))
    edges = {}
    for v in range(1, n):  # spanning tree first: connected
        edges[(int(rng.integers(0, v)), v)] = 0.0
    for _ in range(int(rng.integers(0, 2 * n))):
        a, b = (int(x) for x in rng.integers(0, n, size=2))
        if a != b:
            edges[(min(a, b), max(a, b))] = 0.0
    uniform = bool(rng.integers(0, 2))
    out = []
    for (a, b) in sorted(edges):
        mag = 1.0 if uniform else float(rng.uniform(0.3, 2.0))
        out.append(((a, b), mag * (1.0 if rng.integers(0, 2) else -1.0)))
    gamma = float(rng.choice([0.4, 1.0, 1.7]))
    h = float(rng.choice([0.0, 0.0, 0.25, -0.6]))
    beta = float(rng.choice([0.5, 1.5, 3.0]))
    return out, gamma, h, beta


@pytest.mark.parametrize("seed", range(12))
def test_random_models_beyond_forty_variables(oracle, seed):
    """test_random_models_all_passes with 41 .. 700 variables and RVB sweeps among the drawn passes."""
    rng = np.random.default_rng(3000 + seed)
    edges, gamma, h, beta = _random_model(rng)
    waves = int(rng.choice([0, 1, 4, 8, 16]))
    k = int(rng.choice([0, 1, 2, 4]))
    cfgf = int(rng.choice([0, 1, 2, 3]))
    flags = int(rng.choice([0, 1, 4, 5, 8, 9, 12]))
    R = int(rng.integers(1, 7))
    nvars = max(max(ab) for ab, _ in edges) + 1
    g, m, reps = make_pair(oracle, edges, gamma, h, 8, 64 * nvars, 2555 + seed, R, waves=waves, k=k, cfg_flags=cfgf)
    steps = int(rng.integers(10, 25))
    g.run(steps, beta, sampling_freq=2, flags=flags)
    for rep in reps:
        rep.timesteps(steps, beta, 2, flags)
    what = f"random model seed={seed} n={g.nvars} E={len(edges)} gamma={gamma} h={h} beta={beta} W={waves} K={k} cfg={cfgf} flags={flags}"
    assert_same(g, reps, what)
    acc = g.accumulators()
    for r, rep in enumerate(reps):
        assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), what
    assert g.verify().all(), what
