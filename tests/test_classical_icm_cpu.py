"""Isoenergetic cluster moves without a device: isingmc_classical_host_pt_run_icm and isingmc_classical_host_icm_cluster
(csrc/classical_icm_rule.h by the sequential rule) against the numpy restatement (tests/_classical_icm_cases.py), against the
transition matrix of the move over all pairs of states of a small system, against exact enumeration, and their argument checks.
Every compared value of the runs is an integer or a double computed in one fixed order: those comparisons are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _classical_cases as cc
import _classical_icm_cases as ic
import _classical_overlap_cases as oc
import _classical_pt_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


RULE_MAIN = """#include "classical_icm_rule.h"
struct Ring { uint32_t n; uint32_t row(uint32_t v) const { return 2u * v; } uint32_t nbr(uint32_t k) const { return (k / 2u + ((k & 1u) ? 1u : n - 1u)) % n; } };
int main() {
    uint32_t a, b, g, m, t, c[4], bad = 0;
    bad += cmc_icm_pairs(2) != 1 || cmc_icm_pairs(3) != 1 || cmc_icm_pairs(4) != 2 || cmc_icm_pairs(5) != 2;
    cmc_icm_pair(4, 0, 1, a, b); bad += !(a == 2 && b == 3);
    cmc_icm_pair(4, 5, 1, a, b); bad += !(a == 3 && b == 0);
    cmc_icm_pair(3, 2, 0, a, b); bad += !(a == 2 && b == 0);
    cmc_icm_item(3 * 2 * 4 + 1 * 4 + 2, 2, 1, 5, g, m, t); bad += !(g == 3 && m == 1 && t == 3);
    bad += cmc_icm_count_index(2, 7, 3, 1, 5) != (3 * 2 + 1) * 7 + 5;
    cmc_icm_counter(7, 0x0123456789ull, 9, 1, 5, c); bad += !(c[0] == 12 && c[1] == 0x23456789u && c[2] == 9 && c[3] == ((10u << 24) | 1u));
    bad += cmc_icm_nth_bit(0x80000001u, 0) != 0 || cmc_icm_nth_bit(0x80000001u, 1) != 31 || cmc_icm_nth_bit(0xF0u, 2) != 6;
    const uint8_t diff[8] = {1, 1, 0, 1, 1, 1, 0, 1};  // on the ring of 8: the runs {7, 0, 1} and {3, 4, 5}
    uint8_t mark[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t stack[8];
    bad += cmc_icm_grow(Ring{8}, diff, 3, mark, stack) != 3 || !(mark[3] && mark[4] && mark[5]) || mark[0] || mark[1] || mark[7] || mark[2] || mark[6];
    return (int)bad;
}
"""


def test_rule_header_is_plain_cpp(tmp_path):
    """classical_icm_rule.h compiles on its own under g++ -Wall -Wextra -Werror (and -fsyntax-only as the overlap rule does): no HIP
    header, no device code; its small functions give the values of the rule's text."""
    csrc = os.path.join(ROOT, "isingmontecarlo_amd", "csrc")
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I.", "-x", "c++", "-"], input='#include "classical_icm_rule.h"\n',
                       cwd=csrc, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    src = tmp_path / "rule.cpp"
    src.write_text(RULE_MAIN)
    exe = str(tmp_path / "rule")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + csrc, str(src), "-o", exe])
    assert subprocess.call([exe]) == 0


# ---- exactness of the move ----
def _host_cluster(edges, biases):
    cl = _cl()

    def cluster(a, b, k):
        mask, size = cl.host_cluster(edges, biases, a.astype(np.uint8), b.astype(np.uint8), k)
        assert size == int(mask.sum()) and size >= 1
        return mask
    return cluster


def test_the_move_is_exact_by_enumeration():
    """host_cluster over all 1024 pairs of states of the five-variable system (frustrated triangle, biases, a zero coupling, a
    multi-edge) and all ranks: the transition matrix is symmetric, it leaves the product Boltzmann weight of two copies stationary to
    1e-12 at two temperatures, E_A + E_B is unchanged (exactly with the integer couplings and biases, to rounding with their tenths), d
    is unchanged, the seed is in its cluster, and the cluster is the restatement's."""
    edges, biases = ic.TINY
    n = len(biases)
    p, seen = ic.pair_transitions(n, _host_cluster(edges, biases))
    assert np.array_equal(p, p.T) and np.allclose(p.sum(axis=1), 1.0, atol=1e-15)
    for beta in ic.TINY_BETAS:
        w = ic.product_weight(edges, biases, beta)
        assert np.abs(w @ p - w).max() <= 1e-12, (beta, np.abs(w @ p - w).max())
    st = ic.bits_of(n)
    en, en10 = ic.energies(edges, biases, st), ic.energies(*ic.TINY_FLOAT, st)
    restated = ic.restated_cluster(edges, biases, "right")
    weights = 1 << np.arange(n)
    sizes = set()
    for a, b, k, mask in seen:
        c = int((mask * weights).sum())
        d = st[a] ^ st[b]
        assert mask[np.flatnonzero(d)[k]] and not (mask & ~d).any()
        assert np.array_equal(st[a ^ c] ^ st[b ^ c], d)
        assert en[a ^ c] + en[b ^ c] == en[a] + en[b]
        assert abs((en10[a ^ c] + en10[b ^ c]) - (en10[a] + en10[b])) <= 1e-12
        assert np.array_equal(mask, restated(st[a], st[b], k))
        sizes.add(int(mask.sum()))
    assert sizes == {1, 2, 3, 4, 5}  # the zero coupling on (3, 4) connects: only then is a cluster of five possible from d = all
    with pytest.raises(_cl().IsingMcError) as ei:
        _cl().host_cluster(edges, biases, [0, 1, 0, 0, 0], [0, 0, 0, 0, 0], 1)
    assert "rank must be below" in str(ei.value)


def test_wrong_rules_break_stationarity():
    """The test of the test above, on the numpy restatement alone: the same matrix built from two wrong rules is not stationary, and
    from the right rule it is.  Observed max |w P - w| at beta = 0.03, 0.11:
      right        4e-19   9e-19     (bound 1e-12)
      neighbours   1.7e-3  8.9e-3    growth stops at the seed's neighbours
      satisfied    7.4e-3  3.1e-2    the cluster grown over A's satisfied bonds instead of over d
    A miss counts as visible from 1e-6, a million times the bound of the test above."""
    edges, biases = ic.TINY
    miss = {}
    for rule in ic.RULES:
        p, _ = ic.pair_transitions(len(biases), ic.restated_cluster(edges, biases, rule))
        assert np.allclose(p.sum(axis=1), 1.0, atol=1e-15)
        miss[rule] = [float(np.abs(w @ p - w).max()) for w in (ic.product_weight(edges, biases, beta) for beta in ic.TINY_BETAS)]
    print(miss)
    assert max(miss["right"]) <= 1e-12, miss
    assert min(miss["neighbours"]) > 1e-6 and min(miss["satisfied"]) > 1e-6, miss


# ---- the host run against the restatement ----
@pytest.mark.parametrize("name", list(ic.CASES))
def test_host_run_matches_the_restatement(oracle, name):
    """Every case, in every respect: states, epochs, counters and maps, swap counts, the E, M, Q and QL series, both histograms and the
    three cluster counts."""
    c = ic.case(name)
    want = ic.host_parity_reference(name)
    got = ic.restatement_run(name)
    keys = set(want) if c["steps"] else set(want) - {"counters"}
    assert keys == set(got)
    for key in sorted(keys):
        assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), key
    if not c["steps"]:
        assert not want["counters"].any()
    groups = c["chains"] // c["ncopies"]
    assert want["cluster_moves"].shape == (groups, c["ncopies"] // 2, len(c["betas"])) and want["cluster_moves"].dtype == np.uint64


@pytest.mark.parametrize("name", list(ic.CASES))
def test_count_invariants(oracle, name):
    """moves + empty = rounds for every item inside the window; the counts outside the window are zero; size_sum >= moves, and
    size_sum <= N moves."""
    c = ic.case(name)
    want = ic.host_parity_reference(name)
    t_first, t_last = c["window"][0], len(c["betas"]) if c["window"][1] is None else c["window"][1]
    inside = np.zeros(len(c["betas"]), dtype=bool)
    inside[t_first:t_last] = True
    moves, empty, size_sum = (want[k] for k in ic.COUNTS)
    assert ((moves + empty)[:, :, inside] == c["rounds"]).all()
    assert not moves[:, :, ~inside].any() and not empty[:, :, ~inside].any() and not size_sum[:, :, ~inside].any()
    assert (size_sum >= moves).all() and (size_sum <= moves * np.uint64(len(c["biases"]))).all()
    if name == "ring200_path_T2_K2":
        assert (size_sum == 199 * c["rounds"]).all() and (moves == c["rounds"]).all()
    if name == "ring200_equal_T2_K2":
        assert (empty == c["rounds"]).all() and not moves.any() and np.array_equal(want["states"], c["states"])
    if name == "complete65_T2_K2":
        assert np.array_equal(size_sum[0, 0], ((65 - want["overlap"][:, 0, 0, :].astype(np.int64)) // 2).sum(axis=0))  # the cluster is all of d


@pytest.mark.parametrize("name", list(ic.CASES))
def test_the_moves_leave_both_overlaps_alone(oracle, name):
    """With steps = 0, one round at a time from the case's initial states, the maps put back to the identity before every round and the
    step number advancing (so that the pairs rotate): Q and QL of the moved pairs, measured on the states a round leaves at the
    temperatures it found them at, repeat the values the round measured before its moves, round after round, and for K = 2 with a
    whole window so do both histograms.  (The swaps of a run re-pair the states at a temperature, and with K > 2 the moves of one pair
    change the overlaps of that pair's copies with the others: neither is the moves' doing, so the maps are put back and the other
    pairs are left out.)  E_A + E_B of a moved pair is unchanged to rounding."""
    cl = _cl()
    c = ic.case(name)
    k, t_all = c["ncopies"], len(c["betas"])
    t_first, t_last = c["window"][0], t_all if c["window"][1] is None else c["window"][1]
    pairs = oc.pairs_of(k)
    common = dict(edges=c["edges"], biases=c["biases"], seed=cc.SEED, epochs=0, betas=c["betas"], rounds=1, steps=0, ncopies=k, couplings=c["couplings"],
                  replica_offset=ic.offset(name))
    states = ic.initial(c, ic.offset(name))
    rounds = 2 if len(c["biases"]) > 5000 else 4
    for i in range(rounds):
        before = cl.host_tempering_run(states=states, pt_step=i, cluster_moves=c["window"], **common)
        after = cl.host_tempering_run(states=before["states"], pt_step=i, **common)  # the identity maps again; no moves
        moved = [pairs.index(tuple(sorted(((i % k + 2 * m) % k, (i % k + 2 * m + 1) % k)))) for m in range(k // 2)]
        for key in ("overlap", "link_overlap"):
            assert np.array_equal(before[key][0][:, moved, t_first:t_last], after[key][0][:, moved, t_first:t_last]), (i, key)
        if k == 2 and (t_first, t_last) == (0, t_all):
            assert all(np.array_equal(before[key], after[key]) for key in oc.HISTS + ("overlap", "link_overlap"))
            e0, e1 = before["energy"][0], after["energy"][0]  # [C][T]: after the moves / of the states they left; equal by construction
            assert np.array_equal(e0, e1)
            plain = cl.host_tempering_run(states=states, pt_step=i, **common)["energy"][0]  # before the moves
            assert np.allclose(plain[0::2] + plain[1::2], e0[0::2] + e0[1::2], rtol=1e-12, atol=1e-9)  # E_A + E_B of every pair, to rounding
        states = before["states"]


# ---- composition and sharding ----
RING = cc.CASES["ring33"]
LADDER4 = [0.2, 0.5, 1.0, 2.0]
RING_CASE = ic._case(RING, LADDER4, 2, 4, window=(1, 4))


def test_calls_compose_and_groups_shard(oracle):
    """10 rounds = 3 + 7 with the counts and the histograms handed on; two groups = two batches of one group at the replica offsets 0
    and K T; measure = False moves the same and measures nothing."""
    cl = _cl()
    c = RING_CASE
    whole = ic.host_run(cl, c, rounds=10)
    a = ic.host_run(cl, c, rounds=3)
    b = cl.host_tempering_run(c["edges"], c["biases"], cc.SEED, a["states"], a["epochs"], c["betas"], 7, c["steps"], kinds=cl.KINDS_ALL, temp_of=a["temp_of"],
                              pt_step=a["pt_step"], ncopies=2, histograms=(a["overlap_hist"], a["link_hist"]), cluster_moves=c["window"],
                              cluster_counts=tuple(a[k] for k in ic.COUNTS))
    assert ((a["cluster_moves"] + a["cluster_empty"])[:, :, 1:] == 3).all()  # (the second call worked on copies)
    for key in ic.COUNTS + ic.HISTS + ("states", "temp_of", "epochs", "counters", "attempts", "accepts"):
        want = whole[key] if key != "counters" and key not in ("attempts", "accepts") else whole[key] - a[key]
        assert np.array_equal(want, b[key]), key
    for key in ic.SERIES:
        assert np.array_equal(whole[key], np.concatenate([a[key], b[key]])), key
    half = dict(c, chains=2)
    lo, hi = ic.host_run(cl, half, rounds=10, replica_offset=0), ic.host_run(cl, half, rounds=10, replica_offset=8)
    for key in ic.COUNTS + ic.HISTS + ("states",):
        assert np.array_equal(whole[key], np.concatenate([lo[key], hi[key]])), key
    for key in ic.SERIES:
        assert np.array_equal(whole[key], np.concatenate([lo[key], hi[key]], axis=1)), key
    quiet = ic.host_run(cl, c, rounds=10, measure=False)
    assert "overlap" not in quiet and "overlap_hist" not in quiet
    for key in ic.COUNTS + ("states", "temp_of", "energy", "magnetization"):
        assert np.array_equal(whole[key], quiet[key]), key
    plain = oc.host_run(cl, c["edges"], c["biases"], c["betas"], 4, 2, 10, c["steps"], kinds=cl.KINDS_ALL)
    assert not np.array_equal(plain["states"], whole["states"])  # the moves did move
    with pytest.raises(cl.IsingMcError):
        ic.host_run(cl, c, rounds=1, cluster_counts=(np.zeros((2, 1, 3), dtype=np.uint64),) * 3)


def test_every_refusal(oracle):
    """Every ISINGMC_EINVAL of icm_attach through the host entry that shares its checks, each with its own message, and the null
    handle.  (The refusals that need a handle: tests/test_gpu_classical_icm.py.)"""
    cl = _cl()
    edges, biases = cc.CASES["triangle"]
    ok = dict(edges=edges, biases=biases, seed=1, states=np.zeros((12, 3), dtype=np.uint8), epochs=0, betas=[0.5, 1.0, 2.0], rounds=1, steps=1, ncopies=2,
              cluster_moves=(0, None))
    out = cl.host_tempering_run(**ok)
    assert out["cluster_moves"].shape == (2, 1, 3) and ((out["cluster_moves"] + out["cluster_empty"]) == 1).all()
    assert cl.host_tempering_run(**{**ok, "cluster_moves": (2, 3)})["pt_step"] == 1 and cl.host_tempering_run(**{**ok, "cluster_moves": (0, 3)})["pt_step"] == 1
    for change, words in [
        (dict(ncopies=None), "cluster moves need ncopies >= 2"),
        (dict(cluster_moves=(1, 1)), "[1, 1) is empty or reversed"),
        (dict(cluster_moves=(2, 1)), "[2, 1) is empty or reversed"),
        (dict(cluster_moves=(3, None)), "[3, 3) is empty or reversed"),
        (dict(cluster_moves=(0, 4)), "t_last = 4 exceeds the 3 temperatures"),
        (dict(cluster_moves=(5, 4)), "t_last = 4 exceeds the 3 temperatures"),
        (dict(ncopies=1), "ncopies >= 2"),  # the refusals of the overlaps and of tempering come first
        (dict(ncopies=3), "multiple of ncopies"),
        (dict(betas=[1.0]), "ntemps >= 2"),
    ]:
        with pytest.raises(cl.IsingMcError) as ei:
            cl.host_tempering_run(**{**ok, **change})
        assert ei.value.code == -1 and words in str(ei.value), (change, str(ei.value))
    import isingmontecarlo_amd as im
    lib = im.load_library()
    assert lib.isingmc_classical_icm_attach(None, 0, 0) == -1 and lib.isingmc_classical_icm_reset(None) == -1 and lib.isingmc_classical_icm_window(None, None, None) == -1
    assert lib.isingmc_classical_icm_counts(None, None, None, None) == -1 and lib.isingmc_classical_icm_set_counts(None, None, None, None) == -1
    assert lib.isingmc_classical_pt_run_icm(None, 1, 1, 1, 1, 1, 0, None, None, None, None, 1) == -1 and lib.isingmc_classical_icm_launch_plan(None, None) == -1
    assert lib.isingmc_classical_icm_plan(8, 65536, None) == -1 and b"null output" in lib.isingmc_classical_last_error(None)
    # every output of the host entry may be null
    ed, js, hs = cl._model(edges, biases)
    cfg = cl._config(ed, js, hs, 1, 12)
    st, ep, tof, step = np.zeros((12, 3), dtype=np.uint8), np.zeros(12, dtype=np.uint64), np.arange(12, dtype=np.uint32) % 3, C.c_uint64(0)
    ladder = np.array([0.5, 1.0, 2.0])
    args = [1, 1, cl.NONE, cl.NONE, cl.NONE, 0, im._ptr(st, C.c_uint8), im._ptr(ep, C.c_uint64), im._ptr(tof, C.c_uint32), C.byref(step)] + [None] * 9
    assert lib.isingmc_classical_host_pt_run_icm(C.byref(cfg), 3, im._ptr(ladder, C.c_double), 2, *args, 1, 0, 0, None, None, None) == 0 and step.value == 1
    assert np.array_equal(st, out["states"])
    mask = np.zeros(3, dtype=np.uint8)
    assert lib.isingmc_classical_host_icm_cluster(C.byref(cfg), None, None, 0, im._ptr(mask, C.c_uint8), None) == -1


def test_icm_plan_follows_the_carve(oracle):
    """The waves fall 4, 2, 1, refused at the carve's own boundaries (a wave's area is three bit sets of ceil(N / 32) words), from below
    and one past, and the words are the carve's."""
    cl = _cl()
    for lds_bytes in (ic.LDS_BYTES, 65536):
        total = lds_bytes // 4
        edge = {w: 32 * (total // (3 * w)) for w in (4, 2, 1)}  # the largest N with w waves
        for w, past in ((4, 2), (2, 1)):
            n = edge[w]
            for nvars, waves in ((n, w), (n + 1, past)):
                p = cl.icm_plan(nvars, lds_bytes)
                words = (nvars + 31) // 32
                assert p == dict(waves=waves, lds_words=3 * words * waves, wave_words=3 * words, max_vars=edge[1]), (nvars, p)
        assert cl.icm_plan(edge[1], lds_bytes)["waves"] == 1 and cl.icm_plan(1, lds_bytes) == dict(waves=4, lds_words=12, wave_words=3, max_vars=edge[1])
        with pytest.raises(cl.IsingMcError) as ei:
            cl.icm_plan(edge[1] + 1, lds_bytes)
        assert ei.value.code == -5 and f"at most {edge[1]} variables in {lds_bytes} bytes" in str(ei.value)
    assert ic.gate(4) == 32 * (40960 // 12) and ic.gate(2) == 32 * (40960 // 6) and ic.gate(1) == 32 * (40960 // 3)
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(cl.IsingMcError):
            cl.icm_plan(bad)


# ---- statistics ----
@pytest.mark.parametrize("name", list(cc.ENUM_SYSTEMS))
def test_host_cluster_moves_match_exact_enumeration(oracle, name):
    """The inputs of test_host_overlaps_match_exact_enumeration with cluster moves at every temperature: 1024 groups of 2 copies of the
    ladder beta |J| = 0.2 .. 1.0 (T = 4), 48 rounds of one only_basic_moves step from random states.  Q^2 / N^2 and QL of the last round
    and the energy of each copy after the last round's moves have means within 4.5 exact standard deviations over sqrt(1024) of the
    enumerated values at every temperature.  Measured: at most 2.0 sigma over the three systems, four temperatures and four
    quantities."""
    cl = _cl()
    edges, biases = cc.ENUM_SYSTEMS[name]
    init = pc.initial_states(cc.SEED, pc.ENUM_PT_CHAINS * 4, len(biases))
    out = cl.host_tempering_run(edges, biases, cc.SEED, init, 0, pc.enum_pt_betas(name), pc.ENUM_PT_ROUNDS, 1, only_basic_moves=True, ncopies=2, cluster_moves=(0, None))
    assert out["overlap"].shape == (pc.ENUM_PT_ROUNDS, oc.ENUM_GROUPS, 1, 4) and oc.ENUM_GROUPS == 1024
    assert ((out["cluster_moves"] + out["cluster_empty"]) == pc.ENUM_PT_ROUNDS).all() and out["cluster_moves"].sum() > 98304
    sigmas = ic.enum_icm_sigmas(name, out["overlap"][-1, :, 0, :], out["link_overlap"][-1, :, 0, :], out["energy"][-1])
    print(name, sigmas)
    assert max(max(s) for s in sigmas) <= cc.ENUM_SIGMAS, sigmas
