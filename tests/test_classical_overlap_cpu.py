"""Overlaps between copies of a realisation without a device: isingmc_classical_host_pt_run_overlaps (csrc/classical_overlap_rule.h
by the sequential rule) against the numpy restatement (tests/_classical_overlap_cases.py), against exact enumeration of pairs of
states, and its argument checks.  Every compared value is an integer: every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _classical_cases as cc
import _classical_overlap_cases as oc
import _classical_pt_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


RULE_MAIN = """#include "classical_overlap_rule.h"
struct Bits { uint32_t w; bool get(uint32_t v) const { return ((w >> v) & 1u) != 0u; } };
struct Ring { uint32_t n; uint32_t E() const { return n; } void edge(uint32_t e, uint32_t &a, uint32_t &b) const { a = e; b = (e + 1u) % n; } };
int main() {
    uint32_t a, b, g, p, t, bad = 0;
    cmc_ov_pair(4, 0, a, b); bad += !(a == 0 && b == 1);
    cmc_ov_pair(4, 2, a, b); bad += !(a == 0 && b == 3);
    cmc_ov_pair(4, 3, a, b); bad += !(a == 1 && b == 2);
    cmc_ov_pair(4, 5, a, b); bad += !(a == 2 && b == 3);
    cmc_ov_item(3 * 6 * 5 + 4 * 5 + 2, 6, 5, g, p, t); bad += !(g == 3 && p == 4 && t == 2);
    const Bits A{0x0Fu}, B{0x3Cu};  // d = 0x33: 4 of 8 variables differ, and on the ring of 8 the edges 1, 3, 5, 7 have one such endpoint
    bad += cmc_ov_count_spins(8, A, B, 0, 1) != 4 || cmc_ov_count_spins(8, A, B, 1, 2) != 2 || cmc_ov_count_links(Ring{8}, A, B, 0, 1) != 4;
    bad += cmc_ov_overlap(8, 4) != 0 || cmc_ov_overlap(8, 8) != -8 || cmc_ov_pairs(4) != 6;
    return (int)bad;
}
"""


def test_rule_header_is_plain_cpp(tmp_path):
    """classical_overlap_rule.h compiles on its own under g++ -Wall -Wextra -Werror: no HIP header, no device code."""
    src = tmp_path / "rule.cpp"
    src.write_text(RULE_MAIN)
    exe = str(tmp_path / "rule")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "isingmontecarlo_amd", "csrc"), str(src), "-o", exe])
    assert subprocess.call([exe]) == 0


@pytest.mark.parametrize("name", list(oc.CASES))
def test_host_run_matches_the_restatement(oracle, name):
    """Both series and both histograms on every GPU parity case, and E and M with them."""
    c = oc.CASES[name]
    want = oc.host_parity_reference(name)
    series, hq, hl = oc.restatement_run(name)
    for key in oc.SERIES:
        assert np.array_equal(series[key], want[key]), key
    assert np.array_equal(hq, want["overlap_hist"]) and np.array_equal(hl, want["link_hist"])
    groups, pairs = c["chains"] // c["ncopies"], len(oc.pairs_of(c["ncopies"]))
    assert want["overlap"].shape == (c["rounds"], groups, pairs, len(c["betas"])) and want["overlap"].dtype == np.int32
    assert want["overlap_hist"].shape[3] == len(c["biases"]) + 1 and want["link_hist"].shape[3] == len(c["edges"]) + 1
    assert want["accepts"].sum() > 0  # the labels moved: pairing by temperature is not pairing by slot


@pytest.mark.parametrize("name", ["ring33_T3_K2", "ring65_T3_K3", "k8_per_replica_T2_K2"])
def test_measuring_disturbs_nothing(oracle, name):
    """With ncopies given, states, epochs, counters, temp_of, swap counts, E and M equal those of host_tempering_run without it."""
    cl = _cl()
    c = oc.CASES[name]
    want = oc.host_parity_reference(name)
    plain = pc.host_run(cl, c["edges"], c["biases"], c["betas"], c["chains"], c["rounds"], c["steps"], replica_offset=oc.offset(name), kinds=cl.KINDS_ALL,
                        couplings=c["couplings"])
    assert set(want) - set(plain) == {"overlap", "link_overlap", "overlap_hist", "link_hist"}
    for key in plain:
        assert np.array_equal(plain[key], want[key]), key


@pytest.mark.parametrize("name", list(oc.CASES))
def test_histogram_identities(oracle, name):
    """Every (g, p, t) row sums to the number of measured rounds; hq is the bincount of (N - overlap) / 2, hl that of (E - link) / 2."""
    c = oc.CASES[name]
    want = oc.host_parity_reference(name)
    for hist, series, total in ((want["overlap_hist"], want["overlap"], len(c["biases"])), (want["link_hist"], want["link_overlap"], len(c["edges"]))):
        assert (hist.sum(axis=3) == c["rounds"]).all()
        assert ((total - series) % 2 == 0).all() and (np.abs(series) <= total).all()
        n = (total - series.astype(np.int64)) // 2
        for g, p, t in np.ndindex(hist.shape[:3]):
            assert np.array_equal(hist[g, p, t], np.bincount(n[:, g, p, t], minlength=total + 1))


def test_histograms_accumulate_over_calls_and_without_the_series(oracle):
    """10 rounds = 3 + 7 with the histograms handed on; record = False gives the same histograms and no series."""
    cl = _cl()
    edges, biases = cc.CASES["ring33"]
    betas = [0.2, 0.5, 1.0, 2.0]
    whole = oc.host_run(cl, edges, biases, betas, 4, 2, 10, 2, kinds=cl.KINDS_ALL)
    a = oc.host_run(cl, edges, biases, betas, 4, 2, 3, 2, kinds=cl.KINDS_ALL)
    b = cl.host_tempering_run(edges, biases, cc.SEED, a["states"], a["epochs"], betas, 7, 2, kinds=cl.KINDS_ALL, temp_of=a["temp_of"], pt_step=a["pt_step"], ncopies=2,
                              histograms=(a["overlap_hist"], a["link_hist"]))
    assert (a["overlap_hist"].sum(axis=3) == 3).all()  # (the second call worked on copies)
    for key in oc.HISTS + ("states", "temp_of"):
        assert np.array_equal(whole[key], b[key]), key
    for key in ("overlap", "link_overlap"):
        assert np.array_equal(whole[key], np.concatenate([a[key], b[key]])), key
    quiet = oc.host_run(cl, edges, biases, betas, 4, 2, 10, 2, kinds=cl.KINDS_ALL, record=False)
    assert "overlap" not in quiet and all(np.array_equal(quiet[key], whole[key]) for key in oc.HISTS)
    lo = oc.host_run(cl, edges, biases, betas, 2, 2, 10, 2, replica_offset=0, kinds=cl.KINDS_ALL)
    hi = oc.host_run(cl, edges, biases, betas, 2, 2, 10, 2, replica_offset=8, kinds=cl.KINDS_ALL)
    for key in oc.HISTS:  # two groups = two batches of one group at the offsets 0 and K T
        assert np.array_equal(whole[key], np.concatenate([lo[key], hi[key]])), key
    assert np.array_equal(whole["overlap"], np.concatenate([lo["overlap"], hi["overlap"]], axis=1))


def test_every_refusal(oracle):
    """Every ISINGMC_EINVAL of overlap_attach through the host entry that shares its check, and the null handle.  (Overlaps before
    tempering, and the overlap calls before overlap_attach, need a handle: tests/test_gpu_classical_overlap.py.)"""
    cl = _cl()
    edges, biases = cc.CASES["triangle"]
    ok = dict(edges=edges, biases=biases, seed=1, states=np.zeros((12, 3), dtype=np.uint8), epochs=0, betas=[0.5, 1.0, 2.0], rounds=1, steps=1, ncopies=2)
    out = cl.host_tempering_run(**ok)
    assert out["overlap"].shape == (1, 2, 1, 3) and (out["overlap_hist"].sum(axis=3) == 1).all()
    rows = np.tile(np.array([1.0, 0.0, -1.0]), (12, 1))
    assert cl.host_tempering_run(**ok, couplings=rows)["pt_step"] == 1
    other, signed = rows.copy(), rows.copy()
    other[9:12] = [1.0, 0.5, -1.0]  # the second chain of group 1 is another realisation (a whole chain: tempering itself accepts it)
    signed[3:6, 1] = -0.0           # the second chain of group 0 differs from the first in the sign of a zero
    assert cl.host_tempering_run(**{**ok, "ncopies": None}, couplings=other)["pt_step"] == 1
    for change, words in [
        (dict(ncopies=1), "ncopies >= 2"),
        (dict(ncopies=0), "ncopies >= 2"),
        (dict(ncopies=3), "multiple of ncopies"),
        (dict(ncopies=8), "multiple of ncopies"),
        (dict(replica_offset=3), "a group does not straddle"),
        (dict(replica_offset=9), "a group does not straddle"),
        (dict(couplings=other), "group 1 (replicas 6 .. 11) differ"),
        (dict(couplings=signed), "group 0 (replicas 0 .. 5) differ"),
        (dict(betas=[1.0]), "ntemps >= 2"),  # tempering's own refusals come first
        (dict(replica_offset=4), "replica_offset must be a multiple"),
    ]:
        with pytest.raises(cl.IsingMcError) as ei:
            cl.host_tempering_run(**{**ok, **change})
        assert ei.value.code == -1 and words in str(ei.value), (change, str(ei.value))
    assert cl.host_tempering_run(**{**ok, "replica_offset": 6})["pt_step"] == 1  # a whole group further on
    import isingmontecarlo_amd as im
    lib = im.load_library()
    assert lib.isingmc_classical_overlap_attach(None, 2) == -1 and lib.isingmc_classical_overlap_reset(None) == -1
    assert lib.isingmc_classical_overlap_histograms(None, None, None) == -1 and lib.isingmc_classical_overlap_set_histograms(None, None, None) == -1
    assert lib.isingmc_classical_pt_run_overlaps(None, 1, 1, 1, 1, 1, 0, None, None, None, None) == -1
    # every output of the host entry may be null
    ed, js, hs = cl._model(edges, biases)
    cfg = cl._config(ed, js, hs, 1, 12)
    st, ep, tof, step = np.zeros((12, 3), dtype=np.uint8), np.zeros(12, dtype=np.uint64), np.arange(12, dtype=np.uint32) % 3, C.c_uint64(0)
    ladder = np.array([0.5, 1.0, 2.0])
    args = [1, 1, cl.NONE, cl.NONE, cl.NONE, 0, im._ptr(st, C.c_uint8), im._ptr(ep, C.c_uint64), im._ptr(tof, C.c_uint32), C.byref(step)] + [None] * 9
    assert lib.isingmc_classical_host_pt_run_overlaps(C.byref(cfg), 3, im._ptr(ladder, C.c_double), 2, *args) == 0 and step.value == 1
    assert np.array_equal(st, out["states"])


@pytest.mark.parametrize("name", list(cc.ENUM_SYSTEMS))
def test_host_overlaps_match_exact_enumeration(oracle, name):
    """1024 groups of 2 copies of the ladder beta |J| = 0.2 .. 1.0 (T = 4), R = 8192, 48 rounds of one only_basic_moves step from random
    states.  Q^2 / N^2 and QL of the last round, one sample per group, have means within 4.5 exact standard deviations over sqrt(1024)
    of the values enumerated over the pairs of states, at every temperature.  Measured: at most 1.7 sigma over the three systems, four temperatures and two observables."""
    cl = _cl()
    edges, biases = cc.ENUM_SYSTEMS[name]
    out = oc.host_run(cl, edges, biases, pc.enum_pt_betas(name), pc.ENUM_PT_CHAINS, 2, pc.ENUM_PT_ROUNDS, 1, only_basic_moves=True)
    assert out["overlap"].shape == (pc.ENUM_PT_ROUNDS, oc.ENUM_GROUPS, 1, 4) and oc.ENUM_GROUPS == 1024
    sigmas = oc.enum_overlap_sigmas(name, out["overlap"][-1, :, 0, :], out["link_overlap"][-1, :, 0, :])
    assert max(max(s) for s in sigmas) <= cc.ENUM_SIGMAS, sigmas
    assert (out["overlap_hist"].sum(axis=3) == pc.ENUM_PT_ROUNDS).all()


def test_enumeration_inputs_catch_pairing_by_slot(oracle):
    """The test of the test: on the restatement alone, at the inputs of the test above for frustrated2x4, pairing the copies by
    temperature passes and equals the host entry, and pairing them by slot index (the states of equal position in their chains,
    whatever temperatures they hold) misses the bound.  Observed sigmas per temperature (q2, ql):
      temperature   0.3  0.3    1.0  0.9    0.6  0.1    0.0  0.0
      slot         20.0 21.6   11.2 11.0    6.7 10.3   26.4 35.4"""
    cl = _cl()
    name = "frustrated2x4"
    edges, biases = cc.ENUM_SYSTEMS[name]
    seen = {}
    for pairing in oc.PAIRINGS:
        ref = oc.OverlapRef(edges, biases, cc.SEED, pc.enum_pt_betas(name), pc.ENUM_PT_CHAINS, 2, basic=True, pairing=pairing)
        got = ref.run(pc.ENUM_PT_ROUNDS, 1)
        seen[pairing] = oc.enum_overlap_sigmas(name, got["overlap"][-1, :, 0, :], got["link_overlap"][-1, :, 0, :])
        if pairing == "temperature":
            host = oc.host_run(cl, edges, biases, pc.enum_pt_betas(name), pc.ENUM_PT_CHAINS, 2, pc.ENUM_PT_ROUNDS, 1, only_basic_moves=True)
            assert np.array_equal(got["overlap"], host["overlap"]) and np.array_equal(got["link_overlap"], host["link_overlap"])
            assert np.array_equal(ref.hq, host["overlap_hist"]) and np.array_equal(ref.hl, host["link_hist"])
    assert max(max(s) for s in seen["temperature"]) <= cc.ENUM_SIGMAS, seen
    assert max(max(s) for s in seen["slot"]) > cc.ENUM_SIGMAS, seen
