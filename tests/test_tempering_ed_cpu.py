"""The tempering rule against exact diagonalisation (ED), on the CPU: a chain with swaps switched on must still sample each
temperature's Gibbs ensemble, and a wrong rule must be seen.

The tempering parity tests prove that the kernel, the host path and the oracle take the same decisions; a wrong decision that all
three share (a wrong exponent, swapped arguments of relative_weight, sweeps credited to the wrong slot's accumulator row) keeps
them green.  Here oracle replicas run under tests/_pt_reference.py (one sweep, then one tempering step), and per slot the energy,
|m|, m^2 and <sigma_x> of the measured sweeps (the accumulator rows, turned into observables as tests/test_gpu_ed_statistics.py
does) are compared with ED computed in the test (tests/golden/make_ed_golden.py:thermal), each slot with its own beta, Hamiltonian
and offset.  tests/test_gpu_tempering_ed.py does the same with the HIP path at 8 times the statistics or more.

Statistics.  The independent unit is the chain: the slots of one chain are correlated through the swaps.
  * per slot t and observable: z_t = (mean over chains - exact_t) / (std over chains / sqrt K);
  * lean of a ladder: per chain k, S_k = sum_t (x_tk - exact_t) / sd_t with sd_t the std over chains at slot t, and
    z_lean = mean_k S_k / (std_k S_k / sqrt K): a proper z whatever the correlation between the slots;
  * gates: |z_t| < 4.5 at every slot and |z_lean| < 3.5, for each of the four observables (Z_POINT, Z_AGGREGATE of the sweep module);
  * condition: accepted / attempted swaps >= 0.3 over the measured steps, or the test would reduce to the sweep test.
Every replica starts at the fixed cutoff of the coldest slot, 2 <n> + 64 (see tests/test_gpu_ed_statistics.py for why a fixed
cutoff), so the per-chain equalisation never changes a cutoff; the test asserts that none grew.  300 warm-up steps.

The test of the test: six wrong rules run through reference_pt's `accept` hook on the same row, seed and gates.  Each must fail
the gates, and the statistics are chosen so that each reaches |z| >= 6 (MUTANT_Z) on a slot's energy or on the energy's lean
while the correct rule passes.

Measured (fixed seeds, so these are the values the test sees; z of the energy per slot, hot to cold, then the largest |z_t| of
any observable and the largest |z_lean|):

  row, rule                          chains x steps  swap rate  energy z_t                                        energy z_lean  max |z_t|  max |z_lean|
  a_ring4_afm, correct                   512 x 600      0.608    +0.07   +0.46   -0.10   -0.07   -0.23   +0.53        +0.23        1.97      1.08
  b_ring6_fm_long, correct              1024 x 800      0.427    +1.56   +0.64   -0.66   -1.07   -0.21   +1.65        +0.69        2.51      0.78
  c_ring4_hams, correct                  512 x 600      0.516    +1.39   +0.11   -0.22   -1.39                        -0.05        1.88      0.62
  a_ring4_afm, inverted_exponent         512 x 600      0.904  -187.49 -123.64  -56.02  +11.87 +104.39 +206.49       -13.85      206.49     31.78
  a_ring4_afm, always_accept             512 x 600      1.000  -154.94 -101.19  -48.17   +0.15  +80.97 +156.72       -21.67      156.72     47.21
  a_ring4_afm, off_by_one                512 x 600      0.531   +13.98   +6.08   +0.46   -2.07   -4.01   -5.77        +3.03       14.17      6.30
  c_ring4_hams, rel_dropped              512 x 600      0.587   -15.14   -1.56   +5.11   +5.46                        -2.63       26.89      7.56
  c_ring4_hams, rel_one_side             512 x 600      0.708   -36.83   -5.62  +11.40  +26.23                        -2.03       43.48     11.56
  c_ring4_hams, rel_inverted             512 x 600      0.693   -55.98   -7.43  +21.35  +28.57                        -5.57       76.16     13.06

(off_by_one at 128 chains x 400 steps, same seed: largest energy |z_t| 5.85, energy z_lean +0.48: the statistics make this test.)  The whole
module takes about 80 s on 8 cores; reference_pt sweeps all replicas in one threaded call and decides a pair of slots for all
chains at once, which is what made these statistics affordable (the same decisions, bit for bit, as one chain at a time).
"""

import numpy as np
import pytest

import _oracle as O
import _pt_reference as ptref
from test_gpu_ed_statistics import OBS, SYSTEMS, Z_AGGREGATE, Z_POINT, _ed_module, capacity_for, fixed_cutoff, observables, offset_of, seed_of

WARMUP = 300
MIN_SWAP_RATE = 0.3
MUTANT_Z = 6.0


def ring(n, j):
    return [(i, (i + 1) % n, j) for i in range(n)]


def _slot_rows(n, edges, gamma, h, betas):
    """One Hamiltonian for all slots."""
    return [dict(n=n, edges=list(edges), gamma=gamma, h=h, beta=float(b)) for b in betas]


def ring4_afm(betas=None):
    """Row (a): 4-site antiferromagnetic ring, J = +1, Gamma = 1, h = 0."""
    return _slot_rows(4, ring(4, 1.0), 1.0, 0.0, np.geomspace(0.25, 1.0, 6) if betas is None else betas)


def ring6_fm_long(betas=None):
    """Row (b): ring6_fm_long of tests/golden/ed_tfim.json, J = -1, Gamma = 1, h = 0.3."""
    c = SYSTEMS["ring6_fm_long"]
    edges = [(a, b, j) for (a, b), j in zip(c["edges"], c["J"])]
    return _slot_rows(c["nvars"], edges, c["gamma"], c["h"], np.geomspace(0.7, 2.0, 6) if betas is None else betas)


def slot_hamiltonians(n, betas, dj, dg, dh):
    """Ferromagnetic n-ring whose Hamiltonian changes with the slot: J_t = -(1 + dj t), Gamma_t = 0.8 + dg t, h_t = 0.30 - dh t.  Every
    h_t stays well away from 0: relative_weight skips the longitudinal ratio when |h_from| <= epsilon, a corner that is not physics."""
    rows = [dict(n=n, edges=ring(n, -(1.0 + dj * t)), gamma=0.8 + dg * t, h=0.30 - dh * t, beta=float(b)) for t, b in enumerate(betas)]
    assert all(r["h"] > 0.1 for r in rows)
    return rows


def ring4_hams(betas=None):
    """Row (c)."""
    return slot_hamiltonians(4, np.geomspace(0.5, 0.9, 4) if betas is None else betas, 0.1, 0.1, 0.04)


def ring4_hams_common_beta():
    """Row (c)'s Hamiltonians at one common beta: swaps are decided by the relative weights alone (the reference's test_bondstrength
    situation, tempering_container.rs:830-858)."""
    return ring4_hams(np.full(4, 0.7))


def ring6_hams():
    """Six slots on the 6-ring: J_t = -(1 + 0.05 t), Gamma_t = 0.8 + 0.05 t, h_t = 0.30 - 0.02 t."""
    return slot_hamiltonians(6, np.geomspace(1.0, 1.6, 6), 0.05, 0.05, 0.02)


# lat3x3_villain from beta = 1 to 4.  The number of temperatures comes from oracle runs (64 chains, 100 warm-up + 200 measured steps,
# geomspace): 8 temperatures swap at a rate of 0.21, 10 at 0.33, 12 at 0.42, 14 at 0.49, 16 at 0.55.  12 keeps a margin over 0.3.
VILLAIN_TEMPERATURES = 12


def villain_ladder():
    c = SYSTEMS["lat3x3_villain"]
    edges = [(a, b, j) for (a, b), j in zip(c["edges"], c["J"])]
    return _slot_rows(c["nvars"], edges, c["gamma"], c["h"], np.geomspace(1.0, 4.0, VILLAIN_TEMPERATURES))


# row id -> (slots, chains, measured steps).  The GPU twins (tests/test_gpu_tempering_ed.py) run at least 8 times chains * steps.
ROWS = {
    "a_ring4_afm": (ring4_afm, 512, 600),
    "b_ring6_fm_long": (ring6_fm_long, 1024, 800),
    "c_ring4_hams": (ring4_hams, 512, 600),
}


def differ(slots):
    first = {k: v for k, v in slots[0].items() if k != "beta"}
    return any({k: v for k, v in s.items() if k != "beta"} != first for s in slots)


def slot_offset(s):
    return offset_of(dict(J=[j for _, _, j in s["edges"]], nvars=s["n"], gamma=s["gamma"], h=s["h"]))


def exact_of(slots):
    """ED per slot, computed here."""
    ed = _ed_module()
    return [ed.thermal(s["n"], s["edges"], s["gamma"], s["h"], s["beta"]) for s in slots]


def start_cutoff(slots, exact):
    """The fixed cutoff of the coldest slot."""
    t = int(np.argmax([s["beta"] for s in slots]))
    return fixed_cutoff(slots[t]["beta"], slot_offset(slots[t]), exact[t]["energy"])


def ladder_statistics(acc, slots, exact, K, offsets=None):
    """acc[T*K][8], row t*K + k -> (z[obs][t], lean[obs]) as the module docstring defines them."""
    T = len(slots)
    acc = np.asarray(acc)
    assert acc.shape[0] == T * K
    z, lean = {}, {}
    per_slot = [observables(acc[t * K:(t + 1) * K], s["beta"], slot_offset(s) if offsets is None else offsets[t], s["gamma"], s["n"])
                for t, s in enumerate(slots)]
    for k in OBS:
        x = np.array([per_slot[t][k] for t in range(T)])  # [T][K]
        ex = np.array([exact[t][k] for t in range(T)])[:, None]
        sd = x.std(axis=1, ddof=1)[:, None]
        z[k] = ((x.mean(axis=1, keepdims=True) - ex) / (sd / np.sqrt(K)))[:, 0]
        s_k = ((x - ex) / sd).sum(axis=0)
        lean[k] = float(s_k.mean() / (s_k.std(ddof=1) / np.sqrt(K)))
    return z, lean


def table(what, z, lean, rate):
    lines = [f"{what}: swap rate {rate:.3f}"]
    for k in OBS:
        lines.append(f"  {k:>6} z_t " + " ".join(f"{v:+6.2f}" for v in z[k]) + f"   z_lean {lean[k]:+.2f}")
    return "\n".join(lines)


def violations(z, lean):
    bad = [(k, t, round(float(v), 2)) for k in OBS for t, v in enumerate(z[k]) if not abs(v) < Z_POINT]
    bad += [(k, "lean", round(lean[k], 2)) for k in OBS if not abs(lean[k]) < Z_AGGREGATE]
    return bad


def check_ladder(what, z, lean, rate):
    """The gates and the swap-rate condition; prints the z table either way."""
    print("\n" + table(what, z, lean, rate))
    assert rate >= MIN_SWAP_RATE, f"{what}: swap rate {rate:.3f} < {MIN_SWAP_RATE}: the row tests the sweep, not the swaps"
    bad = violations(z, lean)
    assert not bad, f"{what}: beyond the gates ({Z_POINT} per slot, {Z_AGGREGATE} lean): {bad}\n{table(what, z, lean, rate)}"


def slot_arrays(slots, K):
    """(edges, J[T*K][E], gamma[T*K], h[T*K]) with row t*K + k."""
    e = [[a, b] for a, b, _ in slots[0]["edges"]]
    assert all([[a, b] for a, b, _ in s["edges"]] == e for s in slots)
    J = np.repeat(np.array([[j for _, _, j in s["edges"]] for s in slots], dtype=np.float64), K, axis=0)
    return e, J, np.repeat([s["gamma"] for s in slots], K).astype(np.float64), np.repeat([s["h"] for s in slots], K).astype(np.float64)


def run_reference(row, slots, K, steps, accept=None, flags=0, warmup=WARMUP):
    """The row under reference_pt: (z, lean, swap rate).  Asserts that no cutoff grew."""
    exact = exact_of(slots)
    cut = start_cutoff(slots, exact)
    betas = [s["beta"] for s in slots]
    e, J, gam, h = slot_arrays(slots, K)
    hams = model = None
    if differ(slots):
        hams = ptref.SlotHamiltonians(slots[0]["n"], e, J, gam, h)
    else:
        model = O.Model(slots[0]["n"], e, list(J[0]), slots[0]["gamma"], slots[0]["h"])
    ref = ptref.reference_pt(model, betas, K, seed_of(row), capacity_for(cut), cut, warmup + steps, 1, flags=flags, hams=hams,
                             accept=accept, warmup=warmup)
    assert ref.attempts == (len(slots) - 1) * K * steps and (ref.acc[:, 1] == steps).all()
    grew = [r.cutoff for chain in ref.by_slot for r in chain if r.cutoff != cut]
    assert not grew, f"{row}: cutoffs grew from {cut}: {grew[:4]}"
    z, lean = ladder_statistics(ref.acc, slots, exact, K)
    return z, lean, ref.swaps / ref.attempts


# ---- the wrong rules ----
def inverted_exponent(bt, bt1, na, nb, rel):
    return ptref.powi(bt / bt1, na - nb) * rel


def always_accept(bt, bt1, na, nb, rel):
    return np.full(np.shape(na), 2.0)


def off_by_one(bt, bt1, na, nb, rel):
    return ptref.powi(bt / bt1, nb - na + 1) * rel


def rel_dropped(bt, bt1, na, nb, rel):
    return ptref.powi(bt / bt1, nb - na)


def rel_one_side(bt, bt1, na, nb, rel):
    return ptref.powi(bt / bt1, nb - na) * rel[0]


rel_one_side.sides = True


def rel_inverted(bt, bt1, na, nb, rel):
    return ptref.powi(bt / bt1, nb - na) / rel


MUTANTS = [("a_ring4_afm", inverted_exponent), ("a_ring4_afm", always_accept), ("a_ring4_afm", off_by_one),
           ("c_ring4_hams", rel_dropped), ("c_ring4_hams", rel_one_side), ("c_ring4_hams", rel_inverted)]


@pytest.mark.parametrize("row", list(ROWS))
def test_correct_rule_matches_ed(oracle, row):
    make, K, steps = ROWS[row]
    z, lean, rate = run_reference(row, make(), K, steps)
    check_ladder(f"{row} {K} chains x {steps} steps", z, lean, rate)


@pytest.mark.parametrize("row,rule", MUTANTS, ids=[f"{r}-{f.__name__}" for r, f in MUTANTS])
def test_wrong_rule_is_seen(oracle, row, rule):
    """The same row, seed and gates with a wrong rule: it must fail the gates, by |z| >= 6 on a slot's energy or the energy's lean."""
    make, K, steps = ROWS[row]
    z, lean, rate = run_reference(row, make(), K, steps, accept=rule)
    print("\n" + table(f"{row} with {rule.__name__}", z, lean, rate))
    assert violations(z, lean), f"{rule.__name__} passes the gates on {row}"
    reach = max(float(np.abs(z["energy"]).max()), abs(lean["energy"]))
    assert reach >= MUTANT_Z, f"{rule.__name__} on {row}: largest energy |z| {reach:.2f} < {MUTANT_Z}: the row lacks the power to see it"


# rows that only the GPU module runs at full statistics: here at a glance, for the swap-rate condition (and the gates, which are free)
GPU_ONLY_ROWS = {"villain_ladder": (villain_ladder, 64, 200), "c_ring4_hams_common_beta": (ring4_hams_common_beta, 256, 400),
                 "ring6_hams": (ring6_hams, 256, 400)}


@pytest.mark.parametrize("row", list(GPU_ONLY_ROWS))
def test_rows_of_the_gpu_module_swap_on_the_oracle(oracle, row):
    make, K, steps = GPU_ONLY_ROWS[row]
    z, lean, rate = run_reference(row, make(), K, steps)
    check_ladder(f"{row} {K} chains x {steps} steps", z, lean, rate)


def test_hook_and_warmup_leave_the_default_alone(oracle):
    """reference_pt with the rule spelled out through the hook takes the decisions of the default, and a warm-up only leaves the
    first steps out of the counts: what it accumulates is the difference of two runs without one."""
    slots = ring4_hams()
    e, J, gam, h = slot_arrays(slots, 3)
    betas = [s["beta"] for s in slots]

    def run(nsteps, **kw):
        hams = ptref.SlotHamiltonians(4, e, J, gam, h)
        return ptref.reference_pt(None, betas, 3, 4242, 1024, 8, nsteps, 1, hams=hams, **kw)
    full, head = run(40), run(15)
    spelled = run(40, accept=lambda bt, bt1, na, nb, rel: ptref.powi(bt / bt1, nb - na) * rel)
    tail = run(40, warmup=15)
    assert 0 < full.swaps < full.attempts and spelled.swaps == full.swaps and np.array_equal(spelled.ids, full.ids)
    assert np.array_equal(spelled.acc, full.acc)
    assert np.array_equal(tail.ids, full.ids) and tail.swaps == full.swaps - head.swaps and tail.attempts == full.attempts - head.attempts
    assert np.array_equal(tail.pair_accepts, full.pair_accepts - head.pair_accepts) and np.array_equal(tail.acc, full.acc - head.acc)
