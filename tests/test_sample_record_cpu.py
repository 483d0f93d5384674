"""CPU tests of the sample record's host side: bit_autocorrelation (the yardstick of csrc/sse_observe.hip.h's kernel) against the
defining circular sum, the observable groups of the reference's three autocorrelations, and the record entry points' null checks."""
import ctypes as C

import numpy as np
import pytest

import _lattices as lat

SHAPES = [(48, 16), (77, 5), (1000, 33), (4096, 7)]


def correlated_bits(seed, tmax, n, p_flip=0.1, constant=None):
    """[T][n] of 0/1: every column a two-state Markov chain (a flip with probability p_flip per step); column `constant` never changes."""
    rng = np.random.default_rng(seed)
    flips = rng.random((tmax, n)) < p_flip
    flips[0] = rng.random(n) < 0.5
    if constant is not None:
        flips[1:, constant] = False
    return (np.cumsum(flips, axis=0) & 1).astype(np.uint8)


@pytest.mark.parametrize("tmax,n", SHAPES)
def test_bit_autocorrelation_matches_the_direct_sum(tmax, n):
    """C(tau) = T - 2 popcount(bits ^ rot(bits, tau)) with centring and unit norm in integers equals the O(T^2) float sum over the
    +-1 series to 1e-10 (test_variable_autocorrelation_values' tolerance for the same comparison); one column is constant and
    contributes 0 at every lag."""
    from isingmontecarlo_amd.autocorrelations import bit_autocorrelation, direct_autocorrelation
    bits = correlated_bits(1000 + tmax, tmax, n, constant=n // 2)
    got = bit_autocorrelation(bits)
    want = direct_autocorrelation(bits.astype(np.float64) * 2.0 - 1.0)
    assert got.shape == (tmax,) and got.dtype == np.float64
    err = np.abs(got - want).max()
    print("bit vs direct", tmax, n, err)
    assert err < 1e-10
    nconst = int((bits.min(axis=0) == bits.max(axis=0)).sum())
    assert nconst >= 1 and abs(got[0] - (1.0 - nconst / n)) < 1e-10


def test_bit_autocorrelation_of_constant_and_single_sample_series_is_zero():
    from isingmontecarlo_amd.autocorrelations import bit_autocorrelation
    assert np.array_equal(bit_autocorrelation(np.ones((9, 3), dtype=np.uint8)), np.zeros(9))
    assert np.array_equal(bit_autocorrelation(np.array([[0, 1, 1]])), np.zeros(1))
    with pytest.raises(ValueError):
        bit_autocorrelation(np.zeros((0, 3)))


@pytest.mark.parametrize("tmax,n", SHAPES[:3])
def test_bit_autocorrelation_does_not_depend_on_flips(tmax, n):
    """x -> -x leaves x[t] x[t + tau], s^2 and therefore every integer of the computation unchanged: flipping any subset of columns
    gives the same bits of the result (this is why isingmc_record_autocorrelation takes no flips)."""
    from isingmontecarlo_amd.autocorrelations import bit_autocorrelation
    bits = correlated_bits(7 + n, tmax, n, constant=0)
    base = bit_autocorrelation(bits)
    rng = np.random.default_rng(5)
    for _ in range(4):
        mask = (rng.random(n) < 0.5).astype(np.uint8)
        assert np.array_equal(bit_autocorrelation(bits ^ mask), base)
    assert np.array_equal(bit_autocorrelation(bits ^ 1), base)


class _Graph:
    """What bond_groups / bond_values ask of a graph."""
    def __init__(self, edges):
        self.edges = np.array([[a, b] for (a, b), _ in edges], dtype=np.uint32)
        self.J = np.array([j for _, j in edges], dtype=np.float64)
        self.nvars = int(self.edges.max()) + 1


def value_for_bond(edges, bond, sample):
    """qmc_ising.rs:988-997, literally"""
    edge, j = edges[bond]
    even = len([i for i in edge if sample[i]]) % 2 == 0
    val = even if j < 0.0 else (not even)
    return 1.0 if val else -1.0


def test_bond_values_match_the_reference_definition():
    from isingmontecarlo_amd.autocorrelations import bond_values, bond_groups
    edges = lat.two_d_periodic(4)  # couplings of both signs
    assert {j for _, j in edges} == {-1.0, 1.0}
    g = _Graph(edges)
    rng = np.random.default_rng(11)
    states = (rng.random((6, 3, g.nvars)) < 0.5).astype(np.uint8)
    got = bond_values(g, states)
    assert got.shape == (6, 3, len(edges)) and got.dtype == np.float64
    for t in range(6):
        for r in range(3):
            want = [value_for_bond(edges, b, states[t, r].astype(bool)) for b in range(len(edges))]
            assert got[t, r].tolist() == want
    groups, flips = bond_groups(g)
    assert groups == [[a, b] for (a, b), _ in edges] and flips.tolist() == [1 if j < 0 else 0 for _, j in edges]


def test_groups_and_flips_give_the_reference_observables():
    """parity(group bits) ^ flip is 1 exactly where the reference's observable is +1: variables, products of even and odd length, bonds."""
    from isingmontecarlo_amd.autocorrelations import variable_groups, product_groups, bond_groups
    edges = lat.two_d_periodic(4)
    g = _Graph(edges)
    rng = np.random.default_rng(2)
    states = (rng.random((40, g.nvars)) < 0.5).astype(np.uint8)
    pm = states.astype(np.float64) * 2.0 - 1.0

    def observe(groups, flips):
        return np.stack([(states[:, vs].sum(axis=1) + int(f)) & 1 for vs, f in zip(groups, flips)], axis=1)

    groups, flips = variable_groups(g.nvars)
    assert groups == [[v] for v in range(g.nvars)] and not flips.any()
    assert np.array_equal(observe(groups, flips), states)
    prods = [(0, 1), (2, 3, 4), (5,), (1, 6, 7, 15), (0, 3, 8, 9, 10)]
    groups, flips = product_groups(prods)
    assert flips.tolist() == [1, 0, 0, 1, 0]
    want = np.stack([pm[:, list(vs)].prod(axis=1) for vs in prods], axis=1)
    assert np.array_equal(observe(groups, flips) * 2.0 - 1.0, want)
    groups, flips = bond_groups(g)
    want = np.array([[value_for_bond(edges, b, s.astype(bool)) for b in range(len(edges))] for s in states])
    assert np.array_equal(observe(groups, flips) * 2.0 - 1.0, want)


def test_bond_groups_refuse_generic_interactions():
    import isingmontecarlo_amd as im
    from isingmontecarlo_amd.autocorrelations import bond_groups

    class Generic(_Graph):
        interactions = [(np.ones(16), [0, 1])]

    with pytest.raises(im.IsingMcError) as ei:
        bond_groups(Generic([((0, 1), 1.0)]))
    assert ei.value.code == -5


def test_record_entry_points_reject_a_null_handle():
    import isingmontecarlo_amd as im
    lib = im.load_library()
    n, cap = C.c_uint32(7), C.c_uint32(9)
    start = (C.c_uint32 * 2)(0, 1)
    vs = (C.c_uint32 * 1)(0)
    flip = (C.c_uint8 * 1)(0)
    bits = (C.c_uint32 * 1)(0)
    out8 = (C.c_uint8 * 4)()
    outd = (C.c_double * 1)(0.0)
    assert lib.isingmc_record_attach(None, 16) == -1
    assert lib.isingmc_record_count(None, C.byref(n), C.byref(cap)) == -1 and (n.value, cap.value) == (7, 9)
    assert lib.isingmc_record_clear(None) == -1
    assert lib.isingmc_record_read(None, 0, 1, 0, out8) == -1
    assert lib.isingmc_record_series(None, 1, start, vs, flip, 0, 1, bits) == -1
    assert lib.isingmc_record_autocorrelation(None, 1, start, vs, 0, 1, outd) == -1
    for name in ("attach_sample_record", "detach_sample_record", "record_count", "record_clear", "record_states", "record_series",
                 "record_autocorrelation", "timesteps_sample"):
        assert callable(getattr(im.QmcIsingGraph, name)) and callable(getattr(im.Qmc, name))
