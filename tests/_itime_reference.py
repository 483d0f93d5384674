"""The imaginary-time fold of two-valued observables and the bond counts, restated the slow way.  Test infrastructure only.

OpContainer::itime_fold (fast_ops.rs:1296-1315) hands the fold function the propagated state BEFORE every slot's op.  fold() does
just that: it propagates the state slot by slot, keeps the state in front of every slot, and evaluates every group on every one of
them.  It knows nothing of events or of where an observable changes (csrc/sse_itime.h is what it checks)."""
import numpy as np


def tfim_bond_vars(edges, nvars, longitudinal):
    """Bond -> variables of a transverse-field Ising batch (include/sse_format.h): [0, E) edges, [E, E + N) transverse field,
    [E + N, E + 2N) longitudinal field when there is one.  int64 [Nb][2], -1 for the missing second variable."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    single = np.stack([np.arange(nvars, dtype=np.int64), np.full(nvars, -1, dtype=np.int64)], axis=1)
    parts = [edges, single] + ([single] if abs(longitudinal) > np.finfo(np.float64).eps else [])
    return np.concatenate(parts, axis=0)


def generic_bond_vars(interactions):
    """Bond -> variables of a batch of generic interactions [(mat, vars), ...]: bond b = interaction b."""
    return np.array([[vs[0], vs[1] if len(vs) == 2 else -1] for _, vs in interactions], dtype=np.int64)


def states_before_slots(state, ops, bond_vars, keep=None):
    """uint8 [M][len(keep)]: the propagated state in front of slot p's op, p = 0 .. M - 1 (an op writes its output bits), for the
    variables `keep` (default: all), and the state behind the last slot (all variables)."""
    st = np.asarray(state, dtype=np.uint8).copy()
    keep = np.arange(len(st)) if keep is None else np.asarray(keep, dtype=np.int64)
    out = np.zeros((len(ops), len(keep)), dtype=np.uint8)
    for p, w in enumerate(ops):
        out[p] = st[keep]
        w = int(w)
        if w:
            a, c = bond_vars[(w >> 4) - 1]
            st[a] = (w >> 2) & 1
            if c >= 0:
                st[c] = (w >> 3) & 1
    return out, st


def fold(state, ops, bond_vars, groups, flips=None):
    """(sum_all [G], sum_occ [G]) of one replica: the sums over all slots, and over the occupied slots, of x_g(p) = +-1, the value of
    group g (parity of its variables' bits ^ flip, 1 standing for +1; a variable listed twice counts twice) on the state in front
    of slot p.  Also checks periodicity."""
    ops = np.asarray(ops, dtype=np.uint32)
    groups = [np.atleast_1d(np.asarray(g, dtype=np.int64)) for g in groups]
    keep = np.unique(np.concatenate(groups))  # only the variables some group reads are kept per slot
    before, last = states_before_slots(state, ops, bond_vars, keep)
    assert np.array_equal(last, np.asarray(state, dtype=np.uint8)), "the op-string does not return to its p = 0 state"
    fl = np.zeros(len(groups), dtype=np.uint8) if flips is None else np.asarray(flips, dtype=np.uint8) & 1
    occupied = ops != 0
    sum_all, sum_occ = np.zeros(len(groups), dtype=np.int64), np.zeros(len(groups), dtype=np.int64)
    for g, vs in enumerate(groups):
        bits = np.bitwise_xor.reduce(before[:, np.searchsorted(keep, vs)], axis=1) ^ fl[g]  # [M]
        x = 2 * bits.astype(np.int64) - 1
        sum_all[g], sum_occ[g] = x.sum(), x[occupied].sum()
    return sum_all, sum_occ


def bond_counts(ops, nbonds):
    ops = np.asarray(ops, dtype=np.uint32)
    return np.bincount((ops[ops != 0] >> 4).astype(np.int64) - 1, minlength=nbonds).astype(np.uint32)


def fold_replicas(reps, bond_vars, groups, flips=None):
    """fold() over oracle replicas: int64 [R][G] twice."""
    res = [fold(rep.state(), rep.ops(), bond_vars, groups, flips) for rep in reps]
    return np.stack([a for a, _ in res]), np.stack([b for _, b in res])
