"""The independent checker of the classical Monte Carlo entry points: GraphState (src/classical/graph.rs) restated in Python from the
reference's source, move by move, with the Philox streams of include/sse_format.h (tags CLASSICAL / CLASSICAL_WORM) in place of its
rng.  `RefGraphState` is the literal, one-replica form (the worm keeps its candidate stack and its path as the reference does);
`BatchRef` steps many replicas at once with numpy for the statistics tests (spin and edge steps only).  Philox comes from the oracle
library's ora_philox4x32_10; the numpy form of it is checked against that function where it is used.  Test infrastructure only."""
import ctypes as C
import math

import numpy as np

import _oracle as O

TAG_INIT, TAG_CLASSICAL, TAG_WORM = 0, 8, 9
EPS = float(np.finfo(np.float64).eps)
M32 = 0xFFFFFFFF


def philox(seed, index, epoch, replica, tag):
    """The four words of the counter (index, epoch_lo, replica, tag << 24 | epoch_hi24) under the key `seed`."""
    ctr = (C.c_uint32 * 4)(index & M32, epoch & M32, replica & M32, (tag << 24) | ((epoch >> 32) & 0xFFFFFF))
    key = (C.c_uint32 * 2)(seed & M32, (seed >> 32) & M32)
    out = (C.c_uint32 * 4)()
    O.lib().ora_philox4x32_10(ctr, key, out)
    return [int(x) for x in out]


def philox_np(seed, index, epoch, replica, tag):
    """philox() for arrays of index / epoch / replica (broadcast together): uint64 array [..., 4]."""
    index, epoch, replica = np.broadcast_arrays(np.asarray(index, dtype=np.uint64), np.asarray(epoch, dtype=np.uint64), np.asarray(replica, dtype=np.uint64))
    m = np.uint64(M32)
    c0, c1, c2 = index & m, epoch & m, replica & m
    c3 = np.uint64(tag << 24) | ((epoch >> np.uint64(32)) & np.uint64(0xFFFFFF))
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & m, n2, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def umulhi(word, n):
    return (int(word) * int(n)) >> 32


def u01(word):
    return float(word) * (1.0 / 4294967296.0)


def random_state(seed, replica, nvars):
    """make_random_spin_state (graph.rs:451-453) as the library draws it: bit 31 of word 0, tag INIT, epoch 0, index = variable."""
    return np.array([philox(seed, v, 0, replica, TAG_INIT)[0] >> 31 for v in range(nvars)], dtype=np.uint8)


def binding_mat(edges, nvars):
    """graph.rs:69-78: push (vb, j) to va's row and (va, j) to vb's in edge order, then a stable sort of each row by neighbour."""
    rows = [[] for _ in range(nvars)]
    for (va, vb), j in edges:
        rows[va].append((vb, float(j)))
        rows[vb].append((va, float(j)))
    for r in rows:
        r.sort(key=lambda t: t[0])
    return rows


def cumulative_weights(edges):
    """enable_edge_importance_sampling (graph.rs:320-336)."""
    v, acc = [], 0.0
    for _, w in edges:
        acc = acc + float(w)
        v.append(acc)
    return v, acc


def get_energy(edges, biases, state):
    """graph.rs:430-447"""
    mat = binding_mat(edges, len(biases))
    acc = 0.0
    for i, si in enumerate(state):
        total_e = 0.0
        for indx, j in mat[i]:
            total_e += j * (1.0 if bool(si) == bool(state[indx]) else -1.0) / 2.0
        bias_e = -float(biases[i]) if si else float(biases[i])
        acc = acc + total_e + bias_e
    return acc


# counters as isingmc_classical_counters lays them out
C_SPIN, C_SPIN_ACC, C_EDGE, C_EDGE_ACC, C_WORM, C_WORM_ACC, C_WORM_FAIL, C_WORM_PATH = range(8)
KINDS_ALL, KINDS_BASIC, KINDS_SPIN, KINDS_EDGE, KINDS_WORM, KINDS_WORM_NO_DOUBLES = range(6)


class RefGraphState:
    """One replica.  `kinds` as in the C ABI; wrong rules for the tests of the tests: bias_sign = -1 reverses the bias term of
    every move, edge_omit = False drops the `omit` filter from the edge move."""

    def __init__(self, edges, biases, seed, replica=0, state=None, epoch=0, importance=False, bias_sign=1.0, edge_omit=True):
        self.edges = [((int(a), int(b)), float(j)) for (a, b), j in edges]
        self.biases = [float(h) for h in biases]
        self.n = len(self.biases)
        self.mat = binding_mat(self.edges, self.n)
        self.seed, self.replica, self.epoch = int(seed), int(replica), int(epoch)
        self.state = [bool(x) for x in (random_state(seed, replica, self.n) if state is None else state)]
        self.cum = cumulative_weights(self.edges) if importance else None
        self.counters = [0] * 8
        self.bias_sign, self.edge_omit = bias_sign, edge_omit

    # ---- the stream ----
    def _move_words(self, i):
        w = philox(self.seed, 1 + i, self.epoch, self.replica, TAG_CLASSICAL)
        return w[0], w[1]

    def _worm_word(self):
        w = philox(self.seed, self._ndraw, self.epoch, self.replica, TAG_WORM)[0]
        self._ndraw += 1
        return w

    @staticmethod
    def should_flip(beta, delta_e, word_fn):
        """graph.rs:339-347; word_fn is called only when a number is drawn"""
        if delta_e > 0.0:
            return u01(word_fn()) < math.exp(-beta * delta_e)
        return True

    # ---- energies ----
    def delta_e(self, v, omit):
        curr = self.state[v]
        de = 0.0
        for ov, j in self.mat[v]:
            if omit is not None and ov == omit:
                continue
            old_coupling = 1.0 if not (curr ^ self.state[ov]) else -1.0
            de += -2.0 * j * old_coupling
        return de

    def bias_e(self, v):
        return self.bias_sign * (2.0 * self.biases[v] * (1.0 if self.state[v] else -1.0))

    # ---- moves ----
    def do_spin_flip(self, beta, i):
        choice, uword = self._move_words(i)
        v = umulhi(choice, self.n)
        de = self.delta_e(v, None) + self.bias_e(v)
        self.counters[C_SPIN] += 1
        if self.should_flip(beta, de, lambda: uword):
            self.state[v] = not self.state[v]
            self.counters[C_SPIN_ACC] += 1

    def do_edge_flip(self, beta, i):
        choice, uword = self._move_words(i)
        if self.cum is not None:
            cum, totalw = self.cum
            p = u01(choice) * totalw
            lo, hi = 0, len(cum)  # binary_search_by: Ok(i) and Err(i) both give the first index whose weight is not below p
            while lo < hi:
                mid = (lo + hi) // 2
                if cum[mid] < p:
                    lo = mid + 1
                else:
                    hi = mid
            e = lo
        else:
            e = umulhi(choice, len(self.edges))
        (va, vb), _ = self.edges[e]
        one = lambda a, b: self.delta_e(a, b if self.edge_omit else None) + self.bias_e(a)
        de = one(va, vb) + one(vb, va)
        self.counters[C_EDGE] += 1
        if self.should_flip(beta, de, lambda: uword):
            self.state[va] = not self.state[va]
            self.state[vb] = not self.state[vb]
            self.counters[C_EDGE_ACC] += 1

    def _move_de(self, wm):
        if len(wm) == 1:
            return self.delta_e(wm[0], None)
        de = self.delta_e(wm[0], wm[1])
        return de + self.delta_e(wm[1], wm[0])

    def do_worm_flip(self, beta, allow_doubles):
        """graph.rs:179-318, with its candidate stack and its path.  A move is (v,) or (va, vb)."""
        st = self.state
        start = umulhi(self._worm_word(), self.n)
        visit_path = [(start,)]
        last_index = start
        starting_e = self._move_de((start,))
        st[start] = not st[start]
        update_failed = False
        while True:
            stack = []
            sel_move = visit_path[-1]
            sel_var = sel_move[-1]
            any_resolve = False
            for ov, _ in self.mat[sel_var]:
                if ov == last_index:
                    continue
                de = self._move_de((ov,))
                if abs(de) < EPS:
                    stack.append(((ov,), de))
                elif abs(de + starting_e) < EPS:
                    stack.append(((ov,), de))
                    any_resolve = True
                if allow_doubles:
                    st[ov] = not st[ov]
                    for oov, _ in self.mat[ov]:
                        if oov != ov and oov != sel_var:
                            de2 = self._move_de((oov,)) + de
                            if abs(de2) < EPS:
                                stack.append(((ov, oov), de2))
                            elif abs(de2 + starting_e) < EPS:
                                stack.append(((ov, oov), de2))
                                any_resolve = True
                    st[ov] = not st[ov]
            if any_resolve:
                stack = [(m, de) for m, de in stack if abs(de + starting_e) < EPS]
            if stack:
                choice = umulhi(self._worm_word(), len(stack))
                ov, de = stack[choice]
                visit_path.append(ov)
            else:
                ov = sel_move if len(sel_move) == 1 else (sel_move[1], sel_move[0])
                visit_path.append(ov)
                de = self._move_de(ov)
            for v in ov:
                st[v] = not st[v]
            last_index = ov[0] if len(ov) == 2 else sel_move[-1]
            if abs(de + starting_e) < EPS:
                break
            if len(visit_path) > len(st):
                update_failed = True
                break
        self.counters[C_WORM] += 1
        self.counters[C_WORM_PATH] += len(visit_path)
        flat = sorted(v for m in visit_path for v in m)
        net = O.remove_doubles(flat) if flat else []
        keep = False
        if not update_failed:
            total_he = 0.0
            for v in net:
                total_he += self.bias_e(v)
            keep = self.should_flip(beta, total_he, self._worm_word)
        else:
            self.counters[C_WORM_FAIL] += 1
        if keep:
            self.counters[C_WORM_ACC] += 1
        else:
            for v in net:
                st[v] = not st[v]

    def do_time_step(self, beta, nspin=None, nedge=None, nworm=None, kinds=KINDS_ALL):
        """graph.rs:350-406; a forced kind draws no kind word.  Every step consumes one epoch."""
        nspin = max(1, self.n // 2) if nspin is None else nspin
        nedge = max(1, len(self.edges) // 2) if nedge is None else nedge
        nworm = 1 if nworm is None else nworm
        if kinds in (KINDS_ALL, KINDS_BASIC):
            choice = umulhi(philox(self.seed, 0, self.epoch, self.replica, TAG_CLASSICAL)[0], 2 if kinds == KINDS_BASIC else 3)
        else:
            choice = {KINDS_SPIN: 0, KINDS_EDGE: 1}.get(kinds, 2)
        if choice == 0:
            for i in range(nspin):
                self.do_spin_flip(beta, i)
        elif choice == 1:
            for i in range(nedge):
                self.do_edge_flip(beta, i)
        else:
            self._ndraw = 0
            for _ in range(nworm):
                self.do_worm_flip(beta, kinds != KINDS_WORM_NO_DOUBLES)
        self.epoch += 1

    def timesteps(self, t, beta, **kw):
        for _ in range(t):
            self.do_time_step(beta, **kw)

    def state_bytes(self):
        return np.array(self.state, dtype=np.uint8)

    def get_energy(self):
        return get_energy(self.edges, self.biases, self.state)


class BatchRef:
    """R replicas stepped together (numpy), spin and edge steps drawn per step as only_basic_moves does: the same rule and the same
    streams as RefGraphState (np.exp in place of libm's exp).  bias_sign / edge_omit: the wrong rules of RefGraphState."""

    def __init__(self, edges, biases, seed, nreplicas, replica_offset=0, bias_sign=1.0, edge_omit=True):
        self.edges = [((int(a), int(b)), float(j)) for (a, b), j in edges]
        self.h = np.asarray(biases, dtype=np.float64)
        self.n, self.R, self.seed = len(self.h), int(nreplicas), int(seed)
        self.rep = np.arange(self.R, dtype=np.uint64) + np.uint64(replica_offset)
        mat = binding_mat(self.edges, self.n)
        deg = max(len(r) for r in mat)
        self.nbr = np.zeros((self.n, deg), dtype=np.int64)
        self.J = np.zeros((self.n, deg))
        self.valid = np.zeros((self.n, deg), dtype=bool)
        for v, row in enumerate(mat):
            for k, (ov, j) in enumerate(row):
                self.nbr[v, k], self.J[v, k], self.valid[v, k] = ov, j, True
        self.ea = np.array([a for (a, _), _ in self.edges], dtype=np.int64)
        self.eb = np.array([b for (_, b), _ in self.edges], dtype=np.int64)
        idx = np.arange(self.n, dtype=np.uint64)
        self.state = (philox_np(self.seed, idx[None, :], 0, self.rep[:, None], TAG_INIT)[..., 0] >> np.uint64(31)).astype(bool)
        self.epoch = 0
        self.bias_sign, self.edge_omit = bias_sign, edge_omit

    def _delta_e(self, rows, v, omit):
        """delta_e of variable v[i] of replica rows[i], entries towards omit[i] left out (omit None: none); row order"""
        sv = self.state[rows, v]
        de = np.zeros(len(rows))
        for k in range(self.nbr.shape[1]):
            ov = self.nbr[v, k]
            use = self.valid[v, k] if omit is None else (self.valid[v, k] & (ov != omit))
            term = -2.0 * self.J[v, k] * np.where(sv == self.state[rows, ov], 1.0, -1.0)
            de = np.where(use, de + term, de)
        return de

    def _bias_e(self, rows, v):
        return self.bias_sign * (2.0 * self.h[v] * np.where(self.state[rows, v], 1.0, -1.0))

    def _accept(self, beta, de, uword):
        with np.errstate(over="ignore"):
            return (de <= 0.0) | (uword.astype(np.float64) * (1.0 / 4294967296.0) < np.exp(-beta * de))

    def do_time_step(self, beta):
        beta = np.broadcast_to(np.asarray(beta, dtype=np.float64), (self.R,))
        kind = (philox_np(self.seed, 0, self.epoch, self.rep, TAG_CLASSICAL)[:, 0] * np.uint64(2)) >> np.uint64(32)
        nspin, nedge = max(1, self.n // 2), max(1, len(self.edges) // 2)
        spin_rows, edge_rows = np.flatnonzero(kind == 0), np.flatnonzero(kind == 1)
        for i in range(nspin):
            rows = spin_rows
            w = philox_np(self.seed, 1 + i, self.epoch, self.rep[rows], TAG_CLASSICAL)
            v = ((w[:, 0] * np.uint64(self.n)) >> np.uint64(32)).astype(np.int64)
            de = self._delta_e(rows, v, None) + self._bias_e(rows, v)
            acc = self._accept(beta[rows], de, w[:, 1])
            self.state[rows[acc], v[acc]] ^= True
        for i in range(nedge):
            rows = edge_rows
            w = philox_np(self.seed, 1 + i, self.epoch, self.rep[rows], TAG_CLASSICAL)
            e = ((w[:, 0] * np.uint64(len(self.edges))) >> np.uint64(32)).astype(np.int64)
            va, vb = self.ea[e], self.eb[e]
            de = ((self._delta_e(rows, va, vb if self.edge_omit else None) + self._bias_e(rows, va)) +
                  (self._delta_e(rows, vb, va if self.edge_omit else None) + self._bias_e(rows, vb)))
            acc = self._accept(beta[rows], de, w[:, 1])
            self.state[rows[acc], va[acc]] ^= True
            self.state[rows[acc], vb[acc]] ^= True
        self.epoch += 1

    def timesteps(self, t, beta):
        for _ in range(t):
            self.do_time_step(beta)


def exact_moments(edges, biases, beta):
    """Boltzmann mean and variance of E, m = sum_v (2 s_v - 1) / N and m^2 by enumeration (N <= ~12), with H = get_energy:
    {name: (mean, standard deviation of one sample)}."""
    n = len(biases)
    states = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(bool)
    spin = np.where(states, 1.0, -1.0)
    en = np.zeros(1 << n)
    for (a, b), j in edges:  # each edge appears in two rows with weight j / 2
        en += j * spin[:, a] * spin[:, b]
    en += -(spin * np.asarray(biases, dtype=np.float64)[None, :]).sum(axis=1)  # s true: -h, false: +h
    w = np.exp(-beta * (en - en.min()))
    w /= w.sum()
    m = spin.mean(axis=1)
    out = {}
    for name, x in (("E", en), ("m", m), ("m2", m * m)):
        mean = float((w * x).sum())
        out[name] = (mean, float(np.sqrt(max((w * (x - mean) ** 2).sum(), 0.0))))
    return out


def sample_moments(edges, biases, states):
    """The same three observables of sampled states [R][N]: {name: array [R]}."""
    spin = np.where(np.asarray(states).astype(bool), 1.0, -1.0)
    en = np.zeros(len(spin))
    for (a, b), j in edges:
        en += j * spin[:, a] * spin[:, b]
    en += -(spin * np.asarray(biases, dtype=np.float64)[None, :]).sum(axis=1)
    m = spin.mean(axis=1)
    return {"E": en, "m": m, "m2": m * m}
