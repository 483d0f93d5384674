"""Classical Ising Monte Carlo on the device: `GraphState` (qmc::classical::GraphState, src/classical/graph.rs) for a batch of R
replicas of one graph (with `couplings`: of R disorder realisations on one graph), over the isingmc_classical_* entry points of include/isingmc_hip.h.  All moves run in gfx950 kernels
(csrc/sse_classical.hip.h), and so do replica exchange between the temperatures of a chain (csrc/sse_classical_pt.hip.h) and the overlaps between copies of a
realisation (csrc/sse_classical_overlap.hip.h) and the isoenergetic cluster moves between those copies (csrc/sse_classical_icm.hip.h); there is no CPU fallback.
`host_steps`, `host_tempering_run`, `host_cluster`, `plan` and `icm_plan` are the device-free test entries of the C ABI."""
import ctypes as C

import numpy as np

from . import ALL, IsingMcError, QmcIsingGraph, _ClassicalConfig, _ptr, load_library  # (imported at the end of the package's __init__)

__all__ = ["GraphState", "new_qmc_from_graph", "host_steps", "host_tempering_run", "host_cluster", "plan", "icm_plan", "CFG_EDGE_IMPORTANCE", "CFG_GLOBAL_TABLES", "CFG_SERIAL_MOVES",
           "CFG_PER_REPLICA_J", "CFG_GLOBAL_CODES",           "KINDS_ALL", "KINDS_BASIC", "KINDS_SPIN", "KINDS_EDGE", "KINDS_WORM", "KINDS_WORM_NO_DOUBLES", "COUNTERS"]

CFG_EDGE_IMPORTANCE, CFG_GLOBAL_TABLES, CFG_SERIAL_MOVES, CFG_PER_REPLICA_J, CFG_GLOBAL_CODES = 1, 2, 4, 8, 16
KINDS_ALL, KINDS_BASIC, KINDS_SPIN, KINDS_EDGE, KINDS_WORM, KINDS_WORM_NO_DOUBLES = range(6)
NONE = 0xFFFFFFFF  # the reference's None for the move counts
COUNTERS = ("spin_attempted", "spin_accepted", "edge_attempted", "edge_accepted", "worm_attempted", "worm_kept", "worm_failures", "worm_path_entries")


def _model(edges, biases):
    ed = np.ascontiguousarray(np.array([[a, b] for (a, b), _ in edges], dtype=np.uint32).reshape(-1, 2))
    js = np.ascontiguousarray(np.array([j for _, j in edges], dtype=np.float64))
    hs = np.ascontiguousarray(np.asarray(biases, dtype=np.float64))
    return ed, js, hs


def _couplings(couplings, js, nreplicas, flags):
    """(J array of the config, flags): `couplings` float64 [nreplicas][nedges] replaces the J of the edges and sets CFG_PER_REPLICA_J."""
    flags = int(flags)
    if couplings is None:
        if flags & CFG_PER_REPLICA_J:
            raise IsingMcError(-1, "CFG_PER_REPLICA_J needs the couplings argument")
        return js, flags
    cj = np.ascontiguousarray(np.asarray(couplings, dtype=np.float64))
    if cj.shape != (int(nreplicas), len(js)):
        raise IsingMcError(-1, "couplings must have shape [nreplicas][nedges]")
    return cj, flags | CFG_PER_REPLICA_J


def _config(ed, js, hs, seed, nreplicas, replica_offset=0, device=-1, init=None, flags=0):
    return _ClassicalConfig(struct_size=C.sizeof(_ClassicalConfig), nreplicas=int(nreplicas), nvars=len(hs), nedges=len(ed),
                            edges=_ptr(ed, C.c_uint32), J=_ptr(js, C.c_double), biases=_ptr(hs, C.c_double) if hs.any() else None,
                            seed=int(seed), replica_offset=int(replica_offset), device=int(device),
                            init_state=_ptr(init, C.c_uint8) if init is not None else None, flags=int(flags))


def _count(x):
    return NONE if x is None else int(x)


def _kinds(only_basic_moves, kinds):
    return (KINDS_BASIC if only_basic_moves else KINDS_ALL) if kinds is None else int(kinds)


def _plan_dict(out):
    return dict(waves=out[0], in_lds=out[1], lds_words=out[2], wave_words=out[3], tables=out[4], compact_couplings=bool(out[5]), packed_edges=bool(out[6]),
                coupling_format=out[7])


def plan(edges, biases, lds_bytes=160 * 1024, flags=0, couplings=None):
    """isingmc_classical_plan: the launch isingmc_classical_create would choose, without a device.  `couplings` [R][E]: the plan of a
    batch of R realisations (coupling_format: 0 shared, 1 per-replica codes, 2 per-replica doubles)."""
    lib = load_library()
    ed, js, hs = _model(edges, biases)
    nrep = 1 if couplings is None else len(couplings)
    js, flags = _couplings(couplings, js, nrep, flags)
    out = (C.c_uint32 * 8)()
    rc = lib.isingmc_classical_plan(C.byref(_config(ed, js, hs, 0, nrep, flags=flags)), int(lds_bytes), out)
    if rc:
        raise IsingMcError(rc, lib.isingmc_classical_last_error(None).decode())
    return _plan_dict(out)


def icm_plan(nvars, lds_bytes=160 * 1024):
    """isingmc_classical_icm_plan: the cluster-move launch of a model of `nvars` variables, without a device: {"waves": 4, 2 or 1,
    "lds_words": the dynamic LDS, "wave_words": one wave's three bit sets, "max_vars": the most variables the launch takes}."""
    lib = load_library()
    out = (C.c_uint32 * 4)()
    rc = lib.isingmc_classical_icm_plan(int(nvars), int(lds_bytes), out)
    if rc:
        raise IsingMcError(rc, lib.isingmc_classical_last_error(None).decode())
    return _icm_plan_dict(out)


def _icm_plan_dict(out):
    return dict(waves=out[0], lds_words=out[1], wave_words=out[2], max_vars=out[3])


def host_cluster(edges, biases, a, b, rank):
    """isingmc_classical_host_icm_cluster: the cluster of one isoenergetic cluster move between the states `a` and `b` [N], seeded at
    the `rank`-th variable (in increasing order) in which they differ: (mask uint8 [N], size)."""
    lib = load_library()
    ed, js, hs = _model(edges, biases)
    sa, sb = (np.ascontiguousarray(np.array(x, dtype=np.uint8).reshape(-1)) for x in (a, b))
    if len(sa) != len(hs) or len(sb) != len(hs):
        raise IsingMcError(-1, "state has the wrong length")
    mask, size = np.zeros(len(hs), dtype=np.uint8), C.c_uint32(0)
    rc = lib.isingmc_classical_host_icm_cluster(C.byref(_config(ed, js, hs, 0, 1)), _ptr(sa, C.c_uint8), _ptr(sb, C.c_uint8), int(rank), _ptr(mask, C.c_uint8),
                                                C.byref(size))
    if rc:
        raise IsingMcError(rc, lib.isingmc_classical_last_error(None).decode())
    return mask, int(size.value)


def _window(t_first, t_last):
    """The window as the C ABI takes it: t_last None -> 0 (every temperature from t_first on)."""
    return int(t_first), 0 if t_last is None else int(t_last)


def _cluster_counts(counts, shape):
    """Copies of (moves, empty, size_sum) as contiguous uint64 arrays of `shape`."""
    out = tuple(np.ascontiguousarray(np.array(x, dtype=np.uint64)) for x in counts)
    if len(out) != 3 or any(x.shape != tuple(shape) for x in out):
        raise IsingMcError(-1, "cluster-move counts have the wrong shape")
    return out


def _counts_dict(moves, empty, size_sum):
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(moves=moves, empty=empty, size_sum=size_sum, mean_size=size_sum.astype(np.float64) / moves.astype(np.float64))


def host_steps(edges, biases, seed, states, epochs, t, beta, nspinupdates=None, nedgeupdates=None, nwormupdates=None, only_basic_moves=None,
               kinds=None, replica_offset=0, flags=0, couplings=None):
    """isingmc_classical_host_steps: t time steps of the sequential rule on the CPU.  Returns (states, epochs, counters).
    `couplings` [R][E]: replica r runs on row r."""
    lib = load_library()
    ed, js, hs = _model(edges, biases)
    st = np.ascontiguousarray(np.array(states, dtype=np.uint8).reshape(-1, len(hs)))
    js, flags = _couplings(couplings, js, len(st), flags)
    ep = np.ascontiguousarray(np.broadcast_to(np.asarray(epochs, dtype=np.uint64), (len(st),)).copy())
    ctr = np.zeros((len(st), 8), dtype=np.uint64)
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(beta, dtype=np.float64), (len(st),)))
    rc = lib.isingmc_classical_host_steps(C.byref(_config(ed, js, hs, seed, len(st), replica_offset, flags=flags)), int(t), _ptr(b, C.c_double),
                                          _count(nspinupdates), _count(nedgeupdates), _count(nwormupdates), _kinds(only_basic_moves, kinds),
                                          _ptr(st, C.c_uint8), _ptr(ep, C.c_uint64), _ptr(ctr, C.c_uint64))
    if rc:
        raise IsingMcError(rc, lib.isingmc_classical_last_error(None).decode())
    return st, ep, ctr


def host_tempering_run(edges, biases, seed, states, epochs, betas, rounds, steps, nspinupdates=None, nedgeupdates=None, nwormupdates=None,
                       only_basic_moves=None, kinds=None, temp_of=None, pt_step=0, replica_offset=0, flags=0, record=True, couplings=None, ncopies=None,
                       histograms=None, cluster_moves=None, cluster_counts=None, measure=True):
    """isingmc_classical_host_pt_run: `rounds` rounds of (`steps` time steps, one tempering step) by the sequential rule on the CPU, for
    R = len(states) slots as chains of T = len(betas) temperatures.  Returns a dict: states [R][N], epochs [R], temp_of [R], pt_step,
    counters [R][8], attempts and accepts [C][T - 1], and with `record` energy and magnetization [rounds][C][T].  `couplings` [R][E]:
    the T rows of every chain must be equal (C realisations x T temperatures).
    With `ncopies` = K it is isingmc_classical_host_pt_run_overlaps: consecutive chains are G = C / K groups of K copies with
    P = K (K - 1) / 2 pairs, and the dict gains overlap_hist uint64 [G][P][T][N + 1] and link_hist [G][P][T][E + 1] (`histograms`:
    the pair (hq, hl) they continue from) and, with `record`, overlap and link_overlap int32 [rounds][G][P][T].
    With `cluster_moves` = (t_first, t_last) (t_last None: T) it is isingmc_classical_host_pt_run_icm: every round also makes the
    isoenergetic cluster moves of csrc/classical_icm_rule.h at the temperatures of the window, after its measurement and before its
    swaps (energy and magnetization are then the values after the moves), and the dict gains cluster_moves, cluster_empty and
    cluster_size_sum, uint64 [G][K // 2][T] (`cluster_counts`: the triple they continue from).  `measure` = False leaves the overlaps
    unmeasured in such a run."""
    lib = load_library()
    ed, js, hs = _model(edges, biases)
    st = np.ascontiguousarray(np.array(states, dtype=np.uint8).reshape(-1, len(hs)))
    nrep = len(st)
    js, flags = _couplings(couplings, js, nrep, flags)
    ep = np.ascontiguousarray(np.broadcast_to(np.asarray(epochs, dtype=np.uint64), (nrep,)).copy())
    ladder = None if betas is None else np.ascontiguousarray(np.asarray(betas, dtype=np.float64).reshape(-1))
    ntemps = 0 if ladder is None else len(ladder)
    chains = nrep // ntemps if ntemps and nrep % ntemps == 0 else 0
    tof = np.ascontiguousarray((np.arange(nrep, dtype=np.uint32) % max(ntemps, 1)) if temp_of is None else np.array(temp_of, dtype=np.uint32).reshape(-1))
    if len(tof) != nrep:
        raise IsingMcError(-1, "temp_of has the wrong length")
    step = C.c_uint64(int(pt_step))
    ctr = np.zeros((nrep, 8), dtype=np.uint64)
    att, acc = (np.zeros((chains, max(ntemps, 1) - 1), dtype=np.uint64) for _ in range(2))
    energy = np.zeros((int(rounds), chains, ntemps), dtype=np.float64) if record else None
    mag = np.zeros((int(rounds), chains, ntemps), dtype=np.int32) if record else None
    cfg = _config(ed, js, hs, seed, nrep, replica_offset, flags=flags)
    run = (int(rounds), int(steps), _count(nspinupdates), _count(nedgeupdates), _count(nwormupdates), _kinds(only_basic_moves, kinds), _ptr(st, C.c_uint8),
           _ptr(ep, C.c_uint64), _ptr(tof, C.c_uint32), C.byref(step), _ptr(ctr, C.c_uint64), _ptr(att, C.c_uint64), _ptr(acc, C.c_uint64),
           _ptr(energy, C.c_double) if record else None, _ptr(mag, C.c_int32) if record else None)
    betas_ptr = None if ladder is None else _ptr(ladder, C.c_double)
    icm = None
    if ncopies is None and cluster_moves is None:
        rc = lib.isingmc_classical_host_pt_run(C.byref(cfg), ntemps, betas_ptr, *run)
    else:
        k = 0 if ncopies is None else int(ncopies)
        groups, pairs = (chains // k, k * (k - 1) // 2) if k >= 2 and chains % k == 0 else (0, 0)  # (a shape the library refuses: empty outputs)
        shape = (groups, pairs, ntemps)
        q, ql = (np.zeros((int(rounds),) + shape, dtype=np.int32) if record else None for _ in range(2))
        hq, hl = np.zeros(shape + (len(hs) + 1,), dtype=np.uint64), np.zeros(shape + (len(ed) + 1,), dtype=np.uint64)
        if histograms is not None:
            hq, hl = _histograms(histograms, hq.shape, hl.shape)
        tail = (_ptr(q, C.c_int32) if record else None, _ptr(ql, C.c_int32) if record else None, _ptr(hq, C.c_uint64), _ptr(hl, C.c_uint64))
        if cluster_moves is None:
            rc = lib.isingmc_classical_host_pt_run_overlaps(C.byref(cfg), ntemps, betas_ptr, k, *run, *tail)
        else:
            cshape = (groups, k // 2, ntemps)
            icm = tuple(np.zeros(cshape, dtype=np.uint64) for _ in range(3)) if cluster_counts is None else _cluster_counts(cluster_counts, cshape)
            rc = lib.isingmc_classical_host_pt_run_icm(C.byref(cfg), ntemps, betas_ptr, k, *run, *tail, 1 if measure else 0, *_window(*cluster_moves),
                                                       *(_ptr(x, C.c_uint64) for x in icm))
    if rc:
        raise IsingMcError(rc, lib.isingmc_classical_last_error(None).decode())
    out = dict(states=st, epochs=ep, temp_of=tof, pt_step=int(step.value), counters=ctr, attempts=att, accepts=acc)
    if record:
        out.update(energy=energy, magnetization=mag)
    if ncopies is not None and (measure or cluster_moves is None):
        out.update(overlap_hist=hq, link_hist=hl)
        if record:
            out.update(overlap=q, link_overlap=ql)
    if icm is not None:
        out.update(cluster_moves=icm[0], cluster_empty=icm[1], cluster_size_sum=icm[2])
    return out


def _histograms(pair, hq_shape, hl_shape):
    """Copies of the histograms (hq, hl) as contiguous uint64 arrays of the given shapes."""
    hq, hl = (np.ascontiguousarray(np.array(x, dtype=np.uint64)) for x in pair)
    if hq.shape != tuple(hq_shape) or hl.shape != tuple(hl_shape):
        raise IsingMcError(-1, "overlap histograms have the wrong shape")
    return hq, hl


class GraphState:
    """R replicas of GraphState::new / new_with_state_and_rng (graph.rs:56-88): `edges` = [((a, b), J), ...], `biases` the
    longitudinal fields (their length is the number of variables), `seed` in place of the rng; `state` [N] or [R][N] (None: random).
    `couplings` (float64 [nreplicas][nedges]) gives every replica its own J values on the same graph (disorder realisations, as in
    QmcIsingGraph); the J of `edges` is then ignored.  Replica r runs exactly as a replica of a batch with J = couplings[r]."""

    def __init__(self, edges, biases, seed, state=None, nreplicas=1, replica_offset=0, device=-1, cfg_flags=0, couplings=None):
        self._lib = load_library()
        self._h = None
        self._edge_list = [((int(a), int(b)), float(j)) for (a, b), j in edges]
        self.edges, self.J, self.biases = _model(edges, biases)
        self.nvars, self.nreplicas = len(self.biases), int(nreplicas)
        self.seed, self.replica_offset, self.device = int(seed), int(replica_offset), int(device)
        cj, self._cfg_flags = _couplings(couplings, self.J, self.nreplicas, cfg_flags)
        self.couplings = None if couplings is None else cj  # [R][E], or None: the batch shares the J of its edges
        self._counter_base = np.zeros((self.nreplicas, 8), dtype=np.uint64)
        self._ladder = None  # the ladder of attach_tempering
        self._ncopies = None  # the copies per group of attach_overlaps
        self._icm_window = None  # (t_first, t_last) of attach_cluster_moves
        init = None
        if state is not None:
            st = np.asarray(state, dtype=np.uint8)
            if st.ndim == 1:
                st = np.broadcast_to(st, (self.nreplicas, self.nvars))
            init = np.ascontiguousarray(st)
            if init.shape != (self.nreplicas, self.nvars):
                raise IsingMcError(-1, "initial state has the wrong shape")
        self._create(init)

    def _create(self, init):
        cfg = _config(self.edges, self.J if self.couplings is None else self.couplings, self.biases, self.seed, self.nreplicas, self.replica_offset, self.device, init, self._cfg_flags)
        h = C.c_void_p()
        rc = self._lib.isingmc_classical_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise IsingMcError(rc, self._lib.isingmc_classical_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.isingmc_classical_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise IsingMcError(rc, self._lib.isingmc_classical_last_error(self._h).decode())

    # ---- updates ----
    def timesteps(self, t, beta, nspinupdates=None, nedgeupdates=None, nwormupdates=None, only_basic_moves=None, kinds=None):
        """t x do_time_step in one launch; beta a number or [R].  `kinds` (KINDS_*) forces one kind of step, for tests."""
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(beta, dtype=np.float64), (self.nreplicas,)))
        self._check(self._lib.isingmc_classical_timesteps(self._h, int(t), _ptr(b, C.c_double), _count(nspinupdates), _count(nedgeupdates),
                                                          _count(nwormupdates), _kinds(only_basic_moves, kinds)))

    def do_time_step(self, beta, nspinupdates=None, nedgeupdates=None, nwormupdates=None, only_basic_moves=None):
        """graph.rs:350-406"""
        self.timesteps(1, beta, nspinupdates, nedgeupdates, nwormupdates, only_basic_moves)

    def enable_edge_importance_sampling(self, enable):
        """graph.rs:320-336.  The cumulative weights are part of the device tables: the batch is rebuilt around its states, time-step
        counters and move counters."""
        flags = (self._cfg_flags | CFG_EDGE_IMPORTANCE) if enable else (self._cfg_flags & ~CFG_EDGE_IMPORTANCE)
        if flags == self._cfg_flags:
            return
        state, epoch, counters, attached = self.state_ref(), self.get_epoch(), self.counters(), self._attachments()
        old, self._cfg_flags = self._cfg_flags, flags
        handle, self._h = self._h, None
        try:
            self._create(state)
        except IsingMcError:
            self._h, self._cfg_flags = handle, old
            raise
        self._lib.isingmc_classical_destroy(handle)
        self.set_epoch(epoch)
        self._counter_base = counters
        self._restore_attachments(attached)

    # ---- the attachments: the state of each is its checkpoint keys, as save_checkpoint writes them ----
    def _attachments(self):
        """The keys of whatever is attached, in one dict (nothing attached: empty)."""
        parts = ((self._ladder, self._tempering_keys), (self._ncopies, self._overlap_keys), (self._icm_window, self._cluster_keys))
        return {k: v for attached, keys in parts if attached is not None for k, v in keys().items()}

    def _restore_attachments(self, z):
        """Attaches and restores what the mapping `z` holds the keys of (each is marked by its first key), in the order they depend on
        each other."""
        for key, restore in (("ladder", self._restore_tempering), ("ncopies", self._restore_overlaps), ("cluster_window", self._restore_cluster_moves)):
            if key in z:
                restore(z)

    # ---- parallel tempering (csrc/classical_pt_rule.h) ----
    def attach_tempering(self, betas):
        """The batch as C chains of T = len(betas) temperatures, slot r = c T + i starting at betas[i]; one ladder for all chains.
        Attaching again resets the maps, the swap counters and the step number, and detaches the overlaps (attach_overlaps) and the
        cluster moves (attach_cluster_moves)."""
        ladder = np.ascontiguousarray(np.asarray(betas, dtype=np.float64).reshape(-1))
        self._check(self._lib.isingmc_classical_pt_attach(self._h, len(ladder), _ptr(ladder, C.c_double)))
        self._ladder, self._ncopies, self._icm_window = ladder, None, None

    def _chains(self):
        if self._ladder is None:
            raise IsingMcError(-1, "tempering is not attached (attach_tempering)")
        return self.nreplicas // len(self._ladder), len(self._ladder)

    def tempering_run(self, rounds, steps, nspinupdates=None, nedgeupdates=None, nwormupdates=None, only_basic_moves=None, kinds=None, record=True,
                      overlaps=False, cluster_moves=False):
        """`rounds` rounds of (`steps` time steps of every slot at its temperature, one tempering step of every chain), enqueued on the
        device with one synchronisation at the end.  With `record`: {"energy": float64 [rounds][C][T], "magnetization": int32
        [rounds][C][T]}, by temperature, the values before each round's swaps; otherwise None.
        `overlaps` (after attach_overlaps): every round also measures the overlaps between the copies of every group, after its steps
        and before its swaps.  The histograms accumulate, and with `record` the dict also holds "overlap" and "link_overlap", int32
        [rounds][G][P][T].  Without `overlaps` nothing is measured and the histograms stay as they are (thermalisation).
        `cluster_moves` (after attach_cluster_moves): every round also makes the isoenergetic cluster moves between the copies of every
        group at the temperatures of the window, after its measurement and before its swaps; "energy" and "magnetization" are then the
        values after the moves.  Without it no cluster move is made and their counts stay as they are."""
        c, t = self._chains()
        energy = np.zeros((int(rounds), c, t), dtype=np.float64) if record else None
        mag = np.zeros((int(rounds), c, t), dtype=np.int32) if record else None
        run = (self._h, int(rounds), int(steps), _count(nspinupdates), _count(nedgeupdates), _count(nwormupdates), _kinds(only_basic_moves, kinds),
               _ptr(energy, C.c_double) if record else None, _ptr(mag, C.c_int32) if record else None)
        if cluster_moves and self._icm_window is None:
            raise IsingMcError(-1, "cluster moves are not attached (attach_cluster_moves)")
        if not overlaps:
            if cluster_moves:
                self._check(self._lib.isingmc_classical_pt_run_icm(*run, None, None, 0))
            else:
                self._check(self._lib.isingmc_classical_pt_run(*run))
            return {"energy": energy, "magnetization": mag} if record else None
        shape = self._overlap_shape()
        q, ql = (np.zeros((int(rounds),) + shape, dtype=np.int32) if record else None for _ in range(2))
        series = (_ptr(q, C.c_int32) if record else None, _ptr(ql, C.c_int32) if record else None)
        if cluster_moves:
            self._check(self._lib.isingmc_classical_pt_run_icm(*run, *series, 1))
        else:
            self._check(self._lib.isingmc_classical_pt_run_overlaps(*run, *series))
        return {"energy": energy, "magnetization": mag, "overlap": q, "link_overlap": ql} if record else None

    # ---- overlaps between copies of a realisation (csrc/classical_overlap_rule.h) ----
    def attach_overlaps(self, ncopies=2):
        """Consecutive chains as G = C / ncopies groups of `ncopies` independent copies of one realisation (with `couplings`: the chains
        of a group must hold the same rows); the P = K (K - 1) / 2 pairs of a group are (a, b), a < b, a-major.  Needs
        attach_tempering.  The histograms start at zero; ncopies = 0 detaches.  Either way the cluster moves are detached."""
        self._chains()
        self._check(self._lib.isingmc_classical_overlap_attach(self._h, int(ncopies)))
        self._ncopies = int(ncopies) if ncopies else None
        self._icm_window = None

    def _overlap_shape(self):
        """(G, P, T)"""
        if self._ncopies is None:
            raise IsingMcError(-1, "overlaps are not attached (attach_overlaps)")
        c, t = self._chains()
        return c // self._ncopies, self._ncopies * (self._ncopies - 1) // 2, t

    def overlap_histograms(self):
        """(hq, hl): uint64 [G][P][T][N + 1] by the number of differing variables nq (spin overlap Q = N - 2 nq) and uint64
        [G][P][T][E + 1] by the number of differing edges nl (link overlap QL = E - 2 nl); one count per measured round since
        attach_overlaps or reset_overlaps."""
        shape = self._overlap_shape()
        hq, hl = np.zeros(shape + (self.nvars + 1,), dtype=np.uint64), np.zeros(shape + (len(self.edges) + 1,), dtype=np.uint64)
        self._check(self._lib.isingmc_classical_overlap_histograms(self._h, _ptr(hq, C.c_uint64), _ptr(hl, C.c_uint64)))
        return hq, hl

    def reset_overlaps(self):
        self._overlap_shape()
        self._check(self._lib.isingmc_classical_overlap_reset(self._h))

    def overlap_moments(self):
        """From the spin-overlap histogram summed over the pairs of a group, per (group, temperature): {"q2": <q^2>, "q4": <q^4>,
        "binder": (3 - <q^4> / <q^2>^2) / 2}, float64 [G][T] each, q = Q / N.  NaN where nothing was measured."""
        hq = self.overlap_histograms()[0].sum(axis=1).astype(np.float64)  # [G][T][N + 1]
        q = (self.nvars - 2.0 * np.arange(self.nvars + 1)) / self.nvars
        with np.errstate(invalid="ignore", divide="ignore"):
            w = hq / hq.sum(axis=2, keepdims=True)
            q2, q4 = (w * q ** 2).sum(axis=2), (w * q ** 4).sum(axis=2)
            return {"q2": q2, "q4": q4, "binder": 0.5 * (3.0 - q4 / q2 ** 2)}

    def _overlap_keys(self):
        hq, hl = self.overlap_histograms()
        return dict(ncopies=np.array([self._ncopies], dtype=np.uint32), overlap_hist=hq, link_hist=hl)

    def _restore_overlaps(self, z):
        self.attach_overlaps(int(z["ncopies"][0]))
        shape = self._overlap_shape()
        hq, hl = _histograms((z["overlap_hist"], z["link_hist"]), shape + (self.nvars + 1,), shape + (len(self.edges) + 1,))
        self._check(self._lib.isingmc_classical_overlap_set_histograms(self._h, _ptr(hq, C.c_uint64), _ptr(hl, C.c_uint64)))

    # ---- isoenergetic cluster moves between the copies of a group (csrc/classical_icm_rule.h) ----
    def attach_cluster_moves(self, t_first=0, t_last=None, waves=None):
        """Houdayer / isoenergetic cluster moves at the ladder indices t_first <= t < t_last (None: T); needs attach_overlaps.  A round
        of tempering_run(cluster_moves=True) pairs the copies of a group (K // 2 disjoint pairs that rotate with the tempering step
        number) and, at every temperature of the window, flips in both states of a pair one connected cluster of the variables in which
        they differ.  Keep the window away from temperatures where those clusters percolate.  The counts start at zero;
        t_first = t_last = NONE detaches.  `waves` (1, 2 or 4, at most the launch plan's) runs the launch with fewer waves per workgroup
        than planned, for tests and A-B timing; the moves do not depend on it."""
        self._overlap_shape()
        first, last = _window(t_first, t_last)
        self._check(self._lib.isingmc_classical_icm_attach(self._h, first, last))
        if first == NONE and last == NONE:
            self._icm_window = None
            return
        lo, hi = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.isingmc_classical_icm_window(self._h, C.byref(lo), C.byref(hi)))
        self._icm_window = (int(lo.value), int(hi.value))
        if waves is not None:
            self._check(self._lib.isingmc_classical_icm_force_waves(self._h, int(waves)))

    def _cluster_shape(self):
        """(G, M, T)"""
        if self._icm_window is None:
            raise IsingMcError(-1, "cluster moves are not attached (attach_cluster_moves)")
        g, _, t = self._overlap_shape()
        return g, self._ncopies // 2, t

    def _cluster_counts(self):
        out = tuple(np.zeros(self._cluster_shape(), dtype=np.uint64) for _ in range(3))
        self._check(self._lib.isingmc_classical_icm_counts(self._h, *(_ptr(x, C.c_uint64) for x in out)))
        return out

    def cluster_move_counts(self):
        """{"moves", "empty", "size_sum"}: uint64 [G][K // 2][T], cumulative since attach_cluster_moves or reset_cluster_moves: the moves
        made, the items whose two states were equal, and the sizes of the flipped clusters added up (all zero outside the window);
        "mean_size": size_sum / moves, float64, NaN where no move was made."""
        return _counts_dict(*self._cluster_counts())

    def reset_cluster_moves(self):
        self._cluster_shape()
        self._check(self._lib.isingmc_classical_icm_reset(self._h))

    def cluster_move_plan(self):
        """isingmc_classical_icm_launch_plan: the cluster-move launch of this batch on its device; the dict of icm_plan()."""
        self._cluster_shape()
        out = (C.c_uint32 * 4)()
        self._check(self._lib.isingmc_classical_icm_launch_plan(self._h, out))
        return _icm_plan_dict(out)

    def _cluster_keys(self):
        moves, empty, size_sum = self._cluster_counts()
        return dict(cluster_window=np.array(self._icm_window, dtype=np.uint32), cluster_moves=moves, cluster_empty=empty, cluster_size_sum=size_sum)

    def _restore_cluster_moves(self, z):
        self.attach_cluster_moves(int(z["cluster_window"][0]), int(z["cluster_window"][1]))
        counts = _cluster_counts((z["cluster_moves"], z["cluster_empty"], z["cluster_size_sum"]), self._cluster_shape())
        self._check(self._lib.isingmc_classical_icm_set_counts(self._h, *(_ptr(x, C.c_uint64) for x in counts)))

    def temperature_of(self):
        """uint32 [R]: the index into the ladder of the temperature each slot holds."""
        self._chains()
        out = np.zeros(self.nreplicas, dtype=np.uint32)
        self._check(self._lib.isingmc_classical_pt_get(self._h, _ptr(out, C.c_uint32), None))
        return out

    def tempering_step_number(self):
        self._chains()
        step = C.c_uint64(0)
        self._check(self._lib.isingmc_classical_pt_get(self._h, None, C.byref(step)))
        return int(step.value)

    def slot_at(self):
        """uint32 [C][T]: the slot (within its chain) that holds each temperature: the inverse of temperature_of()."""
        c, t = self._chains()
        tof = self.temperature_of().reshape(c, t)
        out = np.zeros((c, t), dtype=np.uint32)
        np.put_along_axis(out, tof.astype(np.int64), np.broadcast_to(np.arange(t, dtype=np.uint32), (c, t)), axis=1)
        return out

    def states_by_temperature(self):
        """uint8 [C][T][N]: the state at each temperature of each chain."""
        c, t = self._chains()
        return np.take_along_axis(self.state_ref().reshape(c, t, self.nvars), self.slot_at().astype(np.int64)[:, :, None], axis=1)

    def swap_counts(self):
        """(attempts, accepts), uint64 [C][T - 1] each: swaps of the pairs (t, t + 1), cumulative since attach_tempering."""
        c, t = self._chains()
        att, acc = np.zeros((c, t - 1), dtype=np.uint64), np.zeros((c, t - 1), dtype=np.uint64)
        self._check(self._lib.isingmc_classical_pt_swap_counts(self._h, _ptr(att, C.c_uint64), _ptr(acc, C.c_uint64)))
        return att, acc

    def _tempering_keys(self):
        attempts, accepts = self.swap_counts()
        return dict(ladder=self._ladder.copy(), temp_of=self.temperature_of(), pt_step=np.array([self.tempering_step_number()], dtype=np.uint64),
                    swap_attempts=attempts, swap_accepts=accepts)

    def _restore_tempering(self, z):
        self.attach_tempering(z["ladder"])
        tof = np.ascontiguousarray(np.asarray(z["temp_of"], dtype=np.uint32).reshape(-1))
        att, acc = (np.ascontiguousarray(np.asarray(z[k], dtype=np.uint64)) for k in ("swap_attempts", "swap_accepts"))
        c, t = self._chains()
        if len(tof) != self.nreplicas or att.shape != (c, t - 1) or acc.shape != att.shape:
            raise IsingMcError(-1, "tempering state has the wrong shape")
        self._check(self._lib.isingmc_classical_pt_set(self._h, _ptr(tof, C.c_uint32), int(z["pt_step"][0])))
        self._check(self._lib.isingmc_classical_pt_set_swap_counts(self._h, _ptr(att, C.c_uint64), _ptr(acc, C.c_uint64)))

    def set_temperature_of(self, temp_of, pt_step=None):
        """isingmc_classical_pt_set: the map [R] (a permutation within each chain) and, unless None, the step number."""
        self._chains()
        tof = np.ascontiguousarray(np.asarray(temp_of, dtype=np.uint32).reshape(-1))
        if len(tof) != self.nreplicas:
            raise IsingMcError(-1, "temp_of has the wrong length")
        self._check(self._lib.isingmc_classical_pt_set(self._h, _ptr(tof, C.c_uint32), self.tempering_step_number() if pt_step is None else int(pt_step)))

    # ---- accessors ----
    def state_ref(self):
        out = np.zeros((self.nreplicas, self.nvars), dtype=np.uint8)
        self._check(self._lib.isingmc_classical_get_state(self._h, ALL, _ptr(out, C.c_uint8)))
        return out

    clone_state = state_ref

    def set_state(self, state, r=None):
        st = np.ascontiguousarray(np.asarray(state, dtype=np.uint8))
        if st.size != (self.nreplicas if r is None else 1) * self.nvars:  # graph.rs:425
            raise IsingMcError(-1, "state has the wrong length")
        self._check(self._lib.isingmc_classical_set_state(self._h, ALL if r is None else int(r), _ptr(st, C.c_uint8)))

    def get_epoch(self):
        out = np.zeros(self.nreplicas, dtype=np.uint64)
        self._check(self._lib.isingmc_classical_get_epoch(self._h, _ptr(out, C.c_uint64)))
        return out

    def set_epoch(self, epochs):
        ep = np.ascontiguousarray(np.broadcast_to(np.asarray(epochs, dtype=np.uint64), (self.nreplicas,)).copy())
        self._check(self._lib.isingmc_classical_set_epoch(self._h, _ptr(ep, C.c_uint64)))

    def get_energy(self):
        """graph.rs:430-447 for every replica, computed on the device: float64 [R]."""
        out = np.zeros(self.nreplicas, dtype=np.float64)
        self._check(self._lib.isingmc_classical_energies(self._h, _ptr(out, C.c_double)))
        return out

    def counters(self):
        """uint64 [R][8], columns COUNTERS: attempted and accepted moves per kind, worm failures, worm path entries."""
        out = np.zeros((self.nreplicas, 8), dtype=np.uint64)
        self._check(self._lib.isingmc_classical_counters(self._h, _ptr(out, C.c_uint64)))
        return out + self._counter_base

    def set_stream(self, stream_ptr):
        self._check(self._lib.isingmc_classical_set_stream(self._h, C.c_void_p(int(stream_ptr))))

    def synchronize(self):
        self._check(self._lib.isingmc_classical_synchronize(self._h))

    def launch_plan(self):
        """isingmc_classical_launch_plan: the launch this batch runs with, chosen from its device's own LDS size; the dict of plan()."""
        out = (C.c_uint32 * 8)()
        self._check(self._lib.isingmc_classical_launch_plan(self._h, out))
        return _plan_dict(out)

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._check(self._lib.isingmc_classical_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    # ---- checkpoint / resume ----
    def save_checkpoint(self, path):
        """States, time-step counters, move counters and options of every replica (.npz).  A batch built on the same model and seed and
        restored with load_checkpoint continues bit-exactly.  With tempering attached the file is format 2: it also holds the ladder, the
        map of slots to temperatures, the tempering step number and both swap counters; without, it is the format-1 file.  A batch with
        per-replica couplings writes format 3: `couplings` [R][E] next to the keys of format 1, and those of format 2 when tempering is
        attached.  A batch with overlaps attached writes format 4: the keys it would otherwise write, and `ncopies`, `overlap_hist`,
        `link_hist`.  A batch with cluster moves attached writes format 5: the keys it would otherwise write, and `cluster_window`
        (t_first, t_last), `cluster_moves`, `cluster_empty`, `cluster_size_sum`."""
        extra = self._attachments()
        fmt = 5 if "cluster_window" in extra else 4 if "ncopies" in extra else 3 if self.couplings is not None else 2 if extra else 1
        if self.couplings is not None:
            extra["couplings"] = self.couplings
        np.savez_compressed(path, format=np.array([fmt], dtype=np.uint32), edges=self.edges, J=self.J, biases=self.biases,
                            seed=np.array([self.seed], dtype=np.uint64), replica_offset=np.array([self.replica_offset], dtype=np.uint32),
                            importance=np.array([bool(self._cfg_flags & CFG_EDGE_IMPORTANCE)]), state=self.state_ref(), epoch=self.get_epoch(),
                            counters=self.counters(), **extra)

    def load_checkpoint(self, path):
        with np.load(path, allow_pickle=False) as f:
            z = {k: f[k] for k in f.files}
        fmt = int(z["format"][0])
        if fmt not in (1, 2, 3, 4, 5):
            raise IsingMcError(-1, "unknown checkpoint format")
        has_couplings = "couplings" in z
        if not np.array_equal(z["edges"], self.edges) or not np.array_equal(z["J"], self.J) or not np.array_equal(z["biases"], self.biases):
            raise IsingMcError(-1, "checkpoint belongs to a different model")
        if has_couplings != (self.couplings is not None) or (has_couplings and not np.array_equal(z["couplings"].view(np.uint64), self.couplings.view(np.uint64))):
            raise IsingMcError(-1, "checkpoint belongs to a batch with different per-replica couplings")
        if z["state"].shape != (self.nreplicas, self.nvars) or int(z["seed"][0]) != self.seed or int(z["replica_offset"][0]) != self.replica_offset:
            raise IsingMcError(-1, "checkpoint belongs to a different batch (replicas, seed or replica offset)")
        self.enable_edge_importance_sampling(bool(z["importance"][0]))
        self.set_state(z["state"])
        self.set_epoch(z["epoch"])
        self._counter_base = z["counters"].astype(np.uint64) - (self.counters() - self._counter_base)
        self._restore_attachments(z)

    def edge_list(self, r=None):
        """The edges as they were given: [((a, b), J), ...]; with `r`, the edges of replica r's realisation (its row of `couplings`)."""
        if r is None or self.couplings is None:
            return list(self._edge_list)
        return [(ab, float(j)) for (ab, _), j in zip(self._edge_list, self.couplings[int(r)])]


def new_qmc_from_graph(graph, transverse, longitudinal, cutoff, seed, **kw):
    """qmc_ising.rs:67-75"""
    return QmcIsingGraph.new_from_graph(graph, transverse, longitudinal, cutoff, seed, **kw)
