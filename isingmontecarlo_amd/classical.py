"""Classical Ising Monte Carlo on the device: `GraphState` (qmc::classical::GraphState, src/classical/graph.rs) for a batch of R
replicas of one graph, over the isingmc_classical_* entry points of include/isingmc_hip.h.  All moves run in gfx950 kernels
(csrc/sse_classical.hip.h); there is no CPU fallback.  `host_steps` and `plan` are the device-free test entries of the C ABI."""
import ctypes as C

import numpy as np

from . import ALL, IsingMcError, QmcIsingGraph, _ClassicalConfig, _ptr, load_library  # (imported at the end of the package's __init__)

__all__ = ["GraphState", "new_qmc_from_graph", "host_steps", "plan", "CFG_EDGE_IMPORTANCE", "CFG_GLOBAL_TABLES", "CFG_SERIAL_MOVES",
           "KINDS_ALL", "KINDS_BASIC", "KINDS_SPIN", "KINDS_EDGE", "KINDS_WORM", "KINDS_WORM_NO_DOUBLES", "COUNTERS"]

CFG_EDGE_IMPORTANCE, CFG_GLOBAL_TABLES, CFG_SERIAL_MOVES = 1, 2, 4
KINDS_ALL, KINDS_BASIC, KINDS_SPIN, KINDS_EDGE, KINDS_WORM, KINDS_WORM_NO_DOUBLES = range(6)
NONE = 0xFFFFFFFF  # the reference's None for the move counts
COUNTERS = ("spin_attempted", "spin_accepted", "edge_attempted", "edge_accepted", "worm_attempted", "worm_kept", "worm_failures", "worm_path_entries")


def _model(edges, biases):
    ed = np.ascontiguousarray(np.array([[a, b] for (a, b), _ in edges], dtype=np.uint32).reshape(-1, 2))
    js = np.ascontiguousarray(np.array([j for _, j in edges], dtype=np.float64))
    hs = np.ascontiguousarray(np.asarray(biases, dtype=np.float64))
    return ed, js, hs


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
    return dict(waves=out[0], in_lds=out[1], lds_words=out[2], wave_words=out[3], tables=out[4], compact_couplings=bool(out[5]), packed_edges=bool(out[6]))


def plan(edges, biases, lds_bytes=160 * 1024, flags=0):
    """isingmc_classical_plan: the launch isingmc_classical_create would choose, without a device."""
    lib = load_library()
    ed, js, hs = _model(edges, biases)
    out = (C.c_uint32 * 8)()
    rc = lib.isingmc_classical_plan(C.byref(_config(ed, js, hs, 0, 1, flags=flags)), int(lds_bytes), out)
    if rc:
        raise IsingMcError(rc, lib.isingmc_classical_last_error(None).decode())
    return _plan_dict(out)


def host_steps(edges, biases, seed, states, epochs, t, beta, nspinupdates=None, nedgeupdates=None, nwormupdates=None, only_basic_moves=None,
               kinds=None, replica_offset=0, flags=0):
    """isingmc_classical_host_steps: t time steps of the sequential rule on the CPU.  Returns (states, epochs, counters)."""
    lib = load_library()
    ed, js, hs = _model(edges, biases)
    st = np.ascontiguousarray(np.array(states, dtype=np.uint8).reshape(-1, len(hs)))
    ep = np.ascontiguousarray(np.broadcast_to(np.asarray(epochs, dtype=np.uint64), (len(st),)).copy())
    ctr = np.zeros((len(st), 8), dtype=np.uint64)
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(beta, dtype=np.float64), (len(st),)))
    rc = lib.isingmc_classical_host_steps(C.byref(_config(ed, js, hs, seed, len(st), replica_offset, flags=flags)), int(t), _ptr(b, C.c_double),
                                          _count(nspinupdates), _count(nedgeupdates), _count(nwormupdates), _kinds(only_basic_moves, kinds),
                                          _ptr(st, C.c_uint8), _ptr(ep, C.c_uint64), _ptr(ctr, C.c_uint64))
    if rc:
        raise IsingMcError(rc, lib.isingmc_classical_last_error(None).decode())
    return st, ep, ctr


class GraphState:
    """R replicas of GraphState::new / new_with_state_and_rng (graph.rs:56-88): `edges` = [((a, b), J), ...], `biases` the
    longitudinal fields (their length is the number of variables), `seed` in place of the rng; `state` [N] or [R][N] (None: random)."""

    def __init__(self, edges, biases, seed, state=None, nreplicas=1, replica_offset=0, device=-1, cfg_flags=0):
        self._lib = load_library()
        self._h = None
        self._edge_list = [((int(a), int(b)), float(j)) for (a, b), j in edges]
        self.edges, self.J, self.biases = _model(edges, biases)
        self.nvars, self.nreplicas = len(self.biases), int(nreplicas)
        self.seed, self.replica_offset, self.device = int(seed), int(replica_offset), int(device)
        self._cfg_flags = int(cfg_flags)
        self._counter_base = np.zeros((self.nreplicas, 8), dtype=np.uint64)
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
        cfg = _config(self.edges, self.J, self.biases, self.seed, self.nreplicas, self.replica_offset, self.device, init, self._cfg_flags)
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
        state, epoch, counters = self.state_ref(), self.get_epoch(), self.counters()
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
        restored with load_checkpoint continues bit-exactly."""
        np.savez_compressed(path, format=np.array([1], dtype=np.uint32), edges=self.edges, J=self.J, biases=self.biases,
                            seed=np.array([self.seed], dtype=np.uint64), replica_offset=np.array([self.replica_offset], dtype=np.uint32),
                            importance=np.array([bool(self._cfg_flags & CFG_EDGE_IMPORTANCE)]), state=self.state_ref(), epoch=self.get_epoch(),
                            counters=self.counters())

    def load_checkpoint(self, path):
        z = np.load(path, allow_pickle=False)
        if not np.array_equal(z["edges"], self.edges) or not np.array_equal(z["J"], self.J) or not np.array_equal(z["biases"], self.biases):
            raise IsingMcError(-1, "checkpoint belongs to a different model")
        if z["state"].shape != (self.nreplicas, self.nvars) or int(z["seed"][0]) != self.seed or int(z["replica_offset"][0]) != self.replica_offset:
            raise IsingMcError(-1, "checkpoint belongs to a different batch (replicas, seed or replica offset)")
        self.enable_edge_importance_sampling(bool(z["importance"][0]))
        self.set_state(z["state"])
        self.set_epoch(z["epoch"])
        self._counter_base = z["counters"].astype(np.uint64) - (self.counters() - self._counter_base)

    def edge_list(self):
        """The edges as they were given: [((a, b), J), ...]."""
        return list(self._edge_list)


def new_qmc_from_graph(graph, transverse, longitudinal, cutoff, seed, **kw):
    """qmc_ising.rs:67-75"""
    return QmcIsingGraph.new_from_graph(graph, transverse, longitudinal, cutoff, seed, **kw)
