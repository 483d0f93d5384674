"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/isingmc_hip.h declares, and fails loudly (no CPU fallback) when no HIP device exists."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "isingmc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(isingmc_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    import isingmontecarlo_amd as im
    lib = im.load_library()
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"libisingmc_hip.so does not export {n}"
        assert n in im.SYMBOLS, f"python binding misses {n}"
    assert set(im.SYMBOLS) == set(names)


def test_config_struct_layout_matches_header():
    import isingmontecarlo_amd as im
    # 4 u32, 2 pointers, 2 doubles, 2 u32, u64, u32, i32, pointer, 5 u32 (+4 padding), pointer, u32 (+4), double, 2 pointers -> 144 bytes on LP64
    assert C.sizeof(im._Config) == 144 and C.sizeof(im._Interaction) == 24 and im._Interaction.mat.offset == 16
    assert im._Config.transverse_r.offset == 128 and im._Config.longitudinal_r.offset == 136
    assert im._Config.seed.offset == 56 and im._Config.init_state.offset == 72


def test_no_device_is_a_loud_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import isingmontecarlo_amd as im
    with pytest.raises(im.IsingMcError) as ei:
        im.QmcIsingGraph([((0, 1), 1.0)], 1.0, 0.0, 4, 1)
    assert ei.value.code == -2 and "no CPU fallback" in str(ei.value)


def test_create_rejects_bad_arguments():
    import isingmontecarlo_amd as im
    lib = im.load_library()
    h = C.c_void_p()
    cfg = im._Config(struct_size=4)  # wrong size
    assert lib.isingmc_create(C.byref(cfg), C.byref(h)) == -1
    assert b"struct_size" in lib.isingmc_last_error(None)
    ed = np.array([0, 5], dtype=np.uint32); js = np.array([1.0])
    cfg = im._Config(struct_size=C.sizeof(im._Config), nreplicas=1, nvars=2, nedges=1,
                     edges=ed.ctypes.data_as(C.POINTER(C.c_uint32)), J=js.ctypes.data_as(C.POINTER(C.c_double)),
                     transverse=1.0, capacity=8, cutoff0=4, device=-1)
    assert lib.isingmc_create(C.byref(cfg), C.byref(h)) == -1  # edge endpoint out of range
    cfg.nvars = 6; cfg.cutoff0 = 9
    assert lib.isingmc_create(C.byref(cfg), C.byref(h)) == -1  # cutoff0 > capacity


def test_create_rejects_bad_generic_interactions():
    """Argument checks of the generic-interaction path run before any device is touched."""
    import isingmontecarlo_amd as im
    with pytest.raises(im.IsingMcError) as ei:  # negative weight (Interaction::new, qmc_runner.rs:511-513)
        im.Qmc.from_interactions(2, [(np.array([1.0, -0.5, 0, 1.0]), (0,))], 4, 1)
    assert ei.value.code == -1 and ">= 0" in str(ei.value)
    with pytest.raises(im.IsingMcError) as ei:  # variable outside the model
        im.Qmc.from_interactions(2, [(np.ones(16), (0, 2))], 4, 1)
    assert ei.value.code == -1
    with pytest.raises(im.IsingMcError) as ei:  # the same variable twice
        im.Qmc.from_interactions(2, [(np.ones(16), (1, 1))], 4, 1)
    assert ei.value.code == -1
    # wrong matrix size for the number of variables (two variables take 16 entries, or 4 for a diagonal-only matrix)
    with pytest.raises(im.IsingMcError) as ei:
        im.Qmc.from_interactions(2, [(np.ones(8), (0, 1))], 4, 1)
    assert ei.value.code == -1
    m, off = im.Qmc.interaction_and_offset([3.0, 1.0, 1.0, 2.0])  # Interaction::new_offset: diagonal minimum removed
    assert off == 2.0 and np.allclose(m, [1.0, 1.0, 1.0, 0.0])


def test_create_argument_checks_that_need_no_device():
    """capacity == 0 (would divide by zero in the chunk grid) and interactions on more than two variables."""
    import isingmontecarlo_amd as im
    lib = im.load_library()
    h = C.c_void_p()
    ed = np.array([0, 1], dtype=np.uint32); js = np.array([1.0])
    cfg = im._Config(struct_size=C.sizeof(im._Config), nreplicas=1, nvars=2, nedges=1,
                     edges=ed.ctypes.data_as(C.POINTER(C.c_uint32)), J=js.ctypes.data_as(C.POINTER(C.c_double)),
                     transverse=1.0, capacity=0, cutoff0=0, device=-1)
    assert lib.isingmc_create(C.byref(cfg), C.byref(h)) == -1 and b"capacity" in lib.isingmc_last_error(None)
    mat = np.ones(64)
    it = im._Interaction(nvars=3, mat=mat.ctypes.data_as(C.POINTER(C.c_double)))
    cfg = im._Config(struct_size=C.sizeof(im._Config), nreplicas=1, nvars=3, capacity=8, cutoff0=4, device=-1,
                     interactions=C.cast(C.pointer(it), C.c_void_p), ninteractions=1)
    assert lib.isingmc_create(C.byref(cfg), C.byref(h)) == -5  # ENOTIMPL, qmc_runner.rs:415-680 allows any k
    with pytest.raises(im.IsingMcError) as ei:
        im.Qmc.from_interactions(3, [(np.ones(64), (0, 1, 2))], 4, 1)
    assert ei.value.code == -5
    assert lib.isingmc_clear_errors(None) == -1 and lib.isingmc_set_accumulators(None, None) == -1


def test_into_qmc_moves_the_handle_without_a_device():
    """Advisor finding r1: into_qmc used to share one __dict__ and null the handle of BOTH objects."""
    import isingmontecarlo_amd as im
    g = im.QmcIsingGraph.__new__(im.QmcIsingGraph)
    g._lib, g._h, g._flags, g.nreplicas = None, 12345, im.FLAG_HEATBATH, 1
    q = g.into_qmc(do_loop_updates=True)
    assert q._h == 12345 and g._h is None and q._flags == (im.FLAG_HEATBATH | im.FLAG_LOOP)
    q._h = None  # nothing real to destroy


def test_null_handle_calls_do_not_crash():
    import isingmontecarlo_amd as im
    lib = im.load_library()
    assert lib.isingmc_timesteps(None, 1, None, 1, 0) == -1
    assert lib.isingmc_get_n(None, None) == -1
    assert lib.isingmc_num_bonds(None) == 0
    # the tempering entry points of round 3 (device-side decisions, sweeps at the labels' temperatures)
    import ctypes as C
    on = C.c_int(7)
    assert lib.isingmc_pt_timesteps(None, 1, 1, 0) == -1
    assert lib.isingmc_pt_set_device_decisions(None, 1) == -1
    assert lib.isingmc_pt_get_device_decisions(None, C.byref(on)) == -1 and on.value == 7
    assert lib.isingmc_pt_step(None, None) == -1
    lib.isingmc_destroy(None)


def test_op_word_helpers_round_trip():
    import isingmontecarlo_amd as im
    for bond in (0, 1, 4095, (1 << 28) - 3):
        for i in range(4):
            for o in range(4):
                w = im.op_make(bond, i, o)
                assert w != 0 and im.op_fields(w) == (bond, i, o)
    assert im.op_fields(0) is None


def test_lattice_builders_match_reference_ordering():
    import _lattices as lat
    e = lat.two_d_periodic(4)
    # benches/end_to_end.rs:12-30: 16 right bonds (J=-1) then 16 down bonds (+1 on even columns)
    assert len(e) == 32 and all(j == -1.0 for _, j in e[:16])
    assert e[0][0] == (0, 1) and e[16][0] == (0, 4) and e[16][1] == 1.0
    (a, b), j = e[16 + 4]  # i=1, j=0 -> odd column
    assert (a, b) == (1, 5) and j == -1.0
    assert lat.one_d_periodic(16)[-1] == ((15, 0), 1.0)


def test_rectangular_star_and_complete_builders():
    import _lattices as lat
    fs = [None, lambda i, j, d: -1.0, lambda i, j, d: 0.5 + 0.25 * ((3 * i + 5 * j + d) % 7)]
    for l in (3, 4, 5, 8):
        for f in fs:
            assert lat.rect_periodic(l, l, f) == lat.two_d_periodic(l, f)
    e = lat.rect_periodic(3, 5)
    assert len(e) == 30 and max(max(ab) for ab, _ in e) == 14 and len({ab for ab, _ in e}) == 30
    assert e[0][0] == (0, 1) and e[2 * 5][0] == (2, 0) and e[15][0] == (0, 3) and e[15 + 4][0] == (12, 0)  # wraps: i = 2 -> 0, j = 4 -> 0
    deg = np.bincount(np.array([ab for ab, _ in e]).ravel(), minlength=15)
    assert (deg == 4).all()
    assert lat.star(5, -2.0) == [((0, 1), -2.0), ((0, 2), -2.0), ((0, 3), -2.0), ((0, 4), -2.0)]
    k = lat.complete(12, 1.0)
    assert len(k) == 66 and k[0][0] == (0, 1) and k[-1][0] == (10, 11) and len({ab for ab, _ in k}) == 66


def test_create_rejects_self_loops_before_any_device():
    """An edge (a, a) is sz_a sz_a = 1: a constant the reference never checks for and whose two-variable op would name one variable
    twice (the op word carries two in / out bits for it).  isingmc_create refuses it, before it looks for a device."""
    import isingmontecarlo_amd as im
    lib = im.load_library()
    h = C.c_void_p()
    ed = np.array([0, 1, 2, 2, 1, 2], dtype=np.uint32); js = np.array([1.0, 1.0, -1.0])
    cfg = im._Config(struct_size=C.sizeof(im._Config), nreplicas=1, nvars=3, nedges=3,
                     edges=ed.ctypes.data_as(C.POINTER(C.c_uint32)), J=js.ctypes.data_as(C.POINTER(C.c_double)),
                     transverse=1.0, capacity=8, cutoff0=4, device=-1)
    assert lib.isingmc_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    assert b"self-loop" in lib.isingmc_last_error(None)
    with pytest.raises(im.IsingMcError) as ei:
        im.QmcIsingGraph([((0, 1), 1.0), ((1, 1), 1.0)], 1.0, 0.0, 4, 1)
    assert ei.value.code == -1 and "self-loop" in str(ei.value)


def test_fft_autocorrelation_matches_direct_sum():
    """fft_autocorrelation (autocorrelations.rs:99-133) against the defining circular sum."""
    from isingmontecarlo_amd.autocorrelations import fft_autocorrelation
    rng = np.random.default_rng(3)
    x = rng.normal(size=(37, 5)) + np.linspace(0, 2, 37)[:, None]
    got = fft_autocorrelation(x)
    y = x - x.mean(axis=0)
    y = y / np.sqrt((y * y).sum(axis=0))
    want = np.array([sum((y[:, i] * np.roll(y[:, i], -t)).sum() for i in range(5)) / 5 for t in range(37)])
    assert np.allclose(got, want, atol=1e-12) and abs(got[0] - 1.0) < 1e-12


def test_header_is_plain_c_and_matches_the_python_mirror(tmp_path):
    """include/isingmc_hip.h is the drop-in boundary: it must compile as C99 on its own and agree with the ctypes mirror."""
    import os, subprocess
    import isingmontecarlo_amd as im
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "abi.c"
    src.write_text('#include "isingmc_hip.h"\n#include <stdio.h>\nint main(void){ printf("%zu %zu\\n", sizeof(isingmc_config), sizeof(isingmc_interaction)); return 0; }\n')
    exe = str(tmp_path / "abi")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", exe])
    a, b = (int(x) for x in subprocess.check_output([exe], text=True).split())
    assert a == C.sizeof(im._Config) and b == C.sizeof(im._Interaction)


def test_serde_dict_follows_the_reference_struct_definitions():
    """The dict of serde_format.to_serde walked against a schema written by hand from the Rust struct definitions (field names,
    nesting, Option / tuple / enum shapes as serde_json writes them): SerializeQmcGraph qmc_ising.rs:1010-1028, FastOpsTemplate
    fast_ops.rs:35-49, FastOpNodeTemplate :181-190, BasicOp op_container.rs:224-237, OpType :165-173, PRel directed_loop.rs:12-17,
    DefaultFastOpAllocator fast_op_alloc.rs:29-39, Allocator util/allocator.rs:31-38 (instances as its length).  No GPU: the
    graph is a stand-in that hands out a hand-built op-string."""
    import isingmontecarlo_amd as im
    from isingmontecarlo_amd.serde_format import to_serde

    class Stub:  # what to_serde asks of a graph
        nvars = 3
        edges = np.array([[0, 1], [1, 2]], dtype=np.uint32)
        J = np.array([1.0, -0.5])
        transverse, longitudinal = 0.7, 0.2
        _flags = 8  # run_rvb
        transverse_r = longitudinal_r = None
        def export_ops(self, r):  # two-site diagonal, empty, transverse off-diagonal on var 1, longitudinal diagonal on var 2
            return np.array([im.op_make(0, 0b10, 0b10), 0, im.op_make(2 + 1, 0, 1), im.op_make(2 + 3 + 2, 1, 1)], dtype=np.uint32)
        def state_ref(self):
            return np.array([[0, 1, 1]], dtype=np.uint8)
        def get_offsets(self):
            return np.array([4.2])

    d = to_serde(Stub(), 0, total_rvb_successes=5, rvb_clusters_counted=9)
    usize = lambda x: isinstance(x, int) and not isinstance(x, bool) and x >= 0
    f64 = lambda x: isinstance(x, float)
    boolean = lambda x: isinstance(x, bool)
    opt = lambda f: (lambda x: x is None or f(x))
    vec = lambda f: (lambda x: isinstance(x, list) and all(f(y) for y in x))
    tup = lambda *fs: (lambda x: isinstance(x, list) and len(x) == len(fs) and all(f(y) for f, y in zip(fs, x)))
    def struct(**fields):
        def check(x):
            assert isinstance(x, dict) and list(x.keys()) == list(fields.keys()), (list(x.keys()) if isinstance(x, dict) else x, list(fields.keys()))
            for k, f in fields.items():
                assert f(x[k]), (k, x[k])
            return True
        return check
    prel = struct(p=usize, relv=usize)
    optype = lambda x: isinstance(x, dict) and len(x) == 1 and (("Diagonal" in x and vec(boolean)(x["Diagonal"])) or
                                                                ("Offdiagonal" in x and tup(vec(boolean), vec(boolean))(x["Offdiagonal"])))
    basic_op = struct(vars=vec(usize), bond=usize, in_out=optype, constant=boolean)
    node = struct(op=basic_op, previous_p=opt(usize), next_p=opt(usize), previous_for_vars=vec(opt(prel)), next_for_vars=vec(opt(prel)))
    allocator = struct(instances=usize, gen_more=boolean)
    alloc = struct(usize_alloc=allocator, bool_alloc=allocator, opside_alloc=allocator, leg_alloc=allocator, option_usize_alloc=allocator,
                   f64_alloc=allocator, bond_container_alloc=allocator, bond_container_varpos_alloc=allocator, binary_heap_alloc=allocator)
    manager = struct(ops=vec(opt(node)), n=usize, p_ends=opt(tup(usize, usize)), var_ends=vec(opt(tup(prel, prel))),
                     bond_counters=vec(usize), alloc=alloc)
    graph = struct(edges=vec(tup(vec(usize), f64)), transverse=f64, longitudinal=f64, state=opt(vec(boolean)), cutoff=usize,
                   op_manager=opt(manager), total_energy_offset=f64, nvars=usize, run_rvb_steps=boolean,
                   classical_bonds=opt(vec(vec(usize))), total_rvb_successes=usize, rvb_clusters_counted=usize,
                   bond_weights=opt(struct(max_weight_and_cumulative=vec(tup(usize, f64, f64)))))
    assert graph(json.loads(json.dumps(d)))
    m = d["op_manager"]
    assert m["n"] == 3 and m["p_ends"] == [0, 3] and m["ops"][1] is None and m["bond_counters"] == [1, 0, 0, 1, 0, 0, 0, 1]
    assert m["ops"][0]["op"] == {"vars": [0, 1], "bond": 0, "in_out": {"Diagonal": [False, True]}, "constant": False}
    assert m["ops"][2]["op"] == {"vars": [1], "bond": 3, "in_out": {"Offdiagonal": [[False], [True]]}, "constant": True}
    assert m["ops"][2]["previous_for_vars"] == [{"p": 0, "relv": 1}] and m["ops"][0]["next_for_vars"] == [None, {"p": 2, "relv": 0}]
    assert m["var_ends"] == [[{"p": 0, "relv": 0}, {"p": 0, "relv": 0}], [{"p": 0, "relv": 1}, {"p": 2, "relv": 0}], [{"p": 3, "relv": 0}, {"p": 3, "relv": 0}]]
    assert m["alloc"]["usize_alloc"] == {"instances": 10, "gen_more": False} and m["alloc"]["binary_heap_alloc"]["instances"] == 1
    assert d["run_rvb_steps"] and d["classical_bonds"] == [[0], [0, 1], [1]] and d["total_rvb_successes"] == 5 and d["rvb_clusters_counted"] == 9


def test_row_stride_covers_every_whole_tile_access():
    """Bounds audit of the op-string rows (isingmc_plan_geometry, the function isingmc_create itself uses): for every launch geometry
    a batch can run with, the largest slot index any kernel forms stays inside the row.
      * diagonal / cached-apply passes stream whole tiles of W * 64 * K slots up to the cutoff (<= capacity);
      * a cluster-scan wave owns ceil(used / W) chunks and loads / stores wave-tiles of 64 * K slots from its range start — also
        when its range is empty (range start = end of the chunk-rounded string): that prefetch needs the + 256;
      * the dedicated cluster kernel keeps one 16-bit id per slot, two rows per dword, in the first half of a scratch row.
    (Round 2 saw a GPU memory fault in an uncommitted experiment on the 16-wave HBM-table path; the shipped index arithmetic
    is checked here for all geometries instead of trusting one passing run.)"""
    import isingmontecarlo_amd as im
    lib = im.load_library()
    out = (C.c_uint32 * 4)()
    rng = np.random.default_rng(5)
    caps = [1, 2, 63, 64, 97, 255, 256, 257, 1023, 1024, 4095, 4096, 4097, 8191, 8192, 32768 + 1, 1 << 18, (1 << 18) + 777, 1 << 20, 3_000_001] + [int(x) for x in rng.integers(1, 1 << 22, 60)]
    caps += [24 * n + 256 for n in (1, 33, 4071, 4072, 4095, 4096, 4097, 6144, 6175, 8480, 8481, 11041, 11042, 12288, 12289)]  # tests/test_gpu_shape_edges.py
    for cap in caps:
        for W, Wmax in [(1, 1), (4, 4), (4, 8), (4, 16), (6, 6), (6, 16), (8, 8), (8, 16), (16, 16), (1, 16)]:
            for K in (1, 2, 4):
                assert lib.isingmc_plan_geometry(cap, W, K, Wmax, out) == 0
                CH, nchunks, stride, tile = (int(x) for x in out)
                assert CH % 256 == 0 and nchunks <= 128 and CH * nchunks >= cap
                for Wk in {W, Wmax, 8 if Wmax >= 8 and W < 8 else W}:  # (8 waves: the HBM union-find geometry of run())
                    if Wmax % Wk and Wk != W:
                        continue
                    ts = Wk * 64 * K
                    assert stride % ts == 0, (cap, W, Wmax, K, Wk)
                    # whole-tile streaming up to any cutoff M <= cap: last slot touched = roundup(M, ts) - 1
                    assert (cap + ts - 1) // ts * ts <= stride
                    # cluster scan: wave ranges in chunks, wave-tiles of 64 K slots from the range start, prefetch even when empty
                    for M in {cap, max(1, cap // 2), max(1, cap - 1)}:
                        used = (M + CH - 1) // CH
                        q = (used + Wk - 1) // Wk
                        for w in range(Wk):
                            c0 = min(w * q, used); c1 = min(c0 + q, used)
                            pbeg, pend = c0 * CH, min(c1 * CH, M)
                            last = pbeg + 64 * K - 1  # the unconditional prefetch at the range start
                            if pend > pbeg:
                                last = max(last, pbeg + ((pend - pbeg + 64 * K - 1) // (64 * K)) * 64 * K - 1)
                            assert last < stride, (cap, W, Wmax, K, Wk, M, w, last, stride)
                            assert (last >> 1) + 64 < stride  # 16-bit ids of the dedicated cluster kernel (K >= 2): dword (p0 >> 1) + 32 j + lane


def test_dedicated_cluster_kernel_lds_layout_and_gate():
    """Bounds audit of the dedicated cluster kernel's LDS (csrc/sse_cluster.hip.h, through isingmc_plan_cluster_lds: ClLds::carve,
    the launch's words, the kernel's gate cl_ids_fit and its root-list capacity).  After the joins the kernel reuses its per-wave
    tables o_ent (16 (N + 1) words) for S flip bits (S = 16 N + cuts) and, behind them, a u16 list of roots.  Wherever the gate
    accepts a replica:
      * the flip bits end at or before o_frozen (= o_parent without a longitudinal field), the tables that follow o_ent;
      * the root list fits behind the bits (no wrapped capacity);
      * the 16-bit parent table holds S + 1 entries (id S is the null id of empty slots) inside the launch's LDS.
    The gate must accept every replica that fits (it costs nothing at the headline size) and reject the few-variable, long-string
    models whose flip-bit words (S + 31) / 32 the oracle measured beyond 16 (N + 1)."""
    import isingmontecarlo_amd as im
    lib = im.load_library()
    out = (C.c_uint32 * 13)()

    def plan(N, has_long, ufcap, S, Nb=None):
        assert lib.isingmc_plan_cluster_lds(N, (N + 31) // 32, 4 * N if Nb is None else Nb, has_long, ufcap, S, out) == 0
        return [int(x) for x in out]

    rng = np.random.default_rng(11)
    Ns = sorted(set(range(1, 257)) | set(range(257, 4096, 37)) | {511, 512, 1023, 1024, 1025, 2047, 2048, 4071, 4072, 4094, 4095})
    accepted = rejected_by_bits = 0
    for N in Ns:
        tab = 16 * (N + 1)
        bound = 32 * tab  # largest S whose flip bits fill the tables exactly
        edges = [16 * N, 16 * N + 1, bound - 32, bound - 1, bound, bound + 1, 65534, 65535, 65536]
        ufcaps = {65535, min(65535, 16 * N + 384), min(65535, bound + 1), min(65535, bound), min(65535, 16 * N + 3000 + 3000 // 16 + 384)}
        for has_long in (0, 1):
            for ufcap in sorted(ufcaps):
                Ss = set(edges) | {ufcap - 1, ufcap, ufcap + 1} | {int(x) for x in rng.integers(16 * N, 70000, 4)}
                for S in sorted(Ss):
                    (o_tab, o_state, o_touch, o_misc, o_chn, o_chtr, o_ent, o_frozen, o_froot, o_parent,
                     words, ok, list_cap) = plan(N, has_long, ufcap, S)
                    fits = S < ufcap and S < 65535 and (S + 31) // 32 <= tab
                    # the carve itself: regions in order, the per-wave tables directly in front of the frozen / parent tables
                    assert o_tab == 0 and o_state == 4 * N + 1 and o_ent + tab == o_frozen <= o_froot <= o_parent
                    if has_long:
                        assert o_froot - o_frozen == o_parent - o_froot == (ufcap + 31) // 32
                    assert o_parent + (ufcap + 1) // 2 <= words
                    if ok:
                        accepted += 1
                        bits = (S + 31) // 32
                        assert o_ent + bits <= o_frozen and o_ent + bits <= o_parent, (N, S, bits, tab)
                        assert 0 <= list_cap <= 2 * tab and 2 * (o_ent + bits) + list_cap <= 2 * (o_ent + tab), (N, S, list_cap)
                        assert 2 * o_parent + S + 1 <= 2 * words and o_parent + S // 2 < words  # parent[0..S] (the init writes words 0..S/2)
                    else:
                        rejected_by_bits += S < ufcap and S < 65535
                    assert bool(ok) == fits, (N, has_long, ufcap, S, ok)  # and nothing that fits is refused
    assert accepted > 5000 and rejected_by_bits > 500
    # the headline size never meets the flip-bit bound: every S the 16-bit ids allow is accepted at N = 1024
    assert all(plan(1024, 0, 65535, S)[11] for S in (16 * 1024, 40000, 65534))
    # (S + 31) / 32 as the oracle measured it (60 timesteps, 4 replicas, Gamma = 1) on models that reach the bound: rejected
    for N, words_lo, words_hi in [(8, 245, 256), (4, 104, 107), (2, 96, 97), (6, 136, 140)]:
        for w in range(words_lo, words_hi + 1):
            for S in (32 * w - 31, 32 * w):
                assert plan(N, 0, 65535, S)[11] == 0 and plan(N, 1, 65535, S)[11] == 0, (N, S)
    for w in range(85, 92):  # the control row (ring of 8 at beta = 200) stays with the kernel
        assert plan(8, 0, 65535, 32 * w)[11] == 1


def _plan_cases():
    with open(os.path.join(ROOT, "tests", "golden", "batch_plans.json")) as f:
        return json.load(f)


def _first_lds(plan, nvars, cap, total_words, uf_ids_limit, has_long):
    """lds_words / lds_ufcap of a fresh batch as plan_lds sizes them (no transverse op seen yet), from the recorded pair of the
    parent, which laid out every model as one without a longitudinal field: its words = F + (ids + 1) / 2 (16-bit parents), so F,
    the launch's LDS without a union-find, follows; a field adds two bit arrays of (ids + 31) / 32 words (Lds::carve).  ids = W N +
    384 (or the test limit; 0 with the tables in HBM), at most 65535 and W N + cap, less in steps of 64 while the launch exceeds LDS."""
    import _plan_cases as pc
    p = dict(zip(pc.SLOTS, plan))
    F = p["lds_words"] - (p["lds_ufcap"] + 1) // 2
    words = lambda i: F + (2 * ((i + 31) // 32) if has_long else 0) + (i + 1) // 2
    ids = uf_ids_limit or p["W"] * nvars + 384
    if p["mode"] in (pc.MODE_GLOBAL_TABLES, pc.MODE_PM_GLOBAL_TABLES):
        ids = 0
    ids = min(ids, 65535, p["W"] * nvars + cap)
    while ids > 0 and words(ids) > total_words:
        ids -= min(ids, 64)
    return words(ids), ids


def test_plan_batch_gives_the_recorded_plans():
    """isingmc_plan_batch (check_config, build_tables and the plan_batch that isingmc_create itself calls) against the plans that
    the commit before create was taken apart printed on an MI355X for the same configs (tests/golden/batch_plans.json, recorded
    with profiles/r07_parent_plan_print.patch): every rung of the size ladder, every cfg flag, the explicit geometries, the
    capacity-2^20 lattice, the 32^3 +-J pair, generic interactions, per-replica fields.  Every slot is equal, but for the first
    lds_words / lds_ufcap of models with a longitudinal field ("field" in the file): that commit sized those before it had noted
    the field; they are held to _first_lds.  (On the cases without a field _first_lds must give back the recorded pair: that checks its
    choice of the ids, the clamps and the 64-step loop, before it is applied here; the word count without a union-find it takes from
    the record itself.)"""
    import isingmontecarlo_amd as im
    import _plan_cases as pc
    gold = _plan_cases()
    assert gold["slots"] == pc.SLOTS and len(gold["cases"]) >= 70
    i_words, i_ufcap = pc.SLOTS.index("lds_words"), pc.SLOTS.index("lds_ufcap")
    fields = 0
    for case in gold["cases"]:
        cfg, keep = pc.config_of(im, case)
        rc, got = pc.plan_batch(im, cfg, gold["lds_bytes"])
        assert rc == 0, (case["name"], rc, im.load_library().isingmc_last_error(None))
        want = list(case["plan"])
        assert len(want) == 32 and _first_lds(want, cfg.nvars, cfg.capacity, gold["lds_bytes"] // 4, cfg.lds_uf_ids_limit, False) == (want[i_words], want[i_ufcap]), case["name"]
        if case.get("field"):
            fields += 1
            want[i_words], want[i_ufcap] = _first_lds(want, cfg.nvars, cfg.capacity, gold["lds_bytes"] // 4, cfg.lds_uf_ids_limit, True)
        assert got == want, (case["name"], [(s, g, w) for s, g, w in zip(pc.SLOTS, got, want) if g != w])
    assert fields >= 8


def test_plan_batch_invariants():
    """What every plan must satisfy, whatever the recorded values say."""
    import isingmontecarlo_amd as im
    import _plan_cases as pc
    lib = im.load_library()
    gold = _plan_cases()
    total = gold["lds_bytes"] // 4
    geo = (C.c_uint32 * 4)()
    seen = {k: set() for k in ("fast_diag", "defer", "lean_cluster", "rvb_split", "rvb_global", "mode")}
    for case in gold["cases"]:
        cfg, keep = pc.config_of(im, case)
        rc, out = pc.plan_batch(im, cfg, gold["lds_bytes"])
        assert rc == 0 and out[len(pc.SLOTS):] == [0] * (32 - len(pc.SLOTS)), case["name"]
        p = dict(zip(pc.SLOTS, out))
        for k in ("lds_words_pm_diag", "lds_words_diag", "lds_words_rvb", "lds_words"):
            assert p[k] <= total, (case["name"], k, p[k])
        if p["fast_diag"]:
            assert p["lds_words_fast"] <= total, case["name"]
        assert lib.isingmc_plan_geometry(cfg.capacity, p["W"], p["K"], p["Wmax"], geo) == 0
        assert [p["CH"], p["nchunks"], p["stride"]] == [int(x) for x in geo[:3]], case["name"]
        lds_edges = p["mode"] == pc.MODE_LDS_EDGES
        hbm = p["mode"] in (pc.MODE_GLOBAL_TABLES, pc.MODE_PM_GLOBAL_TABLES)
        assert p["mode"] in (pc.MODE_GENERAL, pc.MODE_LDS_EDGES, pc.MODE_GLOBAL_TABLES, pc.MODE_PM_GLOBAL_TABLES)
        assert bool(p["tbl_stride"]) == hbm and p["W_off"] <= p["Wmax"] >= p["W"], case["name"]
        if p["fast_diag"]:
            assert lds_edges and p["W"] == 4, case["name"]
        if p["defer"]:
            assert p["lean_cluster"] and p["fast_diag"], case["name"]
        if hbm:
            assert p["W_off"] == p["W"] and not lds_edges and p["lds_ufcap"] == 0, case["name"]
        if p["mode"] == pc.MODE_PM_GLOBAL_TABLES:
            assert hbm and p["W"] == 4 and p["K"] == 4 and p["pm_words"] == (cfg.nedges + 31) // 32, case["name"]
        else:
            assert p["pm_words"] == 0 and p["lds_words_pm_diag"] == 0, case["name"]
        if p["rvb_split"]:
            assert not p["rvb_global"] and not (cfg.flags & im.CFG_FUSED_LAUNCH) and not cfg.interactions and not hbm, case["name"]
        for k in seen:
            seen[k].add(p[k])
    assert all(len(v) >= 2 for v in seen.values()) and len(seen["mode"]) == 4, seen


# (what is wrong, changes to the case, changes to the model, code, words of the message)
_CONFIG_ERRORS_BEHIND_THE_PROBE = [
    ("fields without the flag", dict(without_per_replica_flag=True), dict(transverse_r=[1.0, 1.0, 1.0]), -1, b"per-replica fields need ISINGMC_CFG_PER_REPLICA_J (per-replica bond tables)"),
    ("mixed fields", {}, dict(longitudinal_r=[0.2, 0.0, 0.2]), -1, b"longitudinal fields must be all zero or all non-zero within a batch"),
    ("field not finite", {}, dict(transverse_r=[1.0, float("inf"), 1.0]), -1, b"fields must be finite, transverse field >= 0"),
    ("waves_per_replica 5", dict(waves_per_replica=5), {}, -1, b"waves_per_replica must be 1, 4, 6, 8 or 16"),
    ("slots_per_lane 3", dict(slots_per_lane=3), {}, -1, b"slots_per_lane must be 1, 2 or 4"),
    ("waves_offdiag 5", dict(waves_offdiag=5), {}, -1, b"waves_offdiag must be 0, 1, 4, 6, 8 or 16"),
    ("global tables next to the LDS edge table", dict(flags=8), {}, -1, b"ISINGMC_CFG_GLOBAL_TABLES needs the general bond table: combine it with ISINGMC_CFG_NO_LDS_TABLES"),
    ("bit arrays beyond LDS", dict(lds_bytes=1024), {}, -5, b"model too large: the spin-state bit arrays alone exceed LDS"),
    ("row stride", dict(capacity=0xFFFFFFFF, cutoff=16), {}, -1, b"capacity too large for the row stride"),
]


def test_config_errors_behind_the_device_probe_are_reachable_without_a_device():
    """The checks isingmc_create makes once it has a device, through isingmc_plan_batch: code and message.  Where there is no
    device, create still answers ENODEVICE for the same configs (those checks stay behind the probe)."""
    import torch
    import isingmontecarlo_amd as im
    import _plan_cases as pc
    lib = im.load_library()
    base = dict(model=["ferro", 4], nreplicas=3, capacity=4096)
    model = pc.model_of(base["model"])
    cfg, keep = pc.config_of(im, base)
    assert pc.plan_batch(im, cfg, 160 * 1024)[0] == 0
    for what, case_changes, model_changes, code, message in _CONFIG_ERRORS_BEHIND_THE_PROBE:
        case = dict(base, **case_changes)
        cfg, keep = pc.config_of(im, case, dict(model, **model_changes))
        rc, out = pc.plan_batch(im, cfg, case.get("lds_bytes", 160 * 1024))
        assert rc == code and lib.isingmc_last_error(None) == message, (what, rc, lib.isingmc_last_error(None))
        if not torch.cuda.is_available() and "lds_bytes" not in case:
            h = C.c_void_p()
            assert lib.isingmc_create(C.byref(cfg), C.byref(h)) == -2 and not h.value, what
            assert b"no HIP device" in lib.isingmc_last_error(None), what
    # a config error in front of the probe keeps its place there
    cfg, keep = pc.config_of(im, dict(base, cutoff=5000))
    assert pc.plan_batch(im, cfg, 160 * 1024)[0] == -1 and lib.isingmc_last_error(None) == b"cutoff0 exceeds capacity"
    assert lib.isingmc_plan_batch(None, 160 * 1024, None) == -1
