"""csrc/classical_host.hip — the device-free half of the classical C ABI, the sequential rule that every classical parity test compares
against — compiled by the host compiler as plain C++ into a stand-alone program under the address and undefined-behaviour sanitizers.
The link line names no HIP library and no stand-ins for one: that the link succeeds is the check that the unit calls neither the runtime
nor a launcher.  The program reads a list of calls from a file, makes them through the C entries and writes every output to a second
file (a refusal's text through cmc_last_refusal, which isingmc_classical_last_error(NULL) returns in the library); the test makes the
same calls through the built library with ctypes, and the two outputs are equal in every bit.  No device,
nothing loaded into Python under a sanitizer."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _classical_cases as cc
import _classical_icm_cases as ic
import _classical_pt_cases as pc
import _classical_reference as CR

PROGRAM = r"""
#include "../../include/isingmc_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

const char *cmc_last_refusal(); // csrc/classical_host.h: the text isingmc_classical_last_error(NULL) returns (that entry itself lives with the handle)

static FILE *g_in, *g_out;
static void get(void *p, size_t n) { if (n && std::fread(p, 1, n, g_in) != n) { std::printf("short input\n"); std::exit(2); } }
static void put(const void *p, size_t n) { if (n && std::fwrite(p, 1, n, g_out) != n) { std::printf("short output\n"); std::exit(2); } }
template <class T> static std::vector<T> arr() { // u64 count, then the elements
    uint64_t n; get(&n, 8);
    std::vector<T> v(n);
    get(v.data(), n * sizeof(T));
    return v;
}
template <class T> static T *ptr(std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
template <class T> static void put(const std::vector<T> &v) { put(v.data(), v.size() * sizeof(T)); }
static void put_rc(int rc) { // the return code and, of a refusal, its text
    const int32_t r = rc;
    put(&r, 4);
    const char *why = rc ? cmc_last_refusal() : "";
    const uint64_t n = std::strlen(why);
    put(&n, 8); put(why, n);
}

enum { RUN, RUN_OVERLAPS, RUN_ICM, STEPS, CLUSTER, ICM_PLAN };
// scalars of a call, in the order the test writes them
enum { KIND, NREPLICAS, NVARS, NEDGES, SEED, OFFSET, FLAGS, NTEMPS, NCOPIES, ROUNDS, NSTEPS, NSPIN, NEDGE, NWORM, KINDS, PT_STEP, MEASURE, T_FIRST, T_LAST,
       N_SERIES, N_ITEMS, N_HQ, N_HL, N_COUNTS, N_PAIRS, RANK, LDS_BYTES, NSCALARS };

int main(int argc, char **argv) {
    if (argc != 3 || !(g_in = std::fopen(argv[1], "rb")) || !(g_out = std::fopen(argv[2], "wb"))) return 2;
    uint64_t ncalls; get(&ncalls, 8);
    for (uint64_t call = 0; call < ncalls; ++call) {
        uint64_t s[NSCALARS]; get(s, sizeof s);
        std::vector<uint32_t> edges = arr<uint32_t>();
        std::vector<double> J = arr<double>(), biases = arr<double>(), betas = arr<double>();
        std::vector<uint8_t> states = arr<uint8_t>(), other = arr<uint8_t>();
        std::vector<uint64_t> epochs = arr<uint64_t>();
        std::vector<uint32_t> temp_of = arr<uint32_t>();
        isingmc_classical_config cfg;
        std::memset(&cfg, 0, sizeof cfg);
        cfg.struct_size = sizeof cfg; cfg.nreplicas = (uint32_t)s[NREPLICAS]; cfg.nvars = (uint32_t)s[NVARS]; cfg.nedges = (uint32_t)s[NEDGES];
        cfg.edges = ptr(edges); cfg.J = ptr(J); cfg.biases = ptr(biases); cfg.seed = s[SEED]; cfg.replica_offset = (uint32_t)s[OFFSET]; cfg.device = -1;
        cfg.flags = (uint32_t)s[FLAGS];
        const uint32_t T = (uint32_t)s[NTEMPS], K = (uint32_t)s[NCOPIES], nspin = (uint32_t)s[NSPIN], nedge = (uint32_t)s[NEDGE], nworm = (uint32_t)s[NWORM],
                       kinds = (uint32_t)s[KINDS];
        uint64_t pt_step = s[PT_STEP];
        std::vector<uint64_t> counters(8 * s[NREPLICAS]), attempts(s[N_PAIRS]), accepts(s[N_PAIRS]), hq(s[N_HQ]), hl(s[N_HL]), moves(s[N_COUNTS]), empty(s[N_COUNTS]),
            size_sum(s[N_COUNTS]);
        std::vector<double> energy(s[N_SERIES]);
        std::vector<int32_t> mag(s[N_SERIES]), q(s[N_ITEMS]), ql(s[N_ITEMS]);
        if (s[KIND] == RUN || s[KIND] == RUN_OVERLAPS || s[KIND] == RUN_ICM) {
            int rc;
            if (s[KIND] == RUN)
                rc = isingmc_classical_host_pt_run(&cfg, T, ptr(betas), s[ROUNDS], s[NSTEPS], nspin, nedge, nworm, kinds, ptr(states), ptr(epochs), ptr(temp_of), &pt_step,
                                                   ptr(counters), ptr(attempts), ptr(accepts), ptr(energy), ptr(mag));
            else if (s[KIND] == RUN_OVERLAPS)
                rc = isingmc_classical_host_pt_run_overlaps(&cfg, T, ptr(betas), K, s[ROUNDS], s[NSTEPS], nspin, nedge, nworm, kinds, ptr(states), ptr(epochs), ptr(temp_of),
                                                            &pt_step, ptr(counters), ptr(attempts), ptr(accepts), ptr(energy), ptr(mag), ptr(q), ptr(ql), ptr(hq), ptr(hl));
            else
                rc = isingmc_classical_host_pt_run_icm(&cfg, T, ptr(betas), K, s[ROUNDS], s[NSTEPS], nspin, nedge, nworm, kinds, ptr(states), ptr(epochs), ptr(temp_of),
                                                       &pt_step, ptr(counters), ptr(attempts), ptr(accepts), ptr(energy), ptr(mag), ptr(q), ptr(ql), ptr(hq), ptr(hl),
                                                       (uint32_t)s[MEASURE], (uint32_t)s[T_FIRST], (uint32_t)s[T_LAST], ptr(moves), ptr(empty), ptr(size_sum));
            put_rc(rc);
            put(states); put(epochs); put(temp_of); put(&pt_step, 8); put(counters); put(attempts); put(accepts); put(energy); put(mag); put(q); put(ql); put(hq);
            put(hl); put(moves); put(empty); put(size_sum);
        } else if (s[KIND] == STEPS) {
            put_rc(isingmc_classical_host_steps(&cfg, s[NSTEPS], ptr(betas), nspin, nedge, nworm, kinds, ptr(states), ptr(epochs), ptr(counters)));
            put(states); put(epochs); put(counters);
        } else if (s[KIND] == CLUSTER) {
            std::vector<uint8_t> mask(s[NVARS], 0xAB); // (the entry zeroes it)
            uint32_t size = 0;
            put_rc(isingmc_classical_host_icm_cluster(&cfg, ptr(states), ptr(other), (uint32_t)s[RANK], ptr(mask), &size));
            put(mask); put(&size, 4);
        } else if (s[KIND] == ICM_PLAN) {
            uint32_t out[4] = {0, 0, 0, 0};
            put_rc(isingmc_classical_icm_plan((uint32_t)s[NVARS], (uint32_t)s[LDS_BYTES], out));
            put(out, sizeof out);
        } else return 2;
    }
    if (std::fclose(g_out) != 0) return 2;
    std::printf("ok\n");
    return 0;
}
"""

RUN, RUN_OVERLAPS, RUN_ICM, STEPS, CLUSTER, ICM_PLAN = range(6)
SCALARS = ("kind", "nreplicas", "nvars", "nedges", "seed", "offset", "flags", "ntemps", "ncopies", "rounds", "nsteps", "nspin", "nedge", "nworm", "kinds", "pt_step",
           "measure", "t_first", "t_last", "n_series", "n_items", "n_hq", "n_hl", "n_counts", "n_pairs", "rank", "lds_bytes")
ARRAYS = (("edges", np.uint32), ("J", np.float64), ("biases", np.float64), ("betas", np.float64), ("states", np.uint8), ("other", np.uint8), ("epochs", np.uint64),
          ("temp_of", np.uint32))
NONE = 0xFFFFFFFF


def _cl():
    import isingmontecarlo_amd.classical as cl
    return cl


def _call(kind, edges=(((0, 1), 1.0),), biases=(0.0, 0.0), **kw):
    """One call as a dict of the program's scalars and arrays: the model of `edges` and `biases` (couplings [R][E]: per replica), and
    what `kw` sets; every scalar it leaves out is 0, every array empty."""
    cl = _cl()
    ed, js, hs = cl._model(edges, biases)
    couplings = kw.pop("couplings", None)
    st = np.ascontiguousarray(np.asarray(kw.pop("states", np.zeros((0, len(hs)))), dtype=np.uint8).reshape(-1, len(hs)))
    js, flags = cl._couplings(couplings, js, len(st), 0)
    c = dict({k: 0 for k in SCALARS}, kind=kind, nreplicas=len(st), nvars=len(hs), nedges=len(ed), flags=flags, nspin=NONE, nedge=NONE, nworm=NONE)
    c.update(edges=ed, J=js, biases=hs if hs.any() else hs[:0], states=st, epochs=np.zeros(len(st)))
    c.update(kw)
    assert set(c) <= set(SCALARS) | {k for k, _ in ARRAYS}, sorted(c)
    for k, t in ARRAYS:
        c[k] = np.ascontiguousarray(np.asarray(c.get(k, ()), dtype=t).reshape(-1))
    return c


def _run(kind, edges, biases, states, betas, ncopies, rounds, steps, **kw):
    """A call of one of the three isingmc_classical_host_pt_run* entries, with every output asked for (sized as classical.py sizes
    them)."""
    r, t, n, e = len(states), len(betas), len(biases), len(edges)
    chains = r // t if r % t == 0 else 0
    groups, pairs = (chains // ncopies, ncopies * (ncopies - 1) // 2) if ncopies >= 2 and chains % ncopies == 0 else (0, 0)
    items = groups * pairs * t if kind != RUN else 0
    return _call(kind, edges, biases, states=states, betas=betas, ntemps=t, ncopies=ncopies, rounds=rounds, nsteps=steps, kinds=CR.KINDS_ALL,
                 temp_of=np.arange(r) % t, n_series=rounds * chains * t, n_pairs=chains * (t - 1), n_items=rounds * items, n_hq=items * (n + 1), n_hl=items * (e + 1),
                 n_counts=groups * (ncopies // 2) * t if kind == RUN_ICM else 0, **kw)


def _icm_case(name, measure):
    c = ic.case(name)
    t_first, t_last = _cl()._window(*c["window"])
    return _run(RUN_ICM, c["edges"], c["biases"], ic.initial(c, ic.offset(name)), c["betas"], c["ncopies"], c["rounds"], c["steps"], couplings=c["couplings"],
                seed=cc.SEED, offset=ic.offset(name), measure=measure, t_first=t_first, t_last=t_last)


def calls():
    out = [_icm_case(name, measure) for name in ("ring33_T3_K2", "lattice4x4_T8_K4", "k8_per_replica_T2_K2", "ring200_equal_T2_K2") for measure in (1, 0)]
    k8 = ic.case("k8_T2_K2")
    edges, biases, betas = k8["edges"], k8["biases"], k8["betas"]
    states = pc.initial_states(cc.SEED, 4, len(biases))
    out.append(_run(RUN, edges, biases, states, betas, 0, k8["rounds"], k8["steps"], seed=cc.SEED))
    out.append(_run(RUN_OVERLAPS, edges, biases, states, betas, 2, k8["rounds"], k8["steps"], seed=cc.SEED))
    out.append(_call(STEPS, edges, biases, states=states, betas=[0.3, 1.0, 0.3, 1.0], nsteps=3, kinds=CR.KINDS_ALL, seed=cc.SEED))
    out.append(_call(CLUSTER, *ic.TINY, states=[[1, 0, 1, 1, 0]], other=[0, 0, 0, 1, 1], rank=1))
    out += [_call(ICM_PLAN, nvars=ic.gate(4) + extra, lds_bytes=ic.LDS_BYTES) for extra in (0, 1)]
    # one refusal from each of the four check functions: the ladder, the couplings of a chain, the groups, the window
    mixed = np.arange(4 * len(edges), dtype=np.float64).reshape(4, -1) + 1.0
    out.append(_run(RUN, edges, biases, states, [1.0], 0, 1, 1))
    out.append(_run(RUN, edges, biases, states, betas, 0, 1, 1, couplings=mixed))
    out.append(_run(RUN_OVERLAPS, edges, biases, np.zeros((6, len(biases))), betas, 2, 1, 1))
    out.append(_run(RUN_ICM, edges, biases, states, betas, 2, 1, 1, t_first=1, t_last=1))
    return out


REFUSALS = ("tempering needs ntemps >= 2", "the coupling rows of chain 0", "must be a multiple of ncopies", "[1, 1) is empty or reversed")


def through_the_library(call):
    """The bytes the program writes for `call`, from the same call through the built library."""
    import isingmontecarlo_amd as im
    lib = im.load_library()
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in call.items()}

    def p(x, t):
        return im._ptr(x, t) if len(x) else None
    cfg = im._ClassicalConfig(struct_size=C.sizeof(im._ClassicalConfig), nreplicas=a["nreplicas"], nvars=a["nvars"], nedges=a["nedges"], edges=p(a["edges"], C.c_uint32),
                              J=p(a["J"], C.c_double), biases=p(a["biases"], C.c_double), seed=a["seed"], replica_offset=a["offset"], device=-1, init_state=None,
                              flags=a["flags"])
    moves = (a["nspin"], a["nedge"], a["nworm"], a["kinds"])
    u64 = {k: np.zeros(a[n], dtype=np.uint64) for k, n in (("attempts", "n_pairs"), ("accepts", "n_pairs"), ("hq", "n_hq"), ("hl", "n_hl"), ("moves", "n_counts"),
                                                          ("empty", "n_counts"), ("size_sum", "n_counts"))}
    counters, energy = np.zeros(8 * a["nreplicas"], dtype=np.uint64), np.zeros(a["n_series"], dtype=np.float64)
    mag, q, ql = np.zeros(a["n_series"], dtype=np.int32), np.zeros(a["n_items"], dtype=np.int32), np.zeros(a["n_items"], dtype=np.int32)
    step = C.c_uint64(a["pt_step"])
    batch = (p(a["states"], C.c_uint8), p(a["epochs"], C.c_uint64), p(a["temp_of"], C.c_uint32), C.byref(step), p(counters, C.c_uint64), p(u64["attempts"], C.c_uint64),
             p(u64["accepts"], C.c_uint64), p(energy, C.c_double), p(mag, C.c_int32))
    measured = (p(q, C.c_int32), p(ql, C.c_int32), p(u64["hq"], C.c_uint64), p(u64["hl"], C.c_uint64))
    head = (C.byref(cfg), a["ntemps"], p(a["betas"], C.c_double))
    kind = a["kind"]
    if kind == RUN:
        rc = lib.isingmc_classical_host_pt_run(*head, a["rounds"], a["nsteps"], *moves, *batch)
    elif kind == RUN_OVERLAPS:
        rc = lib.isingmc_classical_host_pt_run_overlaps(*head, a["ncopies"], a["rounds"], a["nsteps"], *moves, *batch, *measured)
    elif kind == RUN_ICM:
        rc = lib.isingmc_classical_host_pt_run_icm(*head, a["ncopies"], a["rounds"], a["nsteps"], *moves, *batch, *measured, a["measure"], a["t_first"], a["t_last"],
                                                   *(p(u64[k], C.c_uint64) for k in ("moves", "empty", "size_sum")))
    elif kind == STEPS:
        rc = lib.isingmc_classical_host_steps(C.byref(cfg), a["nsteps"], p(a["betas"], C.c_double), *moves, p(a["states"], C.c_uint8), p(a["epochs"], C.c_uint64),
                                              p(counters, C.c_uint64))
    elif kind == CLUSTER:
        mask, size = np.full(a["nvars"], 0xAB, dtype=np.uint8), C.c_uint32(0)
        rc = lib.isingmc_classical_host_icm_cluster(C.byref(cfg), p(a["states"], C.c_uint8), p(a["other"], C.c_uint8), a["rank"], p(mask, C.c_uint8), C.byref(size))
    else:
        plan = (C.c_uint32 * 4)()
        rc = lib.isingmc_classical_icm_plan(a["nvars"], a["lds_bytes"], plan)
    why = lib.isingmc_classical_last_error(None) if rc else b""
    out = [struct.pack("<iQ", rc, len(why)), why]
    if kind in (RUN, RUN_OVERLAPS, RUN_ICM):
        out += [a["states"], a["epochs"], a["temp_of"], struct.pack("<Q", step.value), counters, u64["attempts"], u64["accepts"], energy, mag, q, ql, u64["hq"], u64["hl"],
                u64["moves"], u64["empty"], u64["size_sum"]]
    elif kind == STEPS:
        out += [a["states"], a["epochs"], counters]
    elif kind == CLUSTER:
        out += [mask, struct.pack("<I", size.value)]
    else:
        out += [bytes(plan)]
    return b"".join(x if isinstance(x, bytes) else x.tobytes() for x in out), rc, why.decode()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "isingmontecarlo_amd", "csrc")
    hipcc = os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "include")
    d = tmp_path_factory.mktemp("classical_host")
    src = d / "classical_host_main.cpp"
    src.write_text(PROGRAM.replace("../../include/isingmc_hip.h", os.path.join(root, "include", "isingmc_hip.h")))
    exe = str(d / "classical_host_main")
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-isystem", rocm_include, "-I" + csrc, os.path.join(csrc, "classical_host.hip"), str(src),
                           "-o", exe])
    return exe


def test_the_device_free_unit_runs_clean_and_agrees_with_the_library(program, tmp_path):
    """The link of `program` is the first check.  Then every call of calls(): the parity cases of the cluster moves with and without
    the measurement, the plain and the measuring rounds, the step loop, one cluster, the plan at the four-wave gate and one past it, and
    four refusals with their texts; the sanitizers stop the program at the first finding."""
    todo = calls()
    inputs, outputs = tmp_path / "calls.bin", tmp_path / "outputs.bin"
    with open(inputs, "wb") as f:
        f.write(struct.pack("<Q", len(todo)))
        for c in todo:
            f.write(struct.pack("<%dQ" % len(SCALARS), *(int(c[k]) for k in SCALARS)))
            for k, _ in ARRAYS:
                f.write(struct.pack("<Q", len(c[k])) + c[k].tobytes())
    p = subprocess.run([program, str(inputs), str(outputs)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-2000:] + p.stderr[-4000:]
    want = [through_the_library(c) for c in todo]
    got = outputs.read_bytes()
    at = 0
    for i, (c, (blob, rc, why)) in enumerate(zip(todo, want)):
        assert got[at:at + len(blob)] == blob, (i, c["kind"])
        at += len(blob)
    assert at == len(got)
    assert [rc for _, rc, _ in want[:-4]] == [0] * (len(want) - 4)
    for (_, rc, why), words in zip(want[-4:], REFUSALS):
        assert rc == -1 and words in why, (rc, why)
    first = todo[0]  # (the first case did run: its step number advanced by its rounds, and every item of its window moved or was empty)
    tail = np.frombuffer(want[0][0][-3 * 8 * first["n_counts"]:], dtype=np.uint64).reshape(3, -1)
    assert first["rounds"] > 0 and (tail[0] + tail[1]).max() == first["rounds"] and tail[2].sum() >= tail[0].sum() > 0
