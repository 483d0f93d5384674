#!/usr/bin/env python3
"""What the sample record costs and what the bit-series autocorrelation takes, at the headline model (bench.py's configs[1]: 32x32
ferromagnet, Gamma = 1, beta = 16, 1024 replicas, directed loops on).  For T in --T at sampling_freq = 1, after equilibration and a
warm-up of every shape, the variants alternating inside this one process (--reps rounds, medians reported):

1. ms per step of run(T) without a record, with a record attached, and of the loop `run(1); state_ref()` (one call, one blocking
   copy of [R][nwords] and an R x N unpack per sample: the only way to the same states without the record);
2. ms of record_autocorrelation over all N variables (host clock around the blocking call), ms and peak device memory of
   fft_autocorrelation_device on the same states where it runs; where it does not fit, the reason is recorded;
3. the largest difference between the two results.

The split of (2) into the two kernels comes from a run of its own under the profiler,
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/bench_autocorr.py --profile-pass
whose kernel trace `--merge-trace DIR/.../*_kernel_trace.csv` adds to the JSON written before.

usage: python tools/bench_autocorr.py [--out profiles/r05_autocorr.json]
"""
import argparse, csv, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_autocorr.json"))
ap.add_argument("--T", type=int, nargs="+", default=[256, 1024, 4096])
ap.add_argument("--L", type=int, default=32)
ap.add_argument("--replicas", type=int, default=1024)
ap.add_argument("--beta", type=float, default=16.0)
ap.add_argument("--equilibrate", type=int, default=80)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--loop-samples", type=int, default=512, help="samples of the run(1); state_ref() loop per round (its cost per sample does not depend on T)")
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--profile-pass", action="store_true", help="only record T samples and call record_autocorrelation twice per T (for the profiler)")
ap.add_argument("--merge-trace", default=None, help="a rocprofv3 kernel-trace CSV of a --profile-pass run: add the per-kernel ms to --out and exit")
a = ap.parse_args()

KERNELS = ("record_series_kernel", "bit_autocorr_kernel")
if a.merge_trace:
    # dispatches in time order: per T two calls, each one launch of each kernel; the second call of every T is reported
    rows = sorted(csv.DictReader(open(a.merge_trace)), key=lambda r: int(r["Start_Timestamp"]))
    per = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows if k in r["Kernel_Name"]] for k in KERNELS}
    out = json.load(open(a.out))
    for k in KERNELS:
        assert len(per[k]) == 2 * len(out["T"]), (k, len(per[k]))
    for i, t in enumerate(out["T"]):
        out["per_T"][str(t)]["kernel_ms_rocprofv3"] = {k: per[k][2 * i + 1] for k in KERNELS}
    out["kernel_ms_rocprofv3_source"] = "rocprofv3 --kernel-trace, a --profile-pass run of its own; second of two calls per T"
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps({str(t): out["per_T"][str(t)]["kernel_ms_rocprofv3"] for t in out["T"]}))
    sys.exit(0)

import numpy as np
import torch  # (initialised before the library: see tests/conftest.py)
import _lattices as lat
import isingmontecarlo_amd as im
from isingmontecarlo_amd.autocorrelations import fft_autocorrelation_device, variable_groups

if not torch.cuda.is_available():
    raise SystemExit("bench_autocorr.py needs a HIP device (no CPU fallback)")
L, R, beta, flags = a.L, a.replicas, a.beta, im.FLAG_LOOP
edges = lat.two_d_ferro(L)
n_est = beta * (3 * L * L + 2.2 * L * L)
cap = 1 << int(np.ceil(np.log2(2.0 * n_est + 4 * L * L)))
g = im.QmcIsingGraph(edges, 1.0, 0.0, L * L, a.seed, nreplicas=R, capacity=cap)
for _ in range(0, a.equilibrate, 10):
    g.run(min(10, a.equilibrate), beta, flags=flags)
groups = variable_groups(g.nvars)[0]
nwords = g.launch_info()["state_words"]


def timed(fn):
    torch.cuda.synchronize(); g.synchronize()
    t0 = time.perf_counter()
    r = fn()
    g.synchronize(); torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def loop_states(n):
    out = []
    for _ in range(n):
        g.run(1, beta, flags=flags)
        out.append(g.state_ref())
    return out


res = {"model": f"{L}x{L} ferromagnet Gamma=1 beta={beta}, {R} replicas, FLAG_LOOP (bench.py configs[1])", "T": a.T, "sampling_freq": 1,
       "record_bytes_per_sample": R * nwords * 4, "reps": a.reps, "per_T": {}}
for T in a.T:
    if a.profile_pass:
        g.attach_sample_record(T)
        g.run(T, beta, flags=flags)
        g.record_autocorrelation(groups)
        g.record_autocorrelation(groups)
        g.detach_sample_record()
        continue
    nloop = min(T, a.loop_samples)
    g.run(8, beta, flags=flags); loop_states(4)  # warm-up of the shapes
    ms = {"run_no_record": [], "run_with_record": [], "loop_run1_state_ref": []}
    g.detach_sample_record()
    for rnd in range(a.reps):  # the variants alternate inside a round
        if rnd:
            g.detach_sample_record()
        ms["run_no_record"].append(timed(lambda: g.run(T, beta, flags=flags))[0] / T)
        ms["loop_run1_state_ref"].append(timed(lambda: loop_states(nloop))[0] / nloop)
        g.attach_sample_record(T)  # (attaching again starts an empty record; the last round's stays for part 2)
        ms["run_with_record"].append(timed(lambda: g.run(T, beta, flags=flags))[0] / T)
    e = {"ms_per_step": {k: {"median": statistics.median(v), "all": v} for k, v in ms.items()}, "loop_samples": nloop}
    # the record of the last round is still attached: T samples
    assert g.record_count() == T
    g.record_autocorrelation(groups)  # warm-up (allocates the series buffer)
    rec_ms, ac = [], None
    for _ in range(a.reps):
        t_ms, ac = timed(lambda: g.record_autocorrelation(groups))
        rec_ms.append(t_ms)
    e["record_autocorrelation_ms"] = {"median": statistics.median(rec_ms), "all": rec_ms}
    e["series_buffer_bytes"] = R * len(groups) * ((T + 31) // 32) * 4
    e["record_bytes"] = T * R * nwords * 4
    # the float path on the same states: [T][R][N] float64 on the host, then hipFFT
    in_bytes = T * R * g.nvars * 8
    e["fft_input_bytes_float64"] = in_bytes
    free_dev = torch.cuda.mem_get_info()[0]
    avail_host = os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
    try:  # a container's own limit, where it has one
        lim, cur = open("/sys/fs/cgroup/memory.max").read().strip(), open("/sys/fs/cgroup/memory.current").read().strip()
        if lim != "max":
            avail_host = min(avail_host, int(lim) - int(cur))
    except OSError:
        pass
    fft = {"device_free_bytes_before": int(free_dev), "host_available_bytes_before": int(avail_host)}
    if 3 * in_bytes > avail_host:
        fft["error"] = f"not attempted: the float64 input is {in_bytes} bytes and the host has {avail_host} available (the path holds the uint8 states, the float64 array and torch's copy)"
    else:
        try:
            t_read, st = timed(lambda: g.record_states())
            fft["record_states_ms"] = t_read
            torch.cuda.reset_peak_memory_stats()
            t_ms, want = timed(lambda: fft_autocorrelation_device(st.astype(np.float64) * 2.0 - 1.0))
            fft["ms"] = t_ms
            fft["peak_device_bytes"] = int(torch.cuda.max_memory_allocated())
            e["max_abs_difference"] = float(np.abs(ac - want).max())
            del st, want
        except (RuntimeError, MemoryError) as ex:  # does not fit: recorded, not worked around
            fft["error"] = f"{type(ex).__name__}: {str(ex)[:300]}"
        torch.cuda.empty_cache()
    e["fft_autocorrelation_device"] = fft
    g.detach_sample_record()
    res["per_T"][str(T)] = e
    print(T, json.dumps(e), flush=True)
if not a.profile_pass:
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({"out": a.out}))
