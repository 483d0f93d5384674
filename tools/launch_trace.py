"""Which launches does each kind of call make?  Runs a fixed list of small scenarios through the public Python API and prints, per
scenario, launch_info() and the three launch counters of its last call.  The printed lines hold no timings: two builds that plan
their launches alike print the same text.  Under a kernel trace,

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_trace.py
    python tools/launch_trace.py --normalise OUT/*/*_kernel_trace.csv > trace.txt

the second command reduces the trace to kernel name, grid, workgroup and LDS size per dispatch, in dispatch order: the sequence
that must not change when the host driver is refactored (profiles/r06_launch_trace.txt is the one it had then)."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def normalise(paths):
    rows = []
    for p in paths:
        with open(p, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        grid = "x".join(r[k] for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
        wg = "x".join(r[k] for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z"))
        print(r["Kernel_Name"], grid, wg, r["LDS_Block_Size"])


def scenarios():
    import numpy as np
    import _lattices as lat
    import isingmontecarlo_amd as im

    def counters(g):
        return "launches=%d pass=%s rvb=%d" % (g.last_kernel_ms()[1], g.last_pass_ms()[1], g.last_rvb_ms()[1])

    def show(name, g):
        print(name, "|", " ".join(f"{k}={v}" for k, v in sorted(g.launch_info().items())), "|", counters(g), flush=True)
        assert g.verify().all(), name
        g.close()

    def small(cfg=0, l=4, **kw):
        return im.QmcIsingGraph(lat.two_d_ferro(l), 1.0, 0.0, 16, 2024, nreplicas=3, capacity=4096, cfg_flags=cfg, **kw)

    def steps(name, g, flags=0, spl=None, record_freq=0, t=20, beta=1.0):
        if spl is not None:
            g.set_steps_per_launch(spl)
        if record_freq:
            g.attach_sample_record(t // record_freq)
        g.run(t, beta, sampling_freq=record_freq or 1, flags=flags)
        show(name, g)

    steps("default", small())
    steps("loop", small(), im.FLAG_LOOP)
    steps("rvb", small(), im.FLAG_RVB)
    steps("rvb_loop", small(), im.FLAG_RVB | im.FLAG_LOOP)
    steps("rvb_fused_kernel", small(im.CFG_RVB_FUSED), im.FLAG_RVB)
    steps("rvb_global_tables", small(im.CFG_RVB_GLOBAL_TABLES), im.FLAG_RVB)
    steps("rvb_global_tables_loop", small(im.CFG_RVB_GLOBAL_TABLES), im.FLAG_RVB | im.FLAG_LOOP)
    steps("rvb_global_tables_fused_launch", small(im.CFG_RVB_GLOBAL_TABLES | im.CFG_FUSED_LAUNCH), im.FLAG_RVB)
    steps("fused_launch_7", small(im.CFG_FUSED_LAUNCH), spl=7)
    steps("fused_launch_7_record_3", small(im.CFG_FUSED_LAUNCH), spl=7, record_freq=3)
    steps("heatbath", small(), im.FLAG_HEATBATH)
    steps("no_lean_cluster", small(im.CFG_NO_LEAN_CLUSTER))
    steps("no_deferred_flips", small(im.CFG_NO_DEFERRED_FLIPS))
    steps("no_fast_diag", small(im.CFG_NO_FAST_DIAG))
    steps("global_tables_6x6", small(im.CFG_GLOBAL_TABLES | im.CFG_NO_LDS_TABLES, l=6))
    steps("lds_uf_ids_limit", small(lds_uf_ids_limit=64))
    for w in (1, 6, 8, 16):
        steps(f"waves_per_replica_{w}", small(waves_per_replica=w))
    steps("waves_offdiag_8", small(waves_offdiag=8))
    # the 8-wave geometry with the union-find in HBM and the flip bits in LDS
    steps("ferro64_beta16", im.QmcIsingGraph(lat.two_d_ferro(64), 1.0, 0.0, 4096, 64, nreplicas=2, capacity=1 << 20), t=40, beta=16.0)
    # the +-J diagonal mode
    edges = lat.cubic_periodic(32)
    J = np.random.default_rng(32768).choice([-1.0, 1.0], size=(2, len(edges)))
    steps("pmj_cubic32", im.QmcIsingGraph(edges, 1.0, 0.1, 32 ** 3, 2026, nreplicas=2, capacity=1 << 21, couplings=J), beta=4.0)
    single = {
        "diagonal_update": lambda g: g.single_diagonal_step(1.0),
        "cluster_update": lambda g: g.single_cluster_step(flip_free=False),
        "loop_update": lambda g: g.loop_update(),
        "rvb_update": lambda g: g.single_rvb_sweep(),
        "flip_free_spins": lambda g: g.flip_free_spins(),
    }
    for name, update in single.items():
        g = small()
        g.run(20, 1.0)
        update(g)
        show(name, g)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--normalise":
        normalise(sys.argv[2:])
    else:
        scenarios()
