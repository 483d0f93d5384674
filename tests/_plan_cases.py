"""Configs as data: the cases of tests/golden/batch_plans.json name a model of _lattices and the wishes of an isingmc_config;
config_of() builds the struct that QmcIsingGraph / Qmc.from_interactions would hand to isingmc_create, without creating anything."""
import ctypes as C

import numpy as np

import _lattices as lat

# out[] of isingmc_plan_batch (include/isingmc_hip.h)
SLOTS = ["W", "K", "mode", "W_off", "Wmax", "w8_ok", "CH", "nchunks", "stride", "pm_words", "lds_words_pm_diag", "lds_words_diag",
         "lds_words_fast", "fast_diag", "lean_cluster", "defer", "lds_words_rvb", "rvb_global", "rvb_split", "rvb_main_W", "tbl_stride",
         "ufstride_lo", "ufstride_hi", "lds_words", "lds_ufcap", "nwords", "Nb"]
MODE_GENERAL, MODE_LDS_EDGES, MODE_GLOBAL_TABLES, MODE_PM_GLOBAL_TABLES = 0, 1, 2, 4
LADDER = {name: (edges, nvars, h) for name, edges, nvars, h in lat.LADDER}


def model_of(spec):
    """spec = [kind, *parameters] -> dict(edges, nvars, transverse, longitudinal[, couplings, transverse_r, longitudinal_r,
    interactions])"""
    kind, args = spec[0], spec[1:]
    if kind == "ladder":          # a rung of _lattices.LADDER by name
        edges, nvars, h = LADDER[args[0]]
        return dict(edges=edges, nvars=nvars, transverse=1.0, longitudinal=h)
    if kind == "ferro":           # l x l ferromagnet (the benchmark's and tools/launch_trace.py's lattice)
        return dict(edges=lat.two_d_ferro(args[0]), nvars=args[0] ** 2, transverse=1.0, longitudinal=0.0)
    if kind == "cubic_pm":        # l^3 lattice, R rows of +-1 couplings drawn with the given seed, h = 0.1
        l, R, seed = args
        edges = lat.cubic_periodic(l)
        J = np.random.default_rng(seed).choice([-1.0, 1.0], size=(R, len(edges)))
        return dict(edges=edges, nvars=l ** 3, transverse=1.0, longitudinal=0.1, couplings=J)
    if kind == "fields_r":        # ring of n sites, R replicas with fields of their own
        n, R = args
        return dict(edges=lat.one_d_periodic(n), nvars=n, transverse=1.0, longitudinal=0.2,
                    transverse_r=np.linspace(0.5, 1.5, R), longitudinal_r=np.linspace(0.1, 0.4, R))
    if kind == "xxz_ring":        # generic interactions
        return dict(edges=[], nvars=args[0], transverse=0.0, longitudinal=0.0, interactions=lat.xxz_ring_interactions(args[0]))
    raise ValueError(spec)


def config_of(im, case, model=None):
    """(isingmc_config, the arrays it points to) for a case: dict(model=spec, nreplicas, capacity[, cutoff, flags, waves_per_replica,
    slots_per_lane, waves_offdiag, lds_uf_ids_limit]).  `model` overrides model_of(case["model"]) (error tests)."""
    m = dict(model_of(case["model"])) if model is None else dict(model)
    R = int(case["nreplicas"])
    keep = []

    def ptr(a, dtype, ctype):
        a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ctype))

    flags = int(case.get("flags", 0))
    cfg = im._Config(struct_size=C.sizeof(im._Config), nreplicas=R, nvars=m["nvars"], transverse=m["transverse"], longitudinal=m["longitudinal"],
                     capacity=int(case["capacity"]), cutoff0=int(case.get("cutoff", min(m["nvars"], case["capacity"]))), seed=17, device=-1,
                     waves_per_replica=int(case.get("waves_per_replica", 0)), slots_per_lane=int(case.get("slots_per_lane", 0)),
                     lds_uf_ids_limit=int(case.get("lds_uf_ids_limit", 0)), waves_offdiag=int(case.get("waves_offdiag", 0)))
    if m.get("interactions") is not None:
        arr = (im._Interaction * len(m["interactions"]))()
        for i, (mat, vs) in enumerate(m["interactions"]):
            arr[i].nvars, arr[i].diagonal_only = len(vs), 1 if len(mat) == 2 ** len(vs) else 0
            arr[i].vars[0], arr[i].vars[1] = vs[0], vs[1] if len(vs) == 2 else 0
            arr[i].mat = ptr(mat, np.float64, C.c_double)
        keep.append(arr)
        cfg.interactions, cfg.ninteractions = C.cast(arr, C.c_void_p), len(arr)
    else:
        edges = m["edges"]
        J = np.array([j for _, j in edges], dtype=np.float64)
        per_replica = any(m.get(k) is not None for k in ("couplings", "transverse_r", "longitudinal_r"))
        if m.get("couplings") is not None:
            J = np.asarray(m["couplings"], dtype=np.float64)
        elif per_replica:  # per-replica tables with the same couplings everywhere
            J = np.broadcast_to(J, (R, len(edges))).copy()
        if per_replica and not case.get("without_per_replica_flag"):
            flags |= im.CFG_PER_REPLICA_J
        cfg.nedges = len(edges)
        cfg.edges = ptr(np.array([ab for ab, _ in edges], dtype=np.uint32).reshape(-1, 2), np.uint32, C.c_uint32)
        cfg.J = ptr(J, np.float64, C.c_double)
        if m.get("transverse_r") is not None:
            cfg.transverse_r = ptr(m["transverse_r"], np.float64, C.c_double)
        if m.get("longitudinal_r") is not None:
            cfg.longitudinal_r = ptr(m["longitudinal_r"], np.float64, C.c_double)
    cfg.flags = flags
    return cfg, keep


def plan_batch(im, cfg, lds_bytes):
    """(return code, the 32 slots) of isingmc_plan_batch"""
    out = (C.c_uint32 * 32)()
    rc = im.load_library().isingmc_plan_batch(C.byref(cfg), int(lds_bytes), out)
    return rc, [int(x) for x in out]
