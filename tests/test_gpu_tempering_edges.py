"""Tempering parity beyond the 4x4 corner (single rank): chain layouts of the decision kernel, states of several words, strings of
many 256-slot chunks, every update rule and launch geometry under device-resident betas, the step counter across 2^32, per-slot
Hamiltonians with two chains, mode toggles, checkpoints and the accumulator rows of a bare C-ABI caller.  Every case is compared bit
for bit with the graph-swapping reference of _pt_reference.py (cases and cached references: _pt_cases.py), which test_tempering_cpu.py
has shown to swap where the case looks."""
import ctypes as C

import numpy as np
import pytest

import _pt_cases as pc

pytestmark = pytest.mark.gpu

DEVICE, NOREAD, HOST = "device", "device, nothing read back between steps", "host"
WHERE = [DEVICE, NOREAD, HOST]


def build(c, flags=None, **geometry):
    import isingmontecarlo_amd as im
    T, K = len(c["betas"]), c["K"]
    kw = dict(geometry)
    hams = pc.slot_hamiltonians(c)
    if hams is not None:
        kw.update(couplings=hams[0], transverse_r=hams[1], longitudinal_r=hams[2])
    gamma, h = (1.0, 0.1) if hams is not None else (c["gamma"], c["h"])  # (ignored with per-slot fields; h != 0 there)
    g = im.QmcIsingGraph(pc.edges_of(c), gamma, h, c["cutoff"], c["seed"], nreplicas=T * K, capacity=c["capacity"], **kw)
    tc = im.NativeTemperingContainer(g, np.array(c["betas"]), K, c["seed"], flags=c["flags"] if flags is None else flags)
    return g, tc


def drive(tc, c, where, nsteps):
    """`nsteps` blocks of sweeps + one tempering step; returns the swaps the steps reported."""
    if where == HOST:
        tc.set_device_decisions(False)
    counted = 0
    for _ in range(nsteps):
        tc.timesteps(c["sweeps"])
        counted += tc.tempering_step(count_swaps=where != NOREAD) or 0
    assert tc.device_decisions == (where != HOST)
    return counted


def compare(g, tc, c, ref, what=""):
    """Everything a label, row or copy bug could touch, bit for bit."""
    K = c["K"]
    assert tc.get_total_swaps() == ref.swaps, what
    st, n, cut, ep = g.state_ref(), g.get_n(), g.get_cutoff(), g.get_epoch()
    slot_of, config_of = tc.slot_of, tc.config_of
    assert sorted(slot_of.tolist()) == list(range(g.nreplicas)), what
    for r in range(g.nreplicas):
        s = int(slot_of[r])
        t, k = divmod(s, K)
        rep = ref.by_slot[k][t]
        w = f"{what} replica {r} at slot (t={t}, k={k})"
        assert int(config_of[r]) == int(ref.ids[s]), w
        assert n[r] == rep.n and cut[r] == rep.cutoff and ep[r] == rep.epoch, w
        assert np.array_equal(st[r], rep.state()), w
        assert np.array_equal(g.export_ops(r), rep.ops()), w
    assert tc.verify(), what
    acc = g.accumulators()
    assert acc.shape == ref.acc.shape
    bad = np.nonzero((acc[:, :7] != ref.acc[:, :7]).any(axis=1))[0]
    assert len(bad) == 0, f"{what} accumulator rows {bad.tolist()[:8]} differ: {acc[bad[:2]].tolist()} vs {ref.acc[bad[:2]].tolist()}"


def run_case(c, where, flags=None, check_launch=None, **geometry):
    ref = pc.check_preconditions(c)  # the same counts the CPU suite asserts, from the reference compared against
    g, tc = build(c, flags=flags, **geometry)
    if c["hams"]:
        assert not tc.device_decisions  # different Hamiltonians decide on the host
        import isingmontecarlo_amd as im
        with pytest.raises(im.IsingMcError) as e:
            tc.set_device_decisions(True)
        assert e.value.code == -5
        where = HOST
    else:
        assert tc.device_decisions
    counted = drive(tc, c, where, c["steps"])
    assert counted == (0 if where == NOREAD else ref.swaps)
    compare(g, tc, c, ref, f"{c['name']} [{where}]")
    if check_launch:
        check_launch(g.launch_info())  # (which kernels the last sweep ran through)
    return g, tc


# ---- layouts of the decision kernel ----
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("c", pc.LAYOUTS, ids=[c["name"] for c in pc.LAYOUTS])
def test_layouts(oracle, c, where):
    """(T, K): one temperature (the step only counts), two and three (odd T: the top pair is in one set only), 5 x 3, K = 65 (a second,
    nearly empty wave) and K = 300 (the chain loop strides, the shared swap counter sums over 256 threads)."""
    run_case(c, where)
    if len(c["betas"]) == 1:
        assert pc.reference(c)[0].swaps == 0


# ---- several state words, long strings ----
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("c", pc.LONG, ids=[c["name"] for c in pc.LONG])
def test_multiword_states_and_long_strings(oracle, c, where):
    """65 sites: three state words, the last holding one bit; 16 x 16: eight words, strings of more than seven 256-slot chunks, swept by
    the trimmed diagonal and the dedicated cluster kernel, whose deferred flips the host path has to materialise before it steps."""
    def launch(info):
        assert info["state_words"] == (pc.nvars_of(c) + 31) // 32
        if c["name"] == "ferro16x16":
            assert info["fast_diagonal"] and info["lean_cluster"]
    g, _ = run_case(c, where, check_launch=launch)
    assert g.get_cutoff().max() > (1024 if c["name"] == "ring65" else 7 * 256)


# ---- device-resident betas into every kind of launch ----
def geometries():
    import isingmontecarlo_amd as im
    return {"default": {}, "w8k2_general_cluster": dict(waves_per_replica=8, slots_per_lane=2, cfg_flags=im.CFG_NO_LEAN_CLUSTER),
            "fused": dict(cfg_flags=im.CFG_FUSED_LAUNCH), "rvb_global_tables": dict(cfg_flags=im.CFG_RVB_GLOBAL_TABLES)}


RULE_GEOMETRIES = [(c, geo) for c in pc.RULES for geo in ("default", "w8k2_general_cluster", "fused")] + \
                  [(c, "rvb_global_tables") for c in pc.RULES if c["flags"] == pc.RVB]
REFUSED = {}  # (flags, geometry) -> error code of isingmc_create or of the sweep; none at this size


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("c,geo", RULE_GEOMETRIES, ids=[f"{c['name']}-{geo}" for c, geo in RULE_GEOMETRIES])
def test_device_betas_reach_every_launch(oracle, c, geo, where):
    """isingmc_pt_timesteps hands the sweep driver a device pointer to the betas: general split kernels, trimmed diagonal + dedicated
    cluster kernel, the fused kernel, the RVB launches (split, fused, tables in HBM) and the heat-bath pass must all read it."""
    import isingmontecarlo_amd as im
    code = REFUSED.get((c["flags"], geo))
    if code is not None:
        with pytest.raises(im.IsingMcError) as e:
            run_case(c, where, **geometries()[geo])
        assert e.value.code == code
        return
    def launch(info):
        if geo == "default":
            assert info["split_launches"] and info["fast_diagonal"]
            assert info["lean_cluster"] or c["flags"] & (pc.LOOP | pc.RVB)
            if not c["flags"] & pc.LOOP:  # (growth launch + main launch when the RVB sweep is the only off-diagonal pass besides the cluster update)
                assert info["rvb_split"] == bool(c["flags"] & pc.RVB)
        elif geo == "w8k2_general_cluster":
            assert info["waves_per_replica"] == 8 and info["slots_per_lane"] == 2 and not info["lean_cluster"]
        elif geo == "fused":
            assert not info["split_launches"]
        else:
            assert info["rvb_global_tables"]
    run_case(c, where, check_launch=launch, **geometries()[geo])


# ---- the step counter across 2^32 ----
@pytest.mark.parametrize("where", [DEVICE, HOST])
def test_step_counter_crosses_2_to_32(oracle, where):
    """Philox counter word 3 carries step >> 32: steps 2^32 - 3 .. 2^32 + 2 draw from both sides of the carry."""
    c = pc.STEP32
    ref = pc.check_preconditions(c)
    g, tc = build(c)
    ident = np.arange(g.nreplicas, dtype=np.uint32)
    p = ident.ctypes.data_as(C.POINTER(C.c_uint32))
    g._check(g._lib.isingmc_pt_set_state(g._h, p, p, c["step0"], 0))
    tc._stale = True
    assert drive(tc, c, where, c["steps"]) == ref.swaps
    step = C.c_uint64(0)
    g._check(g._lib.isingmc_pt_get_state(g._h, C.byref(step), None))
    assert step.value == 2 ** 32 + 3
    compare(g, tc, c, ref, f"{c['name']} [{where}]")


# ---- per-slot Hamiltonians, two chains ----
@pytest.mark.parametrize("c", pc.HAMS, ids=[c["name"] for c in pc.HAMS])
def test_per_slot_hamiltonians_two_chains(oracle, c):
    """J, Gamma and h differ between the slots and K = 2: bond-table rows, relative weights and energy offsets are indexed by
    t*K + k; with RVB the two RVB split kernels apply the replicas' bond-table rows themselves."""
    def launch(info):
        assert info["rvb_split"] == (c["flags"] == pc.RVB)
    g, tc = run_case(c, HOST, check_launch=launch)
    _, hams = pc.reference(c)
    off, slot_of = g.get_offsets(), tc.slot_of
    for r in range(g.nreplicas):
        assert abs(off[r] - hams.offset(int(slot_of[r]))) < 1e-12


# ---- mode toggle, checkpoint ----
def test_swap_total_survives_mode_toggles(oracle):
    """Four steps on the device, four on the host, four on the device again: the total and every label follow the reference."""
    c = pc.TOGGLE
    g, tc = build(c)
    for leg, on in enumerate([True, False, True]):
        tc.set_device_decisions(on)
        for _ in range(4):
            tc.timesteps(c["sweeps"])
            tc.tempering_step(count_swaps=False)
        assert tc.device_decisions == on
        ref = pc.reference(c, nsteps=4 * (leg + 1))[0]
        assert ref.swaps > 0 and tc.get_total_swaps() == ref.swaps == tc.total_swaps_local, f"after leg {leg}"
    compare(g, tc, c, pc.check_preconditions(c), c["name"])


def test_checkpoint_in_the_device_leg_resumes_bit_exactly(oracle, tmp_path):
    """save() after device-decided steps (T = 5), load() into a fresh container: same swaps_local, same continuation."""
    c = pc.TOGGLE
    g1, t1 = build(c)
    drive(t1, c, NOREAD, 6)
    path = str(tmp_path / "ck")
    t1.save(path)
    mid = pc.reference(c, nsteps=6)[0]
    z = np.load(path + ".pt.npz")
    assert int(z["swaps_local"]) == int(z["swaps"]) == mid.swaps > 0 and int(z["step"]) == 6
    g2, t2 = build(c)
    t2.load(path)
    assert t2.device_decisions and t2.total_swaps_local == mid.swaps
    ref = pc.check_preconditions(c)
    for g, tc in ((g1, t1), (g2, t2)):
        drive(tc, c, NOREAD, c["steps"] - 6)
        compare(g, tc, c, ref, c["name"])


# ---- a C-ABI caller who never set accumulator rows ----
def test_c_abi_accumulator_rows_are_the_same_on_both_paths(oracle):
    """isingmc_pt_create on a fresh batch, no isingmc_set_accumulator_rows: row r stays replica r's, whether the decisions run on the
    device or on the host (rows follow the slots only for a caller who passed the slots as rows)."""
    import isingmontecarlo_amd as im
    from isingmontecarlo_amd import _PtLayout
    c = pc.BY_NAME["T5_K3"]
    ref = pc.check_preconditions(c)
    T, K = len(c["betas"]), c["K"]
    tables = {}
    for where in (DEVICE, HOST):
        g = im.QmcIsingGraph(pc.edges_of(c), c["gamma"], c["h"], c["cutoff"], c["seed"], nreplicas=T * K, capacity=c["capacity"])
        betas = np.array(c["betas"])
        lay = _PtLayout(struct_size=C.sizeof(_PtLayout), ntemps=T, nchains=K, rank=0, world=1, betas=betas.ctypes.data_as(C.POINTER(C.c_double)),
                        seed=c["seed"], transport=None)
        g._check(g._lib.isingmc_pt_create(g._h, C.byref(lay)))
        if where == HOST:
            g._check(g._lib.isingmc_pt_set_device_decisions(g._h, 0))
        sw = C.c_uint64(0)
        for _ in range(c["steps"]):
            g._check(g._lib.isingmc_pt_timesteps(g._h, c["sweeps"], 1, 0))
            g._check(g._lib.isingmc_pt_step(g._h, C.byref(sw)))
        assert sw.value == ref.swaps
        slot_of = np.zeros(T * K, dtype=np.uint32)
        g._check(g._lib.isingmc_pt_get_slots(g._h, slot_of.ctypes.data_as(C.POINTER(C.c_uint32)), None, None))
        tables[where] = (g.accumulators(), slot_of)
    (dev, slots_d), (host, slots_h) = tables[DEVICE], tables[HOST]
    assert np.array_equal(slots_d, slots_h) and np.array_equal(dev, host)
    # rows by replica hold the same samples as the reference's rows by slot, binned differently
    assert np.array_equal(dev[:, :7].sum(axis=0), ref.acc[:, :7].sum(axis=0))
    assert (dev[:, 1] == c["steps"] * c["sweeps"]).all() and not np.array_equal(dev[:, :7], ref.acc[:, :7])
