"""The queues of parked unions in the dedicated cluster kernel's LDS (csrc/sse_cluster.hip.h, ClLds::carve: o_queue), audited on
the host through isingmc_plan_cluster_queue and isingmc_plan_cluster_lds over the N / ufcap / field grid of
test_abi_cpu.py::test_dedicated_cluster_kernel_lds_layout_and_gate.

Every wave of the kernel owns a stretch of the region: its queue entries, the count of them and the count of full queues it has
served.  The build scan writes there while the per-wave tables and the parent table are live, and the words are dead once the
scan's barrier is passed, so the region must lie inside the launch's LDS and touch none of: the set-up tables in front of it, the
per-wave tables o_ent (which later hold the flip bits and the root list), the frozen bits, the parent table.  The launch grows by
exactly the region."""
import ctypes as C

import numpy as np

CLUSTER_WAVES = 16  # SSE_CLW


def test_queue_region_of_the_cluster_kernel():
    import isingmontecarlo_amd as im
    lib = im.load_library()
    out, q = (C.c_uint32 * 13)(), (C.c_uint32 * 3)()
    rng = np.random.default_rng(11)
    Ns = sorted(set(range(1, 257)) | set(range(257, 4096, 37)) | {511, 512, 1023, 1024, 1025, 2047, 2048, 4071, 4072, 4094, 4095})
    seen = 0
    for N in Ns:
        tab = CLUSTER_WAVES * (N + 1)
        bound = 32 * tab
        nwords = (N + 31) // 32
        ufcaps = {65535, min(65535, 16 * N + 384), min(65535, bound + 1), min(65535, bound), min(65535, 16 * N + 3000 + 3000 // 16 + 384)}
        for has_long in (0, 1):
            for ufcap in sorted(ufcaps):
                for Nb in (4 * N, 2 * N + int(rng.integers(0, 2 * N + 1))):
                    S = min(ufcap - 1, 16 * N + 100)
                    assert lib.isingmc_plan_cluster_lds(N, nwords, Nb, has_long, ufcap, S, out) == 0
                    assert lib.isingmc_plan_cluster_queue(N, nwords, Nb, has_long, ufcap, q) == 0
                    (o_tab, o_state, o_touch, o_misc, o_chn, o_chtr, o_ent, o_frozen, o_froot, o_parent, words, ok, list_cap) = [int(x) for x in out]
                    off, size, cap = [int(x) for x in q]
                    max_chunks = o_chtr - o_chn
                    ufwords = (ufcap + 31) // 32 if has_long else 0
                    parent_words = (ufcap + 1) // 2
                    assert cap == 64 and size >= CLUSTER_WAVES * (cap + 1)  # per wave: the entries and at least their count
                    # inside the launch, behind the last set-up table and in front of (or behind) everything the scan keeps live
                    assert off >= o_chtr + max_chunks and off + size <= words
                    for lo, n in ((o_tab, Nb + 1), (o_state, nwords), (o_touch, nwords), (o_misc, 16), (o_chn, max_chunks), (o_chtr, max_chunks),
                                  (o_ent, tab), (o_frozen, ufwords), (o_froot, ufwords), (o_parent, parent_words)):
                        assert off + size <= lo or lo + n <= off, (N, has_long, ufcap, Nb, lo, n, off, size)
                    # flip bits and root list reuse o_ent only: they end where the per-wave tables end
                    if ok:
                        bits = (S + 31) // 32
                        assert 2 * (o_ent + bits) + list_cap <= 2 * (o_ent + tab)
                    # the carve without the region: the launch grows by exactly its size
                    without = (Nb + 1) + 2 * nwords + 16 + 2 * max_chunks + tab + 2 * ufwords + parent_words
                    assert words == without + size, (N, has_long, ufcap, Nb, words, without, size)
                    seen += 1
    assert seen > 5000
    # bad arguments are refused like isingmc_plan_cluster_lds refuses them
    assert lib.isingmc_plan_cluster_queue(0, 1, 4, 0, 65535, q) != 0 and lib.isingmc_plan_cluster_queue(4096, 128, 4, 0, 65535, q) != 0
    assert lib.isingmc_plan_cluster_queue(64, 1, 4, 0, 65535, q) != 0
