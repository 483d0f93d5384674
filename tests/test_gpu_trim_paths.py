"""The trimmed diagonal kernel's tile loop (csrc/sse_fast.hip.h) and the deferred apply loop of the dedicated cluster kernel
(csrc/sse_cluster.hip.h) at the smallest shapes where their tile handling can go wrong, bit-exact against the CPU oracle.

Model: the 4x4 periodic ferromagnet, 4 replicas, 12 whole timesteps with a directed loop, deferred flips on (the default).

The diagonal kernel runs 4 waves per replica on tiles of 4 * 64 * K slots.  The cluster kernel runs 16 waves; wave w scans
ceil(used / 16) chunks of CH slots (used = chunks the cutoff M reaches, CH from isingmc_plan_geometry) in tiles of 64 * K slots,
and its deferred apply loop is unrolled over a prefetch queue of three tiles: it leaves behind the first, second or third tile of
an iteration.  So a case is a cutoff M AND a capacity (which sets CH); starting cutoff and beta were found with the oracle, and
each case asserts the cutoffs and the tiles per cluster wave it relies on (tiles_per_wave below restates the kernel's split), so
neither a change of the growth rule nor one of the chunk grid can quietly empty it:
  * capacity 2^13, CH = 256: every wave has at most two tiles.  M below 256 and growing every sweep (one partial tile, pending
    flip bytes beyond the cutoff of the sweep before); M growing from 16 across 256 and 512 (a tile, and a wave's range, that did
    not exist the sweep before); M = 20 * 256 + 1: eleven waves, two tiles in all but the last;
  * capacity 2^18, CH = 2048: wave 0 holds the whole string, the other fifteen ranges are empty.  M fixed at 3 * 256 + 1,
    5 * 256 + 64, 6 * 256 + 255 and 7 * 256 + 255: 4, 6, 7 and 8 tiles with 1, 64, 255 and 255 slots in the last, so the loop fills
    its queue, wraps, and leaves behind the first, third, first and second tile of an iteration; M growing from 16 to three tiles;
    5 * 256 + 64 again with two slots per lane (11 tiles of 128, leaving behind the second);
  * capacity 2^21 + 1024, beyond SSE_ACCEPT_MAX_DEN: the f64 rounds of the diagonal kernel (the selection rule is asserted from
    the sources: launch_info has no field for it); CH = 16640, M = 3 * 256 + 1: four tiles in wave 0.
Every case ends by reading the op-strings back (export_ops: pending flips go through the materialise kernel)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import assert_same, make_pair

pytestmark = pytest.mark.gpu

STEPS, R, SEED, FLAG_LOOP = 12, 4, 4711, 1
CLUSTER_WAVES = 16  # SSE_CLW
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "isingmontecarlo_amd", "csrc")

# name, starting cutoff, beta, slots per lane (0: default = 4), capacity, chunk size, tiles of the cluster waves that have any
# after the last sweep (None: the cutoff differs from replica to replica, see check_shape), slots in the string's last tile
CASES = [
    ("partial_tile_growing", 16, 2.0, 0, 1 << 13, 256, None, None),
    ("growing_across_waves", 16, 8.0, 0, 1 << 13, 256, None, None),
    ("two_tiles_in_each_wave", 20 * 256 + 1, 32.0, 0, 1 << 13, 256, [2] * 10 + [1], 1),
    ("four_tiles_last_1", 3 * 256 + 1, 4.0, 0, 1 << 18, 2048, [4], 1),
    ("six_tiles_last_64", 5 * 256 + 64, 8.0, 0, 1 << 18, 2048, [6], 64),
    ("seven_tiles_last_255", 6 * 256 + 255, 12.0, 0, 1 << 18, 2048, [7], 255),
    ("eight_tiles_last_255", 7 * 256 + 255, 14.0, 0, 1 << 18, 2048, [8], 255),
    ("growing_in_one_wave", 16, 8.0, 0, 1 << 18, 2048, None, None),
    ("eleven_tiles_last_64_k2", 5 * 256 + 64, 8.0, 2, 1 << 18, 2048, [11], 64),
    ("four_tiles_last_1_f64", 3 * 256 + 1, 4.0, 0, (1 << 21) + 1024, 16640, [4], 1),
]


def chunk_size(cap, k):
    import isingmontecarlo_amd as im
    out = (C.c_uint32 * 4)()
    assert im.load_library().isingmc_plan_geometry(cap, 4, k, 16, out) == 0
    return int(out[0])


def tiles_per_wave(M, ch, k):
    """Tiles of every cluster wave that has a range, and the slots in the last tile of the last of them (the split of
    cluster_kernel: used chunks, q = ceil(used / 16) chunks per wave, tiles of 64 k slots; CH is a multiple of 256)."""
    used = -(-M // ch)
    q = -(-used // CLUSTER_WAVES)
    tiles, last = [], 0
    for w in range(CLUSTER_WAVES):
        c0 = min(w * q, used)
        c1 = min(c0 + q, used)
        pbeg, pend = c0 * ch, min(c1 * ch, M)
        if pend > pbeg:
            tiles.append(-(-(pend - pbeg) // (64 * k)))
            last = (pend - pbeg) - (tiles[-1] - 1) * 64 * k
    return tiles, last


def oracle_run(oracle, reps, beta):
    """The 12 timesteps on the oracle, sweep by sweep: cutoffs[s][r] after sweep s."""
    cutoffs = []
    for _ in range(STEPS):
        oracle.batch_timesteps(reps, 1, [beta] * R, 1, FLAG_LOOP)
        cutoffs.append([rep.cutoff for rep in reps])
    return np.array(cutoffs)


def check_shape(name, cut0, cutoffs, ch, k, tiles, last_slots):
    last = cutoffs[-1]
    if name == "partial_tile_growing":
        assert (last < 256).all() and (last > 128).all(), last
        assert (np.diff(cutoffs[:, 0]) > 0).sum() >= 8, cutoffs[:, 0]  # grows in most sweeps
        assert all(tiles_per_wave(int(M), ch, k)[0] == [1] for M in cutoffs.ravel())
    elif name in ("growing_across_waves", "growing_in_one_wave"):
        assert (cutoffs[4] < 256).all() and (last > 256).all() and last.max() > 512, cutoffs
        assert (np.diff(cutoffs[:, 0]) > 0).all(), cutoffs[:, 0]  # every sweep leaves flips for slots beyond the cutoff before
        shapes = [tiles_per_wave(int(M), ch, k)[0] for M in cutoffs[:, 0]]
        # from one tile to three: in three waves (a range that was empty the sweep before) or in wave 0 alone
        assert shapes[0] == [1] and shapes[-1] == ([1, 1, 1] if name == "growing_across_waves" else [3]), shapes
    else:
        assert (cutoffs == cut0).all(), cutoffs  # fixed: the shape of the last tile is the case
        assert tiles_per_wave(cut0, ch, k) == (tiles, last_slots)


def f64_rounds_selected(cap):
    """The rule of launch_sweep_fast (csrc/sweep_fast.hip) with the constant of csrc/sse_accept.h, read from the sources."""
    with open(os.path.join(CSRC, "sweep_fast.hip")) as f:
        assert re.search(r"const bool f64 = B\.cap > SSE_ACCEPT_MAX_DEN;", f.read()), "the selection rule of the f64 rounds changed"
    with open(os.path.join(CSRC, "sse_accept.h")) as f:
        m = re.search(r"#define SSE_ACCEPT_MAX_DEN \(1u << (\d+)\)", f.read())
    assert m, "SSE_ACCEPT_MAX_DEN is no longer written as a power of two"
    return cap > (1 << int(m.group(1)))


@pytest.mark.parametrize("name,cut0,beta,k,cap,ch,tiles,last_slots", CASES, ids=[c[0] for c in CASES])
def test_trimmed_loops_at_tile_edges(oracle, name, cut0, beta, k, cap, ch, tiles, last_slots):
    g, m, reps = make_pair(oracle, lat.two_d_ferro(4), 1.0, 0.0, cut0, cap, SEED, R, k=k)  # (default wave count: an explicit one rules the dedicated cluster kernel out)
    info = g.launch_info()
    assert info["fast_diagonal"] and info["waves_per_replica"] == 4 and info["slots_per_lane"] == (k or 4), info
    assert chunk_size(cap, k or 4) == ch
    assert f64_rounds_selected(cap) == name.endswith("_f64")
    cutoffs = oracle_run(oracle, reps, beta)
    check_shape(name, cut0, cutoffs, ch, k or 4, tiles, last_slots)
    n_ref = np.array([rep.n for rep in reps])
    assert (n_ref > cutoffs[-1] // 4).all(), (n_ref, cutoffs[-1])  # the tiles hold operators, not only empty slots
    g.run(STEPS, beta, flags=FLAG_LOOP)
    assert g.launch_info()["lean_cluster"]  # (known once a timestep has been planned)
    assert_same(g, reps, name)  # (ends with export_ops of every replica: the pending flip bytes are materialised)
    acc = g.accumulators()
    for r, rep in enumerate(reps):
        assert np.array_equal(acc[r, :7], rep.accumulators()[:7]), f"{name}: accumulators differ r={r}"
    assert g.verify().all()
