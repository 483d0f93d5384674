"""Every reader of the deferred cluster flips (DevBatch::flipb: the bytes the dedicated cluster kernel leaves instead of rewriting
the op-strings), bit-exact against the CPU oracle, whatever the layout of the bytes.

Three users share the layout: the cluster kernel's deferred apply loop writes it, the trimmed diagonal kernel of the next
timestep applies the bytes while it streams the strings, and materialize_kernel applies them for every other reader.  A batch
that stops after every timestep and exports its strings takes the third way each time; its twin runs all timesteps in one call
and takes the second; both must give the oracle's strings.
  * shapes (4x4 ferromagnet; tile = 64 * slots per lane): last tiles of 1, 64 and 255 slots with everything in wave 0 (capacity
    2^18), the same with two slots per lane, many waves with two tiles each (capacity 2^13, chunks of 256 slots), and a cutoff
    that grows across a tile and across a wave's range between two sweeps, so that the diagonal pass reads bytes beyond the
    cutoff of the sweep before.  Each asserts the cutoffs and tiles it relies on from the oracle's run;
  * other consumers behind a cluster update with pending bytes: one RVB sweep, a directed-loop-only call, and an export /
    import round trip followed by more timesteps."""
import numpy as np
import pytest

import _lattices as lat
from test_gpu_parity import assert_same, make_pair
from test_gpu_trim_paths import chunk_size, tiles_per_wave

pytestmark = pytest.mark.gpu

STEPS, R, SEED, FLAG_LOOP = 12, 2, 4711, 1  # (a directed loop in every timestep, as in test_gpu_trim_paths.py, whose cutoffs these are)

# name: starting cutoff, beta, slots per lane (0: default = 4), capacity, tiles per cluster wave at the end (None: growing), slots in the last tile
SHAPES = {
    "last_1": (3 * 256 + 1, 4.0, 0, 1 << 18, [4], 1),
    "last_64": (5 * 256 + 64, 8.0, 0, 1 << 18, [6], 64),
    "last_255": (6 * 256 + 255, 12.0, 0, 1 << 18, [7], 255),
    "last_64_k2": (5 * 256 + 64, 8.0, 2, 1 << 18, [11], 64),
    "two_tiles_per_wave": (20 * 256 + 1, 32.0, 0, 1 << 13, [2] * 10 + [1], 1),
    "growing": (16, 8.0, 0, 1 << 13, None, None),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_bytes_through_materialise_and_through_the_diagonal_pass(oracle, name):
    cut0, beta, k, cap, tiles, last_slots = SHAPES[name]
    edges = lat.two_d_ferro(4)
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, cut0, cap, SEED, R, k=k)
    twin, _, _ = make_pair(oracle, edges, 1.0, 0.0, cut0, cap, SEED, R, k=k)
    ch = chunk_size(cap, k or 4)
    cutoffs = []
    for step in range(STEPS):
        oracle.batch_timesteps(reps, 1, [beta] * R, 1, FLAG_LOOP)
        cutoffs.append([rep.cutoff for rep in reps])
        g.run(1, beta, flags=FLAG_LOOP)
        assert_same(g, reps, f"{name} step {step}")  # (export_ops: the pending bytes go through materialize_kernel)
    cutoffs = np.array(cutoffs)
    if tiles is None:  # a tile, then a wave's range, that did not exist the sweep before
        assert (cutoffs[4] < 256).all() and (cutoffs[-1] > 256).all() and cutoffs[-1].max() > 512, cutoffs
        assert (np.diff(cutoffs[:, 0]) > 0).all(), cutoffs[:, 0]
        assert tiles_per_wave(int(cutoffs[0, 0]), ch, k or 4)[0] == [1] and tiles_per_wave(int(cutoffs[-1, 0]), ch, k or 4)[0] == [1, 1, 1]
    else:
        assert (cutoffs == cut0).all(), cutoffs
        assert tiles_per_wave(cut0, ch, k or 4) == (tiles, last_slots)
    info = g.launch_info()
    assert info["lean_cluster"] and info["fast_diagonal"] and info["slots_per_lane"] == (k or 4), info
    twin.run(STEPS, beta, flags=FLAG_LOOP)  # (one call: every sweep's bytes are applied by the diagonal pass of the next)
    assert_same(twin, reps, f"{name} in one call")
    assert g.verify().all() and twin.verify().all()


@pytest.mark.parametrize("consumer", ["rvb", "loop", "export_import"])
def test_other_consumers_behind_a_cluster_update(oracle, consumer):
    edges, beta, cap = lat.two_d_ferro(4), 4.0, 1 << 13
    g, m, reps = make_pair(oracle, edges, 1.0, 0.0, 64, cap, SEED, R)
    g.run(6, beta)  # ends with a cluster update: its flip bytes are pending
    oracle.batch_timesteps(reps, 6, [beta] * R, 1, 0)
    assert g.launch_info()["lean_cluster"]
    assert all(rep.n > 64 for rep in reps), [rep.n for rep in reps]
    if consumer == "rvb":
        succ, upd = g.single_rvb_sweep()
        for r, rep in enumerate(reps):
            assert succ[r] == rep.rvb_update(upd), f"RVB successes differ r={r}"
    elif consumer == "loop":
        lens = g.loop_update()
        for r, rep in enumerate(reps):
            assert lens[r] == rep.loop_update(), f"loop length differs r={r}"
    else:
        for r, rep in enumerate(reps):
            words = g.export_ops(r)
            assert np.array_equal(words, rep.ops())
            g.import_ops(words, r)
    assert_same(g, reps, consumer)
    g.run(4, beta)
    oracle.batch_timesteps(reps, 4, [beta] * R, 1, 0)
    assert_same(g, reps, consumer + ", then four timesteps")
    assert g.verify().all()
