"""Two ranks on one GPU, three temperatures each, through the host-staged transport: configurations of several state words and many
256-slot chunks change ranks (pack / unpack kernels at real string lengths), and per-slot Hamiltonians with two chains exchange their
boundary rows at create and their relative weights at every boundary decision.  Reference and cases as in
test_gpu_tempering_edges.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _pt_cases as pc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_two_ranks(c, port, out):
    ref, hams = pc.reference(c)
    pc.check_preconditions(c)  # every pair swaps, the pair across the rank boundary at least 3 times
    job = dict(c)
    if hams is not None:
        job.update(J=hams.J.tolist(), gamma_r=hams.gamma.tolist(), h_r=hams.h.tolist())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, "_pt_native_case_worker.py"), out, json.dumps(job)]
    subprocess.check_call(cmd, env=env, cwd=os.path.dirname(HERE), timeout=240)
    T, K = len(c["betas"]), c["K"]
    tper, moved = T // 2, 0
    for rank in range(2):
        z = np.load(out + f".rank{rank}.npz")
        assert bool(z["ok"]) and int(z["swaps"]) == ref.swaps
        per = len(z["n"])
        assert per == tper * K and sorted(z["slot_of"].tolist()) == list(range(rank * per, (rank + 1) * per))  # a rank only ever holds its own temperatures
        for r in range(per):
            s = int(z["slot_of"][r])
            t, k = divmod(s, K)
            rep = ref.by_slot[k][t]
            w = f"{c['name']} rank {rank} replica {r} at slot (t={t}, k={k})"
            assert int(z["config_of"][r]) == int(ref.ids[s]), w
            assert int(z["n"][r]) == rep.n and int(z["cutoff"][r]) == rep.cutoff and int(z["epoch"][r]) == rep.epoch, w
            assert np.array_equal(z["state"][r], rep.state()), w
            assert np.array_equal(z["ops"][r][:rep.cutoff], rep.ops()) and not z["ops"][r][rep.cutoff:].any(), w
            moved += int(z["config_of"][r]) // per != rank  # configuration that started on the other rank
            if hams is not None:
                assert abs(z["offsets"][r] - hams.offset(s)) < 1e-12, w
        rows = slice(rank * per, (rank + 1) * per)
        assert z["acc"].shape == ref.acc.shape and np.array_equal(z["acc"][rows, :7], ref.acc[rows, :7]), f"{c['name']} rank {rank}: accumulator rows"
    assert moved > 0
    return ref


@pytest.mark.timeout(300)
def test_two_ranks_exchange_long_multiword_configurations(oracle, tmp_path):
    """16 x 16, two chains: eight state words, cutoffs of several thousand slots (more than seven 256-slot chunks) through pack, the
    transport and unpack."""
    c = pc.BY_NAME["ferro16x16_two_ranks"]
    ref = run_two_ranks(c, 29551, str(tmp_path / "pt"))
    assert max(r.cutoff for chain in ref.by_slot for r in chain) > 7 * 256


@pytest.mark.timeout(300)
def test_two_ranks_with_different_hamiltonians(oracle, tmp_path):
    """40-site ring, J, Gamma and h per slot, K = 2: the neighbours' boundary Hamiltonian rows travel at create, the relative weights
    cross the boundary with every decision, and the bond counts are taken again after a boundary swap of the first phase."""
    run_two_ranks(pc.BY_NAME["ring40_hams_two_ranks"], 29552, str(tmp_path / "pt"))
