"""world_size-2 worker for tests/test_gpu_tempering_two_ranks.py: both ranks on GPU 0, each owns half of the temperatures of the
case it is given as JSON (model, betas, K, flags, capacity, ... and, with per-slot Hamiltonians, J / gamma / h rows for all slots, of
which a rank passes its own); the neighbour exchange runs through the host-staged transport (torch.distributed gloo)."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _pt_cases as pc  # noqa: E402
import isingmontecarlo_amd as im  # noqa: E402


def main():
    out, c = sys.argv[1], json.loads(sys.argv[2])
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    betas, K, cap = np.array(c["betas"]), c["K"], c["capacity"]
    per = len(betas) // world * K
    mine = slice(rank * per, (rank + 1) * per)
    kw, gamma, h = {}, c["gamma"], c["h"]
    if c.get("J") is not None:
        kw = dict(couplings=np.array(c["J"])[mine], transverse_r=np.array(c["gamma_r"])[mine], longitudinal_r=np.array(c["h_r"])[mine])
        gamma, h = 1.0, 0.1
    g = im.QmcIsingGraph(pc.edges_of(c), gamma, h, c["cutoff"], c["seed"], nreplicas=per, capacity=cap, replica_offset=rank * per, device=0, **kw)
    tc = im.NativeTemperingContainer(g, betas, K, c["seed"], flags=c["flags"])
    assert not tc.device_decisions
    for _ in range(c["steps"]):
        tc.timesteps(c["sweeps"])
        tc.tempering_step()
    swaps, ok = tc.get_total_swaps(), tc.verify()
    ops = np.zeros((per, cap), dtype=np.uint32)
    for r in range(per):
        w = g.export_ops(r)
        ops[r, :len(w)] = w
    np.savez(out + f".rank{rank}.npz", swaps=swaps, ok=ok, slot_of=tc.slot_of, config_of=tc.config_of, n=g.get_n(), cutoff=g.get_cutoff(),
             epoch=g.get_epoch(), state=g.state_ref(), ops=ops, acc=g.accumulators(), offsets=g.get_offsets())
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
