#!/usr/bin/env python3
"""Exact values for the imaginary-time estimators (QmcIsingGraph.itime_average / itime_susceptibility): for a product of spins
O_g = prod_{v in g} sz_v of the Hamiltonian of make_ed_golden.py, from the full spectrum H |m> = E_m |m>,

    <O_g>  = (1/Z) sum_m exp(-beta E_m) <m|O_g|m>
    chi_g  = int_0^beta <O_g(tau) O_g(0)> dtau
           = (1/Z) sum_{m,n} |<m|O_g|n>|^2 K(E_m, E_n),   K = (exp(-beta E_n) - exp(-beta E_m)) / (E_m - E_n),  beta exp(-beta E_m) if equal

(the Kubo susceptibility; O_g(tau) = exp(tau H) O_g exp(-tau H)).

Run:  python tests/golden/make_ed_itime.py   (writes tests/golden/ed_itime.json)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_ed_golden import CASES, hamiltonian  # noqa: E402

POINTS = [("ring8_fm", 1.0), ("ring6_fm_long", 2.0)]
GROUPS = [[0], [0, 1], [0, 4], [0, 3], [0, 1, 2]]


def kubo(evals, evecs, diag_op, beta):
    """<O> and chi for an operator diagonal in the sz basis."""
    e = evals - evals.min()
    w = np.exp(-beta * e)
    z = w.sum()
    o = evecs.T @ (diag_op[:, None] * evecs)  # <m|O|n>
    de = e[:, None] - e[None, :]
    same = np.abs(de) < 1e-9
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(same, beta * w[:, None], (w[None, :] - w[:, None]) / np.where(same, 1.0, de))
    return float((w * np.diag(o)).sum() / z), float((o * o * k).sum() / z)


def main():
    cases = {c["name"]: c for c in CASES}
    out = []
    for name, beta in POINTS:
        c = cases[name]
        hmat, sz = hamiltonian(c["n"], c["edges"], c["gamma"], c["h"])
        evals, evecs = np.linalg.eigh(hmat)
        w = np.exp(-beta * (evals - evals.min()))
        rec = dict(name=name, beta=beta, energy=float((w * evals).sum() / w.sum()), groups=[])
        for g in GROUPS:
            op = np.prod(sz[g], axis=0)
            mean, chi = kubo(evals, evecs, op, beta)
            rec["groups"].append(dict(vars=g, mean=mean, chi=chi))
        out.append(rec)
        print(name, beta, [(g["vars"], round(g["mean"], 6), round(g["chi"], 6)) for g in rec["groups"]])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ed_itime.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
