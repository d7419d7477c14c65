"""Generates tests/golden/oscillator_outcomes_n12.npz: the oracle's PTR homotopy of the oscillator with actuator deadband
(oracle/ptr_ref.py::homotopy: the numpy-dynamics model of oracle/models.py through oracle/discretize_ref.py).

  * five Monte-Carlo instances pp = (r0, v0) at N = 12, Nsub = 10, three stages kappa1 = Homotopy(1e-8)(0, 1/2, 1), reference
    parameters of oscillator/tests.jl:24-57.  Per instance and stage: the reference trajectory of the stage's FIRST subproblem
    (the guess, then the previous stage's solution), that subproblem's optimal J_aug, and the stage's status (0 = SCP_SOLVED),
    iteration count and final J;
  * the nominal instance on the reference's own grid N = 30 with its ten stages: status, iterations, J per stage.

    python tests/golden/make_oscillator_outcomes.py          (from the repository root; ~15 s)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)

from oracle import models, ptr_ref  # noqa: E402

OUT = os.path.join(HERE, "oscillator_outcomes_n12.npz")
N12, NSUB = 12, 10


def compute():
    B, S = len(models.INSTANCES), len(models.KAPPA3)
    d = dict(pp=models.INSTANCES.copy(), kappa=np.array(models.KAPPA3), N=np.array(N12), Nsub=np.array(NSUB),
             ref_x=np.zeros((B, S, N12, 2)), ref_u=np.zeros((B, S, N12, 4)), ref_p=np.zeros((B, S, N12)), J_aug_first=np.zeros((B, S)),
             status=np.zeros((B, S), np.int32), iterations=np.zeros((B, S), np.int32), J=np.zeros((B, S)))
    for b, pp in enumerate(models.INSTANCES):
        for s, (st, hist) in enumerate(ptr_ref.homotopy(N12, NSUB, models.KAPPA3, pp)):
            first = hist[0]
            d["ref_x"][b, s], d["ref_u"][b, s], d["ref_p"][b, s] = first["ref"].xd, first["ref"].ud, first["ref"].p
            d["J_aug_first"][b, s] = first["sub"]["J_aug"]
            d["status"][b, s] = 0 if st == "SCP_SOLVED" else 1
            d["iterations"][b, s] = len(hist)
            d["J"][b, s] = hist[-1]["sub"]["J"]
    run = ptr_ref.homotopy(30, NSUB, models.KAPPA10, models.INSTANCES[2])
    d["kappa30"] = np.array(models.KAPPA10)
    d["status30"] = np.array([0 if st == "SCP_SOLVED" else 1 for st, _ in run], np.int32)
    d["iterations30"] = np.array([len(h) for _, h in run], np.int32)
    d["J30"] = np.array([h[-1]["sub"]["J"] for _, h in run])
    return d


if __name__ == "__main__":
    d = compute()
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    print("N = 12: status", d["status"].tolist(), "iterations", d["iterations"].tolist())
    print("N = 30: status", d["status30"].tolist(), "iterations", d["iterations30"].tolist(), "J", d["J30"][-1])
