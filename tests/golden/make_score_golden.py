#!/usr/bin/env python
"""Record the reference's own scores of the committed trajectory fixtures (tests/golden/scores/reference_scores.npz).

Runs ONLY in the build container (needs /root/reference, imported the way make_golden.py does: its _refstub path); the
reference never travels and nothing of it is copied.  What is recorded is what its two scoring functions RETURN --
dpLGAR/data/metrics.py calculate_nse(modeled, observed) and dpLGAR/models/functions/loss.py MSE_loss(modeled, observed) -- for
every committed trajectory fixture with at least 100 completed rows and some runoff: modeled = the recorded giuh_runoff column,
observed = the recorded runoff column, after a warm-up of 0 and of 24 rows (the agent's y_hat_[warmup:]).  Names and scalars
only, a few KB.  The subdirectory keeps the file out of conftest.golden_names(), which lists the top level.

Usage:  python tests/golden/make_score_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "_refstub"))
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import numpy as np
import torch

from dpLGAR.data.metrics import calculate_nse
from dpLGAR.models.functions.loss import MSE_loss

RUNOFF, GIUH_RUNOFF = 4, 6  # columns of the recorded accumulators (ACC_NAMES)
MIN_ROWS, WARMUPS = 100, (0, 24)


def main():
    names, warmups, nse, mse, rows = [], [], [], [], []
    for f in sorted(os.listdir(HERE)):
        if not f.endswith(".npz") or f.startswith("grad_") or f == "leaf_kats.npz":
            continue
        g = np.load(os.path.join(HERE, f))
        if "acc" not in g.files:
            continue
        crash = int(g["crash_step"])
        T = crash if crash >= 0 else g["forcing"].shape[0]
        if T < MIN_ROWS or not float(g["acc"][:T, RUNOFF].max()) > 0:
            continue
        for w in WARMUPS:
            modeled, observed = g["acc"][w:T, GIUH_RUNOFF].astype(np.float64), g["acc"][w:T, RUNOFF].astype(np.float64)
            with np.errstate(all="ignore"):
                names.append(f[:-4])
                warmups.append(w)
                rows.append(T)
                nse.append(float(calculate_nse(modeled, observed)))
                mse.append(float(MSE_loss(torch.from_numpy(modeled), torch.from_numpy(observed))))
    out = os.path.join(HERE, "scores")
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, "reference_scores.npz"), name=np.array(names), warmup=np.array(warmups, dtype=np.int32),
             rows=np.array(rows, dtype=np.int32), nse=np.array(nse), mse=np.array(mse))
    for nm, w, a, b in zip(names, warmups, nse, mse):
        print("%-40s warmup %2d  NSE %.10f  MSE %.6e" % (nm, w, a, b))


if __name__ == "__main__":
    main()
