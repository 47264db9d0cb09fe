"""Shapes of the front table over a run of the bench ensemble, on the device-code simulator (dev tool; no GPU):
python tools/table_shape_census.py [columns=1024]

The first `columns` columns of bench.py's first draw (workloads.perturbed_columns seed 0, forcing_scale seed 1000), fp32, stepped
one forcing row per call; the columns that never fault are kept and grouped into waves of 64 consecutive columns.  Printed: the
share of column-steps per n_fronts, the share whose table is a top-layer table (lgar_column.hpp is_top_table: m >= 1 fronts of
layer 0 that are no boundary fronts, then the layers' boundary fronts), the share whose in-layer fronts are all tagged layer 0
(m = 0 included), the same per wave-step for all 64 lanes, and the first step with an in-layer front below layer 0."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import devsim
from lgar_py_amd import workloads as W

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
P = W.perturbed_columns(N, seed=0)
sc = W.forcing_scale(N, seed=1000)
f = W.synth1_forcing()
T, L = f.shape[0], P["alpha"].shape[0]
eng = devsim.SimEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], dt_h=300.0 / 3600.0,
                       ponded_depth_max=0.0, dtype=np.float32, n_columns=N, search_mode=2)
pr = torch.tensor(f[:, 0:1] * sc[None, :])
nfs, tops, tagged0 = [], [], []
for t in range(T):
    eng.forward(pr[t:t + 1], torch.zeros_like(pr[t:t + 1]), series=("runoff",))
    fl, nf = eng.flags.numpy().astype(np.int64), eng.n_fronts.numpy().astype(np.int64)
    i = np.arange(fl.shape[0])[:, None]
    m = nf[None, :] - L
    want = np.where(i < m, 0, (i - m) | 0x80)
    live = i < nf[None, :]
    tops.append((m[0] >= 1) & np.where(live, fl == want, True).all(axis=0))
    tagged0.append(~(live & ((fl & 0x80) == 0) & ((fl & 0x7f) > 0)).any(axis=0))
    nfs.append(nf.copy())
keep = eng.status.numpy() == 0
keep[np.flatnonzero(keep)[(int(keep.sum()) // 64) * 64:]] = False  # whole waves only
nfs, tops, tagged0 = (np.stack(a)[:, keep] for a in (nfs, tops, tagged0))
waves = nfs.shape[1] // 64
per_wave = lambda a: a.reshape(T, waves, 64).all(axis=2)
off_steps = np.flatnonzero(~tagged0.all(axis=1))
print(json.dumps({
    "columns_kept": int(nfs.shape[1]), "waves": waves, "wave_steps": T * waves,
    "n_fronts_share": {int(k): round(float((nfs == k).mean()), 4) for k in np.unique(nfs)},
    "column_steps_top_layer_table": round(float(tops.mean()), 4),
    "column_steps_in_layer_fronts_all_layer0": round(float(tagged0.mean()), 4),
    "wave_steps_top_layer_table_all_lanes": round(float(per_wave(tops).mean()), 4),
    "wave_steps_in_layer_fronts_all_layer0_all_lanes": round(float(per_wave(tagged0).mean()), 4),
    "first_step_with_in_layer_front_below_layer0": int(off_steps[0]) if off_steps.size else None}))
