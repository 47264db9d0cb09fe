"""What the catchment sums cost on the bench job (synth_1 ensemble, perturbed columns): lgar_catchment_sums over the 144 stored
runoff rows of 1 048 576 fp32 columns.
(dev tool)  usage: python tools/catchment_cost.py [f32|f64] [N]

Cases: B = 1, 64, 4096 and 65 536 catchments of equal size, contiguous (order = None: lane-contiguous reads), and B = 4096 under
a random permutation of the columns (order array: a gather).  Per case: device-event time of one CatchmentMap.sums() call with
the engine's status and random weights (median of 7 after 2 warm-up calls; the 0.6 GB series does not fit the 256 MB last-level
cache, so every call streams it from HBM) and GB/s on the algorithmic bytes -- the series read once, plus weights, status and
the order array once each.

The yardstick, in the same run: the existing basin pass (lgar_basin_reduce_kernel, one 1024-thread workgroup per row) over the
SAME series buffer.  It has no entry point of its own -- lgar_forward launches it after the forward kernels -- so it is timed as
the difference between forward(series=("runoff",), basin=("runoff",)) and forward(series=("runoff",)), alternating, on a dry
forcing (no rain: the forward kernels have next to nothing to do, so the difference of the two medians is the pass itself; both
passes are plain fp64 adds whose time does not depend on the values).  This runs last: it overwrites the buffer.
One JSON line per result."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgar_py_amd as lg
from lgar_py_amd import workloads as W
from lgar_py_amd.catchments import CatchmentMap

dt = torch.float32 if (sys.argv[1] if len(sys.argv) > 1 else "f32") == "f32" else torch.float64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
P = W.perturbed_columns(N, seed=0)
sc = torch.tensor(W.forcing_scale(N, seed=1000), device="cuda")
f = W.synth1_forcing()
eng = lg.LgarEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], dt_h=300.0 / 3600.0,
                    ponded_depth_max=0.0, dtype=dt)
pr = (torch.tensor(f[:, 0], device="cuda")[:, None] * sc[None, :]).to(dt).contiguous()
pe = torch.zeros_like(pr)
T = pr.shape[0]
runoff = torch.empty_like(pr)
eng.forward(pr, pe, series=("runoff",), out={"runoff": runoff}, check=False)
torch.cuda.synchronize()
es = runoff.element_size()
rng = np.random.default_rng(0)
w = rng.random(N)


def timed(fn, reps=7, warm=2):
    us = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            us.append(1e3 * a.elapsed_time(b))
    us.sort()
    return us


perm = rng.permutation(N)
for B, permuted in ((1, False), (64, False), (4096, False), (65536, False), (4096, True)):
    if B > N:
        continue
    ids = (np.arange(N, dtype=np.int64) * B) // N
    cmap = CatchmentMap(ids[perm] if permuted else ids, n_catchments=B, weights=w)
    buf = torch.empty(T, B, dtype=torch.float64, device="cuda")
    us = timed(lambda: cmap.sums(runoff, status=eng.status, out=buf))
    nbytes = T * N * es + N * es + 4 * N + (0 if cmap.order is None else 4 * N)
    med = us[len(us) // 2]
    print(json.dumps({"mode": "catchment_sums", "N": N, "T": T, "dtype": str(dt), "B": B, "permuted": permuted,
                      "gather": cmap.order is not None, "us_median": med, "us_min": us[0], "us_max": us[-1], "reps": len(us),
                      "algorithmic_bytes": nbytes, "GBps": nbytes / (med * 1e-6) / 1e9,
                      "faulted_columns": int(((eng.status & 0x7F) != 0).sum())}), flush=True)

# the yardstick: the basin pass over the same buffer, as the difference of two dry forward() calls
dry = torch.zeros_like(pr)
wt = torch.tensor(w, device="cuda").to(dt)
out = {"runoff": runoff}


def forward(basin):
    eng.reset()
    eng.forward(dry, pe, series=("runoff",), out=out, check=False, basin=basin, weights=wt if basin else None)


plain, with_basin = [], []
for r in range(3):
    plain += timed(lambda: forward(()), reps=5, warm=1 if r else 2)
    with_basin += timed(lambda: forward(("runoff",)), reps=5, warm=1 if r else 2)
plain.sort()
with_basin.sort()
us = with_basin[len(with_basin) // 2] - plain[len(plain) // 2]
nbytes = T * N * es + N * es
print(json.dumps({"mode": "basin_pass_yardstick", "N": N, "T": T, "dtype": str(dt), "us_forward_dry_median": plain[len(plain) // 2],
                  "us_forward_dry_with_basin_median": with_basin[len(with_basin) // 2], "us_basin_pass": us,
                  "us_spread_of_forward_dry": plain[-1] - plain[0], "reps": len(plain), "algorithmic_bytes": nbytes,
                  "GBps": nbytes / (us * 1e-6) / 1e9 if us > 0 else None}), flush=True)
