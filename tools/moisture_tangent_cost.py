"""What the tangent of the soil-moisture output costs beside the value kernel and beside lgar_series' backward pass.
(dev tool)  usage: python tools/moisture_tangent_cost.py [columns] [backward columns] [rows]

kernel    lgar_soil_moisture_tangent on 9 lanes per column (default 100 000 columns: 900 000 lanes; the end state of a tangent
          window over `rows` rows of the synth_1 storm along the nine one-hot directions of a three-layer column), with 8 and with 32
          bins, writing the [bins, lanes] tangent ("out") and contracting a cotangent into the carried gradient ("cot").  Each job
          alternates in one process with its partner, lgar_soil_moisture on the same front tables and bins (the value kernel): 20
          back-to-back bare launches per timing, device events, 2 warm-ups, the median of 7.
backward  ONE backward pass of autograd.lgar_moisture_series(every=12) with a cotangent on the moisture, against lgar_series'
          backward pass on the same rows and weights, alternating; the same timing.
One JSON line per result; there is no bar."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgar_py_amd as lg
import lgar_py_amd.autograd as A
from lgar_py_amd import workloads as W

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
NB = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
ROWS = int(sys.argv[3]) if len(sys.argv) > 3 else 48
G, K, EVERY = 9, 20, 12
PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
dev = torch.device("cuda:0")
KW = dict(dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64, device="cuda:0")


def job(n):
    P = W.perturbed_columns(n, seed=0)
    sc = torch.tensor(W.forcing_scale(n, seed=1000), device=dev)
    f = W.synth1_forcing()[:ROWS]
    pr = (torch.tensor(f[:, 0], device=dev)[:, None] * sc[None, :]).contiguous()
    return {k: torch.tensor(P[k], device=dev) for k in PARAMS}, pr, torch.zeros_like(pr)


def timed_pair(pairs, reps=7, warm=2):
    """[(label, fn)] alternating: every fn `warm` + `reps` times in turn; {label: stats}"""
    ms = {label: [] for label, _ in pairs}
    for i in range(warm + reps):
        for label, fn in pairs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            prep = fn("prepare")
            a.record()
            fn(prep)
            b.record()
            torch.cuda.synchronize()
            if i >= warm:
                ms[label].append(a.elapsed_time(b))
    out = {}
    for label, v in ms.items():
        v.sort()
        out[label] = {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1], "reps": reps}
    return out


# ---- the kernel beside the value kernel -------------------------------------------------------------------------------------
P, pr, pe = job(N)
rep = lambda t: t.repeat_interleave(G, dim=1)
big = lg.LgarEngine(*[rep(P[k]) for k in PARAMS], **KW)
L, M = big.L, big.N
dirs = {k: torch.zeros(L, M, dtype=torch.float64, device=dev) for k in ("alpha", "n", "ksat")}
for b in range(G):
    dirs[("alpha", "n", "ksat")[b // L]][b % L, b::G] = 1.0
_, _, st, end = big.tangent_window(dirs, pr, pe, forcing_group=G)
big.restore(end.value)  # the value kernel reads the engine's own state: the same front tables
torch.cuda.synchronize()
nf = end.value.n_fronts.clamp(0, big.front_slots)
for D in (8, 32):
    edges = torch.linspace(0.0, 200.0, D + 1, dtype=torch.float64).tolist()
    e_dev, _ = big._moisture_bins(edges, "theta")
    buf = torch.empty(D, M, dtype=torch.float64, device=dev)
    cot = torch.rand(D, M // G, dtype=torch.float64, device=dev)
    value = lambda p: None if p == "prepare" else [big._moisture_launch(e_dev, D, "theta", buf, None, None) for _ in range(K)]
    t_out = lambda p: None if p == "prepare" else [big._moisture_tangent_launch(end, e_dev, D, "theta", buf, None, G) for _ in range(K)]
    t_cot = lambda p: None if p == "prepare" else [big._moisture_tangent_launch(end, e_dev, D, "theta", None, cot, G) for _ in range(K)]
    for label, fn in (("out", t_out), ("cot", t_cot)):
        r = timed_pair([("value", value), (label, fn)])
        print(json.dumps({"mode": "kernel", "job": label, "lanes": M, "bins": D, "dtype": "float64", "rows": ROWS,
                          "mean_n_fronts": float(nf.float().mean()), "faulted_lanes": int((st != 0).sum()),
                          "value_us_per_launch": 1e3 * r["value"]["ms_median"] / K, "tangent_us_per_launch": 1e3 * r[label]["ms_median"] / K,
                          "ratio": r[label]["ms_median"] / r["value"]["ms_median"], "stats": r}), flush=True)
del big, end, dirs, buf, cot
torch.cuda.empty_cache()

# ---- one backward pass beside lgar_series' --------------------------------------------------------------------------------
P, pr, pe = job(NB)
edges = torch.linspace(0.0, 200.0, 9, dtype=torch.float64).tolist()
w = torch.rand(ROWS, NB, dtype=torch.float64, device=dev)
wm = torch.rand(ROWS // EVERY, 8, NB, dtype=torch.float64, device=dev)


def leaves():
    return [P[k].clone().requires_grad_(k in ("alpha", "n", "ksat")) for k in PARAMS]


def series(p):
    if p == "prepare":
        ro, pc = A.lgar_series(*leaves(), pr, pe, check=False, **KW)
        return (w * ro).sum() + (w * pc).sum()
    p.backward()


def moisture(p):
    if p == "prepare":
        ro, pc, mo = A.lgar_moisture_series(*leaves(), pr, pe, EVERY, edges=edges, what="theta", check=False, **KW)
        return (w * ro).sum() + (w * pc).sum() + (wm * mo).sum()
    p.backward()


r = timed_pair([("lgar_series", series), ("lgar_moisture_series", moisture)])
print(json.dumps({"mode": "backward", "columns": NB, "rows": ROWS, "every": EVERY, "bins": 8, "dtype": "float64",
                  "series_ms": r["lgar_series"]["ms_median"], "moisture_series_ms": r["lgar_moisture_series"]["ms_median"],
                  "ratio": r["lgar_moisture_series"]["ms_median"] / r["lgar_series"]["ms_median"], "stats": r}), flush=True)
