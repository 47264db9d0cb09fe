"""What the soil-moisture output costs on the bench job (synth_1 ensemble, perturbed columns, 144 steps).
(dev tool)  usage: python tools/moisture_cost.py kernel|window|forward [f32|f64] [N]

kernel   lgar_soil_moisture alone on the state after the 144 steps, 8 bins: device-event time of back-to-back launches ("hot":
         the ~100 MB working set of the 1M-column fp32 job stays in the 256 MB last-level cache) and of single launches each
         preceded by a 1 GiB fill ("cold": from HBM), against the kernel's algorithmic bytes -- the front rows a wave actually
         reads (its largest n_fronts x 64 columns x (depth + theta + flag byte)), n_fronts, the thicknesses and the output.
window   run_with_soil_moisture(every=12) against ONE forward() and against the same 12 windows without the snapshots,
         alternating, so the per-launch ramp / tail of a short forward() shows separately from the new kernel.
forward  ONE forward() only: the same measurement with another library selected through LGAR_LIB (the parent commit's).
One JSON line per result."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgar_py_amd as lg
from lgar_py_amd import workloads as W

mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
dt = torch.float32 if (sys.argv[2] if len(sys.argv) > 2 else "f32") == "f32" else torch.float64
N = int(sys.argv[3]) if len(sys.argv) > 3 else 1 << 20
EVERY = 12
P = W.perturbed_columns(N, seed=0)
sc = torch.tensor(W.forcing_scale(N, seed=1000), device="cuda")
f = W.synth1_forcing()
eng = lg.LgarEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], dt_h=300.0 / 3600.0,
                    ponded_depth_max=0.0, dtype=dt)
pr = (torch.tensor(f[:, 0], device="cuda")[:, None] * sc[None, :]).to(dt).contiguous()
pe = torch.zeros_like(pr)
T = pr.shape[0]
SERIES = ("runoff", "percolation")
out = {k: torch.empty_like(pr) for k in SERIES}


def timed(fn, reps, warm=1):
    ms = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    ms.sort()
    return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "reps": reps}


def single():
    eng.reset()
    eng.forward(pr, pe, series=SERIES, out=out, check=False)


def chunked():
    eng.reset()
    for lo in range(0, T, EVERY):
        eng.forward(pr[lo:lo + EVERY], pe[lo:lo + EVERY], series=SERIES, out={k: out[k][lo:lo + EVERY] for k in SERIES}, check=False)


def windowed():
    eng.reset()
    eng.run_with_soil_moisture(pr, pe, EVERY, edges=EDGES, what="theta", series=SERIES, check=False)


EDGES = [0.0, 5.0, 10.0, 20.0, 40.0, 60.0, 100.0, 150.0, 200.0]  # 8 bins over the 200 cm column
if mode == "forward":
    print(json.dumps(dict(timed(single, 7), mode="single_forward", lib=os.environ.get("LGAR_LIB", "in-tree"), N=N)), flush=True)
elif mode == "window":
    for label, fn in (("single_forward", single), ("twelve_windows_no_snapshot", chunked), ("run_with_soil_moisture", windowed)) * 2:
        print(json.dumps(dict(timed(fn, 5), mode=label, N=N, windows=T // EVERY)), flush=True)
else:
    single()
    torch.cuda.synchronize()
    nf = eng.n_fronts.clamp(0, eng.front_slots)
    pad = (-N) % 64
    rows = torch.cat([nf, nf.new_zeros(pad)]).view(-1, 64).max(dim=1).values.sum().item()  # front rows read, summed over waves
    es = eng.totals.element_size()
    D = len(EDGES) - 1
    parts = {"front_rows": rows * 64 * (2 * es + 1), "n_fronts": 4 * N, "thickness": eng.L * N * es, "output": D * N * es}
    total = sum(parts.values())
    buf = torch.empty(D, N, dtype=dt, device="cuda")
    K = 50
    hot = timed(lambda: [eng.soil_moisture(EDGES, "theta", out=buf) for _ in range(K)], 7, warm=2)
    e_dev, _ = eng._moisture_bins(EDGES, "theta")  # (the bare launch: the edges are validated and uploaded once)
    bare = timed(lambda: [eng._moisture_launch(e_dev, D, "theta", buf, None, None) for _ in range(K)], 7, warm=2)
    fill = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB: four times the last-level cache
    cold = []
    for i in range(12):
        fill.fill_(float(i))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng._moisture_launch(e_dev, D, "theta", buf, None, None)
        b.record()
        torch.cuda.synchronize()
        cold.append(a.elapsed_time(b))
    cold = sorted(cold[2:])
    lay = timed(lambda: [eng.soil_moisture(None, "storage") for _ in range(K)], 5, warm=1)
    rec = {"mode": "kernel", "N": N, "dtype": str(dt), "bins": D, "mean_n_fronts": float(nf.float().mean()),
           "mean_rows_per_wave": rows / ((N + 63) // 64), "algorithmic_bytes": total, "bytes": parts,
           "hot_us_per_call_with_wrapper": 1e3 * hot["ms_median"] / K, "hot_us_per_launch": 1e3 * bare["ms_median"] / K,
           "hot_TBps": total / (bare["ms_median"] / K * 1e-3) / 1e12,
           "cold_us_median": 1e3 * cold[len(cold) // 2], "cold_us_min": 1e3 * cold[0],
           "cold_TBps": total / (cold[len(cold) // 2] * 1e-3) / 1e12,
           "layer_bins_us_per_call_with_wrapper": 1e3 * lay["ms_median"] / K, "faulted": int((eng.status != 0).sum())}
    print(json.dumps(rec), flush=True)
