"""What a backward pass over a window that starts from a spun-up state costs, against what a user had to do before
(lgar_forward_tangent_window).
(dev tool)  usage: python tools/window_cost.py [N] [--out FILE]      (FILE: profiles/r12/window_cost.jsonl by default)

Job: N = 100 000 perturbed columns (workloads.perturbed_columns, per-column forcing scale), 3 layers, the 9 one-hot directions
over (alpha, n, Ksat) x layer side by side (autograd.parameter_vjp: 9 N columns of one launch, the lanes of a column sharing the
trapezoid), fp64, 432 rows of the synth_1 storm (three times over), of which the last 144 are the window.  The incoming
gradient is a ramp on the runoff.
  (a) window:      parameter_vjp(start=snapshot after 288 rows) over the last 144 rows;
  (b) fresh_full:  parameter_vjp over all 432 rows with zero weights on the first 288 -- what a user had to do before;
  (c) fresh_144:   parameter_vjp from a fresh state over 144 rows -- the same kernels without loading a state;
  (d) fresh_288:   parameter_vjp from a fresh state over the first 288 rows: (b) - (d) is what the window's own rows cost inside
                   the fresh run -- the same rows from the same state, which (c) is not (a dry column holds fewer fronts).
Device-event time of one call each, the four alternating in one process, 2 warm-ups, median of 7.  Reported: (a) / (b) as
measured, and the condition in the form of sections 12 - 15: (a) is not above (c) by more than (c)'s own max - min.  (a) and (c)
integrate different rows of different states, so the condition prices the load of the state, not the physics.  One JSON line
per result."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgar_py_amd as lg
from lgar_py_amd import workloads as W
from lgar_py_amd.autograd import parameter_vjp

args = sys.argv[1:]
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "r12", "window_cost.jsonl")
N = int(args[0]) if args and args[0].isdigit() else 100_000
REPS, WARM, SPIN, WIN = 7, 2, 288, 144
PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")

Pn = W.perturbed_columns(N, seed=0)
sc = W.forcing_scale(N, seed=1)
f = W.synth1_forcing(3)
pr = torch.tensor(f[:, 0:1] * sc[None, :], device="cuda")
pe = torch.zeros_like(pr)
T = pr.shape[0]
assert T == SPIN + WIN
eng = lg.LgarEngine(*[Pn[k] for k in PARAMS], dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64)
eng.forward(pr[:SPIN], pe[:SPIN], series=(), check=False)
snap = eng.snapshot()
w = torch.zeros(T, N, dtype=torch.float64, device="cuda")
w[SPIN:] = torch.linspace(0.5, 1.5, WIN, device="cuda", dtype=torch.float64)[:, None]
prw, pew, ww = pr[SPIN:].contiguous(), pe[SPIN:].contiguous(), w[SPIN:].contiguous()
wanted = [(kind, l) for kind in ("alpha", "n", "ksat") for l in range(3)]
jobs = {"window": lambda: parameter_vjp(eng, prw, pew, ww, None, wanted, check=False, start=snap),
        "fresh_full": lambda: parameter_vjp(eng, pr, pe, w, None, wanted, check=False),
        "fresh_144": lambda: parameter_vjp(eng, prw, pew, ww, None, wanted, check=False),
        "fresh_288": lambda: parameter_vjp(eng, pr[:SPIN], pe[:SPIN], w[:SPIN], None, wanted, check=False)}
us = {nm: [] for nm in jobs}
for i in range(WARM + REPS):
    for nm, fn in jobs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            us[nm].append(1e3 * a.elapsed_time(b))
# the window and the zero-weighted full run are the same gradient up to the spin-up's own sensitivity, which the window drops:
# reported, not asserted (tests/test_gpu_tangent_window.py holds the window to the forward's own differences)
gw, stw = jobs["window"]()
gf, stf = jobs["fresh_full"]()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
med = {nm: sorted(v)[len(v) // 2] for nm, v in us.items()}
with open(OUT, "a") as fh:
    for nm, v in us.items():
        v = sorted(v)
        rec = {"mode": "window_cost", "job": nm, "columns": N, "directions": len(wanted), "rows": {"fresh_full": T, "fresh_288": SPIN}.get(nm, WIN),
               "us_median": med[nm], "us_min": v[0], "us_max": v[-1], "reps": REPS, "library": os.environ.get("LGAR_LIB", "default")}
        if nm == "window":
            c = sorted(us["fresh_144"])
            state_bytes = (5 * eng.front_slots + lg._capi.NSCAL) * 8 * N * len(wanted)
            rec.update({"window_over_fresh_full": med[nm] / med["fresh_full"], "window_over_fresh_144": med[nm] / med["fresh_144"],
                        "holds": bool(med[nm] <= med["fresh_144"] + (c[-1] - c[0])),
                        "same_rows_inside_fresh_full_us": med["fresh_full"] - med["fresh_288"],
                        "window_over_same_rows_inside_fresh_full": med[nm] / (med["fresh_full"] - med["fresh_288"]), "state_bytes_laid_out": state_bytes,
                        "faulted_fraction": float((stw != 0).double().mean()), "faulted_fraction_fresh_full": float((stf != 0).double().mean()),
                        "ksat0_gradient_norm": float(gw[("ksat", 0)].norm()), "ksat0_gradient_norm_fresh_full": float(gf[("ksat", 0)].norm())})
        line = json.dumps(rec)
        print(line, flush=True)
        fh.write(line + "\n")
