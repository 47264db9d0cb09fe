"""What the tangent kernels that take a forcing direction cost beside the window kernels they were made from
(lgar_forward_tangent_forced).
(dev tool)  usage: python tools/forcing_tangent_cost.py [N] [--out FILE]   (FILE: profiles/r18/forcing_tangent_cost.jsonl by default)

Job: BASELINE configs[4]'s shape -- N = 100 000 perturbed columns (workloads.perturbed_columns, per-column forcing scale), 3
layers, fp64, the 144 rows of the synth_1 storm, the 9 one-hot directions over (alpha, n, Ksat) x layer side by side in groups of
adjacent lanes that share the trapezoid (what autograd.parameter_vjp launches), a ramp on the runoff as the incoming gradient.
  window:        lgar_forward_tangent_window, 9 lanes per column;
  forced_null:   lgar_forward_tangent_forced with both forcing tangents NULL, the same 9 lanes: the same results bit for bit,
                 so the difference is what the new kernels' two carried registers, two pointer tests per step and larger
                 argument block cost;
  forced_9+2:    9 parameter lanes and 2 forcing lanes (a precipitation and a PET multiplier) per column, 11 lanes;
  forced_9+7:    9 parameter lanes and 7 forcing lanes (the snow parameters), 16 lanes;
  window_11, window_16: the window kernels over as many lanes (the extra lanes carry a zero direction), what the lanes alone cost.
Device-event time of one call each, the jobs alternating in one process, 2 warm-ups, median of 7.  The condition, in the form of
sections 12 - 19: forced_null's median is not above window's by more than window's own max - min.  The others are reported as
measured, and so are window_f32 / forced_null_f32 (the same pair on the fp32 kernels, every lane on its own) and snow_forward_B<n> /
snow_tangent7_B<n> (the snowpack's forward with its pack against its tangent along 7 directions, T = 144); over_window is the ratio
to the job's own partner.  One JSON line per result."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgar_py_amd as lg
from lgar_py_amd import _capi
from lgar_py_amd import workloads as W

args = sys.argv[1:]
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "r18", "forcing_tangent_cost.jsonl")
N = int(args[0]) if args and args[0].isdigit() else 100_000
REPS, WARM = 7, 2
PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
KINDS = ("alpha", "n", "ksat")

Pn = W.perturbed_columns(N, seed=0)
sc = W.forcing_scale(N, seed=1)
f = W.synth1_forcing()
pr = torch.tensor(f[:, 0:1] * sc[None, :], device="cuda")
pe = torch.zeros_like(pr)
T = pr.shape[0]
w = torch.linspace(0.5, 1.5, T, device="cuda", dtype=torch.float64)[:, None].expand(T, N).contiguous()
kw = dict(dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64)
soil = {k: torch.tensor(Pn[k], device="cuda") for k in PARAMS}


def lanes(G):
    """(engine over G lanes per column, its 9 one-hot directions in lanes 0..8, forcing tangents [T, N, G] in lanes 9..)"""
    eng = lg.LgarEngine(*[soil[k].repeat_interleave(G, dim=1) for k in PARAMS], with_state=False, **kw)
    dirs = {k: torch.zeros(3, G * N, dtype=torch.float64, device="cuda") for k in KINDS}
    for b, (kind, l) in enumerate((kind, l) for kind in KINDS for l in range(3)):
        dirs[kind][l, b::G] = 1.0
    dp = torch.zeros(T, N, G, dtype=torch.float64, device="cuda")
    de = torch.zeros(T, N, G, dtype=torch.float64, device="cuda")
    for j in range(9, G):
        dp[:, :, j] = pr * (1.0 + 0.1 * (j - 9))  # (the values do not matter to the time: dual arithmetic has no fast zeros)
        de[:, :, j] = 0.01 * (j - 8)
    return eng, dirs, dp, de


def window(G):
    eng, dirs, _, _ = lanes(G)
    return lambda: eng.tangent_window(dirs, pr, pe, w_runoff=w, keep_state=False, forcing_group=G, share=G)


def forced(G):
    eng, dirs, dp, de = lanes(G)
    return lambda: eng.tangent_window(dirs, pr, pe, w_runoff=w, keep_state=False, forcing_group=G, share=G, d_precip=dp, d_pet=de)


def forced_null(G):
    """the forced entry with both tangents NULL, by the engine's own argument blocks (tangent_window would take the window entry)"""
    eng, dirs, _, _ = lanes(G)
    win = _capi.LgarTangentWindow(None, None, None, None, None)

    def call():
        inputs = eng._tangent_inputs(dirs, pr, pe, w, None, G, G, None)
        return eng._tangent_call("forward_tangent_window", inputs, None, False, (C.byref(win),), d_forcing=(None, None))
    return call


def f32_pair():
    """the fp32 kernels (8-slot, two waves per SIMD: the family whose register spills grew most), every lane on its own: the 9
    directions as 9 N columns, the window entry against the forced entry with NULL tangents"""
    eng = lg.LgarEngine(*[soil[k].repeat_interleave(9, dim=1) for k in PARAMS], with_state=False, **dict(kw, dtype=torch.float32))
    dirs = {k: torch.zeros(3, 9 * N, dtype=torch.float32, device="cuda") for k in KINDS}
    for b, (kind, l) in enumerate((kind, l) for kind in KINDS for l in range(3)):
        dirs[kind][l, b::9] = 1.0
    win = _capi.LgarTangentWindow(None, None, None, None, None)

    def null():
        inputs = eng._tangent_inputs(dirs, pr, pe, w, None, 9, 0, None)
        return eng._tangent_call("forward_tangent_window", inputs, None, False, (C.byref(win),), d_forcing=(None, None))
    return (lambda: eng.tangent_window(dirs, pr, pe, w_runoff=w, keep_state=False, forcing_group=9)), null


def snow_jobs():
    """the snow tangent at section 19's shapes (T = 144): 7 directions, one per parameter, against the forward with its pack"""
    out = {}
    for B in (64, 4096, 65536):
        gen = torch.Generator().manual_seed(B)
        p = (torch.rand(144, B, generator=gen, dtype=torch.float64) * 0.4).cuda()
        ta = (torch.rand(144, B, generator=gen, dtype=torch.float64) * 8.0 - 3.0).cuda()
        snow = lg.CatchmentSnow(-1.0, 2.0, 0.4, 1.1, 0.9, 0.05, 0.1, 1.0, n_catchments=B)
        dpar = torch.zeros(7, 7, B, dtype=torch.float64, device="cuda")
        for k in range(7):
            dpar[k, k] = 1.0
        block = torch.zeros(144, B, 7, dtype=torch.float64, device="cuda")
        out["snow_forward_B%d" % B] = (lambda snow=snow, p=p, ta=ta: snow.run(p, ta, carry=False, pack=True))
        out["snow_tangent7_B%d" % B] = (lambda snow=snow, p=p, ta=ta, dpar=dpar, block=block: snow.tangent(p, ta, 7, dpar=dpar, out=block))
    return out


f32_window, f32_null = f32_pair()
jobs = {"window_f32": f32_window, "forced_null_f32": f32_null, **snow_jobs(), "window": window(9), "forced_null": forced_null(9), "forced_9+2": forced(11), "forced_9+7": forced(16),
        "window_11": window(11), "window_16": window(16)}
lanes_of = {"window": 9, "forced_null": 9, "forced_9+2": 11, "forced_9+7": 16, "window_11": 11, "window_16": 16}


def partner(nm):
    """the job a ratio is taken against: the fp64 window entry, the fp32 one, or the snowpack's forward at the same B"""
    if nm.startswith("snow"):
        return "snow_forward_B" + nm.split("_B")[1]
    return "window_f32" if nm.endswith("f32") else "window"


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
same = all(torch.equal(x, y) for x, y in zip(jobs["window"]()[:3:2], jobs["forced_null"]()[:3:2]))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
med = {nm: sorted(v)[len(v) // 2] for nm, v in us.items()}
with open(OUT, "a") as fh:
    for nm, v in us.items():
        v = sorted(v)
        rec = {"mode": "forcing_tangent_cost", "job": nm, "columns": int(nm.split("_B")[1]) if nm.startswith("snow") else N, "lanes_per_column": lanes_of.get(nm, 9 if "f32" in nm else (7 if "tangent7" in nm else 1)), "rows": T, "us_median": med[nm],
               "us_min": v[0], "us_max": v[-1], "reps": REPS, "over_window": med[nm] / med[partner(nm)],
               "library": os.environ.get("LGAR_LIB", "default")}
        if nm == "forced_null":
            c = sorted(us["window"])
            rec.update({"holds": bool(med[nm] <= med["window"] + (c[-1] - c[0])), "window_spread_us": c[-1] - c[0],
                        "same_bits_as_window": bool(same)})
        line = json.dumps(rec)
        print(line, flush=True)
        fh.write(line + "\n")
