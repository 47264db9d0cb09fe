"""What the catchment canopy costs: lgar_catchment_canopy (forward, with the store and evaporation series),
lgar_catchment_canopy_grad (gp, ge, glai, gpar and gstate in one call) and lgar_catchment_canopy_tangent along all 3 parameters
(dw and dpet into [T, B, 3] blocks) over fp64 [T, B] matrices with leaf area, one launch each.
(dev tool)  usage: python tools/canopy_cost.py [--out FILE]      (FILE: profiles/r19/canopy_cost.jsonl by default)

Shapes: T = 144 x B in {64, 4096, 65536}.  Per shape and job: device-event time of one call (median of 7 after 2 warm-up calls; the
call's output allocation included) and GB/s on the algorithmic bytes -- forward p, e, lai, w, pet_out, store, evap once each:
8 T B 7; adjoint gw, gpet, gstore, gevap, p, e, lai, store, gp, ge, glai: 8 T B 11; tangent p, e, lai once per direction and dw,
dpet: 8 T B 3 (3 + 2).  Each job is measured beside its partner, the snowpack's forward (with the pack series) at the same B, the
two alternating in one process.  There is no bar on these: they are recorded so that the next change has something to compare
with.  One JSON line per result."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lgar_py_amd import _capi, canopy
from lgar_py_amd.canopy import CatchmentCanopy
from lgar_py_amd.snow import CatchmentSnow

args = sys.argv[1:]
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "r19", "canopy_cost.jsonl")
REPS, WARM, T = 7, 2, 144


def timed(fns):
    """the functions alternating: sorted us of each"""
    us = [[] for _ in fns]
    for i in range(WARM + REPS):
        for which, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= WARM:
                us[which].append(1e3 * a.elapsed_time(b))
    return [sorted(u) for u in us]


def report(op, B, nbytes, ker, ref):
    med, rmed = ker[len(ker) // 2], ref[len(ref) // 2]
    rec = {"mode": "canopy_cost", "op": op, "T": T, "B": B, "us_median": med, "us_min": ker[0], "us_max": ker[-1], "reps": REPS,
           "algorithmic_bytes": nbytes, "GBps": nbytes / (med * 1e-6) / 1e9, "partner": "snow forward+pack", "partner_us_median": rmed,
           "partner_us_min": ref[0], "partner_us_max": ref[-1], "over_partner": med / rmed, "library": os.environ.get("LGAR_LIB", "default")}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as fh:
        fh.write(line + "\n")


os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
gen = torch.Generator(device="cuda").manual_seed(0)
rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device="cuda", generator=gen)
dev = torch.device("cuda:0")
lib = _capi.load()
for B in (64, 4096, 65536):
    dt = 1.0
    par = [0.2 * rand(B), 2.5 * rand(B), rand(B)]
    state = 0.3 * rand(1, B)
    p = 2.0 * rand(T, B) * (rand(T, B) < 0.5)  # precipitation in half of the rows
    e, lai = 0.4 * rand(T, B), 0.5 + 4.0 * rand(T, B)
    g = [rand(T, B) - 0.4 for _ in range(4)]
    can = CatchmentCanopy(*par, dt)
    w, pet_out, store, evap = can.run(p, e, lai, carry=False, state=state, store=True)
    dpar = torch.zeros(3, 3, B, dtype=torch.float64, device="cuda")
    dpar[[0, 1, 2], [0, 1, 2]] = 1.0
    tlo = -2.0 + 2.0 * rand(B)
    snow = CatchmentSnow(tlo, tlo + 0.5 + 2.5 * rand(B), -0.5 + 1.5 * rand(B), 0.8 + 0.5 * rand(B), 0.05 + 0.25 * rand(B), 0.02 + 0.08 * rand(B),
                         0.02 + 0.13 * rand(B), dt)
    rows = torch.arange(T, dtype=torch.float64, device="cuda")[:, None]
    ta = 4.0 * torch.sin(6.28 * rand(B)[None, :] + 0.26 * rows) + 2.0 * (rand(T, B) - 0.5)
    pack = torch.stack([5.0 * rand(B), 0.3 * rand(B)])
    partner = lambda: snow.run(p, ta, carry=False, state=pack, pack=True)
    jobs = (("forward+store", 8 * T * B * 7, lambda: can.run(p, e, lai, carry=False, state=state, store=True)),
            ("adjoint+glai+gpar+gstate", 8 * T * B * 11,
             lambda: canopy._backward(lib, dev, g[0], g[1], g[2], g[3], p, e, lai, store, can.par, dt, state, True, True, True)),
            ("tangent D=3 (dw, dpet)", 8 * T * B * 3 * 5, lambda: can.tangent(p, e, 3, lai=lai, dpar=dpar, state=state)))
    for op, nbytes, job in jobs:
        ker, ref = timed([job, partner])
        report(op, B, nbytes, ker, ref)
    del p, e, lai, g, w, pet_out, store, evap, ta
    torch.cuda.empty_cache()
