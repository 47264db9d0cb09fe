"""What the catchment snowpack costs: lgar_catchment_snow (forward, with the pack series) and lgar_catchment_snow_grad (gp, gta,
gpar and gstate in one call) over fp64 [T, B] matrices, one launch each.
(dev tool)  usage: python tools/snow_cost.py [quick] [--out FILE]      (FILE: profiles/r16/snow_cost.jsonl by default)

Shapes: T in {144, 8760} x B in {64, 4096, 65536}; `quick` leaves T = 8760 out.  Per shape and operation: device-event time of
one call (median of 7 after 2 warm-up calls; the call's output allocation included) and GB/s on the algorithmic bytes --
forward p, ta, w, ice, liq once each, the parameters and both states: 8 T B 5 + 8 B 11; backward gw, gice, gliq, p, ta, ice, liq,
gp, gta once each, the parameters, state_in, gpar and gstate: 8 T B 9 + 8 B 18.

The yardstick, alternating with the kernel in the same process on the same tensors: the plain torch statement -- a Python loop
over the rows of two dozen elementwise operations each (torch.where); its gradient by autograd (torch.autograd.grad on the graph
of one forward, built outside the timing).  It is timed at T = 144 only: at T = 8760 it is T x two dozen launches, and autograd
holds T graphs.  The condition of DESIGN.md sections 12 - 17: at no shape where both were timed is the kernel's median above the
torch statement's median by more than that statement's own max - min.  One JSON line per result."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lgar_py_amd import _capi, snow
from lgar_py_amd.snow import CatchmentSnow

args = sys.argv[1:]
quick = "quick" in args
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "r16", "snow_cost.jsonl")
REPS, WARM = 7, 2


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


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as fh:
        fh.write(line + "\n")


def report(op, T, B, nbytes, ker, ref=None, **more):
    med = ker[len(ker) // 2]
    rec = {"mode": "snow_cost", "op": op, "T": T, "B": B, "us_median": med, "us_min": ker[0], "us_max": ker[-1], "reps": REPS,
           "algorithmic_bytes": nbytes, "GBps": nbytes / (med * 1e-6) / 1e9, "us_per_chunk_of_8_rows": med / ((T + 7) // 8),
           "library": os.environ.get("LGAR_LIB", "default")}
    if ref is not None:
        rmed = ref[len(ref) // 2]
        rec.update({"torch_us_median": rmed, "torch_us_min": ref[0], "torch_us_max": ref[-1], "kernel_over_torch": med / rmed,
                    "holds": bool(med <= rmed + (ref[-1] - ref[0]))})
    rec.update(more)
    emit(rec)


def torch_statement(p, ta, par, dt, state):
    """w, ice, liq [T, B] by the plain statement (differentiable)"""
    tlo, thi, tm, sfcf, cfmax, cfr, cwh = par
    cd = cfmax * dt
    cr = cfr * cd
    span = thi - tlo
    ice, liq = state[0], state[1]
    zero, one = torch.zeros_like(ice), torch.ones_like(ice)
    ws, ices, liqs = [], [], []
    for t in range(p.shape[0]):
        Ta, pd = ta[t], p[t] * dt
        lo = Ta <= tlo
        fr = torch.where(lo, zero, torch.where(Ta >= thi, one, (Ta - tlo) / span))
        rain = pd * fr
        d = Ta - tm
        warm = d > 0
        ice1 = ice + sfcf * (pd - rain)
        pm, pr = cd * d, cr * (-d)
        melt = torch.where(warm, torch.where(pm > ice1, ice1, pm), zero)
        refr = torch.where(warm, zero, torch.where(pr > liq, liq, pr))
        ice = (ice1 - melt) + refr
        liq1 = ((liq + rain) + melt) - refr
        cap = cwh * ice
        over = liq1 > cap
        ws.append(torch.where(over, liq1 - cap, zero) / dt)
        liq = torch.where(over, cap, liq1)
        ices.append(ice)
        liqs.append(liq)
    return torch.stack(ws), torch.stack(ices), torch.stack(liqs)


os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
gen = torch.Generator(device="cuda").manual_seed(0)
rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device="cuda", generator=gen)
dev = torch.device("cuda:0")
lib = _capi.load()
for T in ((144,) if quick else (144, 8760)):
    for B in (64, 4096, 65536):
        dt = 1.0
        tlo = -2.0 + 2.0 * rand(B)
        par = [tlo, tlo + 0.5 + 2.5 * rand(B), -0.5 + 1.5 * rand(B), 0.8 + 0.5 * rand(B), 0.05 + 0.25 * rand(B), 0.02 + 0.08 * rand(B),
               0.02 + 0.13 * rand(B)]
        state = torch.stack([5.0 * rand(B), 0.3 * rand(B)])
        rows = torch.arange(T, dtype=torch.float64, device="cuda")[:, None]
        ta = 4.0 * torch.sin(6.28 * rand(B)[None, :] + 0.26 * rows) + 2.0 * (rand(T, B) - 0.5)  # a daily wave around the thresholds
        p = 0.5 * rand(T, B) * (rand(T, B) < 0.3)  # precipitation in a third of the rows
        gw, gi, gl = rand(T, B) - 0.4, 0.1 * (rand(T, B) - 0.4), 0.1 * (rand(T, B) - 0.4)
        store = CatchmentSnow(*par, dt)
        w, ice, liq = store.run(p, ta, carry=False, state=state, pack=True)
        fwd_bytes, bwd_bytes = 8 * T * B * 5 + 8 * B * 11, 8 * T * B * 9 + 8 * B * 18
        kernel_fwd = lambda: store.run(p, ta, carry=False, state=state, pack=True)
        kernel_bwd = lambda: snow._backward(lib, dev, gw, gi, gl, p, ta, ice, liq, store.par, dt, state, True, True, True)
        if T == 144:
            with torch.no_grad():
                ref = torch_statement(p, ta, par, dt, state)
            err = max(float(((a - b).abs() / b.abs().clamp_min(1e-300)).max()) for a, b in zip(ref, (w, ice, liq)))
            leaves = [v.clone().requires_grad_(True) for v in [p, ta] + par + [state]]
            graph = torch_statement(leaves[0], leaves[1], leaves[2:9], dt, leaves[9])

            def torch_fwd():
                with torch.no_grad():
                    torch_statement(p, ta, par, dt, state)

            ker, ref_us = timed([kernel_fwd, torch_fwd])
            report("forward+pack", T, B, fwd_bytes, ker, ref_us, torch_max_rel_diff=err)
            ker, ref_us = timed([kernel_bwd, lambda: torch.autograd.grad(graph, leaves, (gw, gi, gl), retain_graph=True)])
            report("adjoint+gta+gpar+gstate", T, B, bwd_bytes, ker, ref_us)
            del graph, leaves, ref
        else:
            report("forward+pack", T, B, fwd_bytes, timed([kernel_fwd])[0])
            report("adjoint+gta+gpar+gstate", T, B, bwd_bytes, timed([kernel_bwd])[0])
        del p, ta, gw, gi, gl, w, ice, liq, store
        torch.cuda.empty_cache()
