"""What the catchment baseflow costs: lgar_catchment_baseflow (forward, with the storage) and lgar_catchment_baseflow_grad (gr, gpar
and gstate in one call) over fp64 [T, B] matrices, one launch each.
(dev tool)  usage: python tools/baseflow_cost.py [quick] [--out FILE]      (FILE: profiles/r11/baseflow_cost.jsonl by default)

Shapes: T in {144, 8760} x B in {64, 4096, 65536}; `quick` leaves T = 8760 out.  Per shape and operation: device-event time of
one call (median of 7 after 2 warm-up calls; the call's output allocation included) and GB/s on the algorithmic bytes --
forward r, q, s once each, the parameters and both states: 8 T B 3 + 8 B 5; backward gq, gs, r, s, gr once each, the
parameters, state_in, gpar and gstate: 8 T B 5 + 8 B 8.

The yardstick, alternating with the kernel in the same process on the same tensors: the plain torch statement -- a Python loop
over the rows of a dozen elementwise operations each (torch.exp, torch.where); its gradient by autograd (torch.autograd.grad on
the graph of one forward, built outside the timing).  It is timed at T = 144 only: at T = 8760 it is T x a dozen launches, and
autograd holds T graphs.  The condition of DESIGN.md sections 12 - 14: at no shape where both were timed is the kernel's median
above the torch statement's median by more than that statement's own max - min.  One JSON line per result."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lgar_py_amd import _capi, baseflow
from lgar_py_amd.baseflow import CatchmentBaseflow

args = sys.argv[1:]
quick = "quick" in args
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "r11", "baseflow_cost.jsonl")
REPS, WARM = 7, 2
ZMAX = _capi.GW_ZMAX


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
    rec = {"mode": "baseflow_cost", "op": op, "T": T, "B": B, "us_median": med, "us_min": ker[0], "us_max": ker[-1], "reps": REPS,
           "algorithmic_bytes": nbytes, "GBps": nbytes / (med * 1e-6) / 1e9, "us_per_chunk_of_8_rows": med / ((T + 7) // 8),
           "library": os.environ.get("LGAR_LIB", "default")}
    if ref is not None:
        rmed = ref[len(ref) // 2]
        rec.update({"torch_us_median": rmed, "torch_us_min": ref[0], "torch_us_max": ref[-1], "kernel_over_torch": med / rmed,
                    "holds": bool(med <= rmed + (ref[-1] - ref[0]))})
    rec.update(more)
    emit(rec)


def torch_statement(r, cgw, expon, smax, dt, state):
    """q, s [T, B] by the plain statement (differentiable)"""
    S, qs, ss = state, [], []
    cd = cgw * dt
    zero, top = torch.zeros_like(state), torch.full_like(state, ZMAX)
    for t in range(r.shape[0]):
        A = S + r[t]
        z = expon * (A / smax)
        zc = torch.where(z < 0, zero, torch.where(z > ZMAX, top, z))
        f = cd * (torch.exp(zc) - 1.0)
        pre = torch.where(f > A, A, f)
        qq = torch.where(pre < 0, zero, pre)
        S = A - qq
        qs.append(qq)
        ss.append(S)
    return torch.stack(qs), torch.stack(ss)


os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
gen = torch.Generator(device="cuda").manual_seed(0)
rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device="cuda", generator=gen)
dev = torch.device("cuda:0")
lib = _capi.load()
for T in ((144,) if quick else (144, 8760)):
    for B in (64, 4096, 65536):
        cgw, expon, smax = 0.01 + 0.09 * rand(B), 1.0 + 5.0 * rand(B), 10.0 + 30.0 * rand(B)
        dt = 1.0
        state = smax * rand(B)
        r = 0.5 * rand(T, B) * (rand(T, B) < 0.3)  # recharge arrives in a third of the rows
        gq, gs = rand(T, B) - 0.4, 0.1 * (rand(T, B) - 0.4)
        store = CatchmentBaseflow(cgw, expon, smax, dt)
        q, s = store.run(r, carry=False, state=state, storage=True)
        fwd_bytes, bwd_bytes = 8 * T * B * 3 + 8 * B * 5, 8 * T * B * 5 + 8 * B * 8
        kernel_fwd = lambda: store.run(r, carry=False, state=state, storage=True)
        kernel_bwd = lambda: baseflow._backward(lib, dev, gq, gs, r, s, store.par, dt, state, True, True)
        if T == 144:
            with torch.no_grad():
                qt, st_ = torch_statement(r, cgw, expon, smax, dt, state)
            err = max(float(((qt - q).abs() / q.abs().clamp_min(1e-300)).max()), float(((st_ - s).abs() / s.abs().clamp_min(1e-300)).max()))
            leaves = [v.clone().requires_grad_(True) for v in (r, cgw, expon, smax, state)]
            graph = torch_statement(leaves[0], leaves[1], leaves[2], leaves[3], dt, leaves[4])

            def torch_fwd():
                with torch.no_grad():
                    torch_statement(r, cgw, expon, smax, dt, state)

            ker, ref = timed([kernel_fwd, torch_fwd])
            report("forward", T, B, fwd_bytes, ker, ref, torch_max_rel_diff=err)
            ker, ref = timed([kernel_bwd, lambda: torch.autograd.grad(graph, leaves, (gq, gs), retain_graph=True)])
            report("adjoint+gpar+gstate", T, B, bwd_bytes, ker, ref)
            del graph, leaves, qt, st_
        else:
            report("forward", T, B, fwd_bytes, timed([kernel_fwd])[0])
            report("adjoint+gpar+gstate", T, B, bwd_bytes, timed([kernel_bwd])[0])
        del r, gq, gs, q, s, store
        torch.cuda.empty_cache()
