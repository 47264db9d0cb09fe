"""What the catchment network costs: lgar_network_route (forward) and lgar_network_route_grad (adjoint + coefficient gradient in
one call) over fp64 [T, B] matrices, one launch per level of the network.
(dev tool)  usage: python tools/network_cost.py [quick] [--out FILE]      (FILE: profiles/r10/network_cost.jsonl by default)

Networks: a full binary tree, B = 4095 (12 levels); a random river-like forest, B = 65 536 (catchment i drains into a random
earlier one; 1 % outlets; its depth is recorded); a chain, B = 64 (64 levels of one reach).  Each at T = 144; the first two also
at T = 8760 (a year of hourly rows) for the kernel ALONE: the torch statement there is T x depth launches and is timed at
T = 144 only.  Every network with catchments numbered in level order (a wave's 64 reaches are neighbours in memory) and numbered
at random (the gather through `order`).  `quick` leaves T = 8760 out.
Per-level cost by level width: `width` parallel chains of 16 reaches -- 16 levels, each exactly `width` wide -- at T = 144, kernel
alone; us_per_level is the call's time / 16.

A level takes as long as its slowest reach, and a reach's walk one dependent round of loads per upstream entry and chunk of
rows: in_degree_max is recorded beside the level widths.
Per case and operation: device-event time of one call (median of 7 after 2 warm-up calls) and GB/s on the algorithmic bytes --
forward: x and y once each and y of every upstream entry, 8 T (2 B + E) + 24 B; backward: gy, gx, gx[down], x, y and y of every
upstream entry, 8 T (4 B + 2 E) + 48 B.

The yardstick, alternating with the kernel in the same process on the same tensors: the plain torch statement -- for each row
and each level the three-term update of the level's reaches, then index_add of their discharge into the inflow of their
downstream reaches; its gradient by autograd (torch.autograd.grad on the graph of one forward, built outside the timing).  The
condition of DESIGN.md sections 12 - 14: at no shape where both were timed is the kernel's median above the torch statement's
median by more than that statement's own max - min.  One JSON line per result."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lgar_py_amd.network import CatchmentNetwork, muskingum_coefficients

args = sys.argv[1:]
quick = "quick" in args
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "r10", "network_cost.jsonl")
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


def report(op, name, numbering, net, T, nbytes, ker, ref=None, **more):
    med = ker[len(ker) // 2]
    widths = np.diff(net.level_ptr)
    rec = {"mode": "network_cost", "op": op, "network": name, "numbering": numbering, "T": T, "B": net.B, "E": net.n_edges,
           "levels": net.n_levels, "in_degree_max": int(np.diff(net.up_ptr_host).max()), "width_max": int(widths.max()), "width_median": float(np.median(widths)), "width_min": int(widths.min()),
           "us_median": med, "us_min": ker[0], "us_max": ker[-1], "reps": REPS, "algorithmic_bytes": nbytes,
           "GBps": nbytes / (med * 1e-6) / 1e9, "us_per_level": med / net.n_levels, "library": os.environ.get("LGAR_LIB", "default")}
    if ref is not None:
        rmed = ref[len(ref) // 2]
        rec.update({"torch_us_median": rmed, "torch_us_min": ref[0], "torch_us_max": ref[-1], "kernel_over_torch": med / rmed,
                    "holds": bool(med <= rmed + (ref[-1] - ref[0]))})
    rec.update(more)
    emit(rec)


def renumber(down, how, seed=0):
    """down under a relabelling: "level": index order = (level, old index) order; "random": a random permutation."""
    down = np.asarray(down, dtype=np.int64)
    n = len(down)
    if how == "level":
        new_of = np.empty(n, dtype=np.int64)
        new_of[CatchmentNetwork(down, device="cpu").order_host] = np.arange(n)
    else:
        new_of = np.random.default_rng(seed).permutation(n)
    out = np.full(n, -1, dtype=np.int64)
    out[new_of] = np.where(down >= 0, new_of[np.maximum(down, 0)], -1)
    return out


def torch_statement(net, x, coef):
    """y [T, B] by the plain statement (differentiable: no in-place operation on a tensor autograd needs)"""
    T = x.shape[0]
    c0, c1, c2 = coef[0], coef[1], coef[2]
    Iprev = torch.zeros_like(x[0])
    Oprev = torch.zeros_like(x[0])
    rows = []
    for t in range(T):
        I, y = x[t], torch.zeros_like(x[0])
        for bs, src, dst in LEVELS:
            O = (c0[bs] * I[bs] + c1[bs] * Iprev[bs]) + c2[bs] * Oprev[bs]
            y = y.index_copy(0, bs, O)
            if src is not None:
                I = I.index_add(0, dst, O[src])
        rows.append(y)
        Iprev, Oprev = I, y
    return torch.stack(rows)


def level_lists(net):
    """per level: its reaches, the positions among them of those with a downstream reach, and those downstream reaches"""
    out = []
    for l in range(net.n_levels):
        bs = net.order_host[net.level_ptr[l]:net.level_ptr[l + 1]].astype(np.int64)
        d = net.downstream_host[bs].astype(np.int64)
        has = np.nonzero(d >= 0)[0]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        out.append((dev(bs), dev(has) if has.size else None, dev(d[has]) if has.size else None))
    return out


def parallel_chains(width, depth=16):
    """`width` chains of `depth` reaches side by side, numbered in level order: every level is exactly `width` wide"""
    down = np.arange(width * depth, dtype=np.int64) + width
    down[-width:] = -1
    return down


rng = np.random.default_rng(0)
tree = np.array([-1] + [(b - 1) // 2 for b in range(1, 4095)], dtype=np.int64)
river = np.array([-1] + [int(rng.integers(0, i)) if rng.random() >= 0.01 else -1 for i in range(1, 65536)], dtype=np.int64)
chain = np.array(list(range(1, 64)) + [-1], dtype=np.int64)
cases = [(name, down, how, T) for name, down in (("binary_tree", tree), ("river_forest", river), ("chain", chain))
         for how in ("level", "random") for T in ((144,) if quick or name == "chain" else (144, 8760))]
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
gen = torch.Generator(device="cuda").manual_seed(0)
for name, down, how, T in cases:
    net = CatchmentNetwork(renumber(down, how))
    B, E = net.B, net.n_edges
    x = torch.rand(T, B, dtype=torch.float64, device="cuda", generator=gen)
    gy = torch.rand(T, B, dtype=torch.float64, device="cuda", generator=gen)
    coef = muskingum_coefficients(1.0 + 3.0 * torch.rand(B, dtype=torch.float64, device="cuda", generator=gen),
                                  0.3 * torch.rand(B, dtype=torch.float64, device="cuda", generator=gen), 1.0).contiguous()
    fwd_bytes, bwd_bytes = 8 * T * (2 * B + E) + 24 * B, 8 * T * (4 * B + 2 * E) + 48 * B
    y = net.route(x, coef, carry=False)
    kernel_fwd = lambda: net.route(x, coef, carry=False)
    kernel_bwd = lambda: net._backward(gy, coef, x, y)
    if T == 144:
        LEVELS = level_lists(net)
        with torch.no_grad():
            yt = torch_statement(net, x, coef)
        err = float((yt - y).abs().max() / y.abs().max())
        xg, cg = x.clone().requires_grad_(True), coef.clone().requires_grad_(True)
        graph = torch_statement(net, xg, cg)

        def torch_fwd():
            with torch.no_grad():
                torch_statement(net, x, coef)

        ker, ref = timed([kernel_fwd, torch_fwd])
        report("forward", name, how, net, T, fwd_bytes, ker, ref, torch_max_rel_diff=err)
        ker, ref = timed([kernel_bwd, lambda: torch.autograd.grad(graph, (xg, cg), gy, retain_graph=True)])
        report("adjoint+coef_grad", name, how, net, T, bwd_bytes, ker, ref)
        del graph, xg, cg, yt, LEVELS
    else:
        report("forward", name, how, net, T, fwd_bytes, timed([kernel_fwd])[0])
        report("adjoint+coef_grad", name, how, net, T, bwd_bytes, timed([kernel_bwd])[0])
    del x, gy, y, coef, net
    torch.cuda.empty_cache()

# the per-level cost by level width
for width in (1, 16, 64, 256, 1024, 4096, 16384, 65536):
    T = 144
    net = CatchmentNetwork(parallel_chains(width))
    B, E = net.B, net.n_edges
    x = torch.rand(T, B, dtype=torch.float64, device="cuda", generator=gen)
    gy = torch.rand(T, B, dtype=torch.float64, device="cuda", generator=gen)
    coef = muskingum_coefficients(1.0 + 3.0 * torch.rand(B, dtype=torch.float64, device="cuda", generator=gen), 0.2, 1.0).contiguous()
    y = net.route(x, coef, carry=False)
    report("forward", "parallel_chains", "level", net, T, 8 * T * (2 * B + E) + 24 * B, timed([lambda: net.route(x, coef, carry=False)])[0])
    report("adjoint+coef_grad", "parallel_chains", "level", net, T, 8 * T * (4 * B + 2 * E) + 48 * B, timed([lambda: net._backward(gy, coef, x, y)])[0])
    del x, gy, y, coef, net
    torch.cuda.empty_cache()
