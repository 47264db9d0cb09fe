"""What the Muskingum-Cunge network costs: lgar_network_route_mc (forward) and lgar_network_route_mc_grad (adjoint with gpar and
gstate in one call) over fp64 [T, B] matrices, one launch per level of the network.
(dev tool)  usage: python tools/network_mc_cost.py [quick] [--out FILE]      (FILE: profiles/r14/network_mc_cost.jsonl by default)

Networks, as tools/network_cost.py: a full binary tree in heap numbering and a random river-like forest (catchment i drains into
a random earlier one; 1 % outlets), each with B in {64, 4096, 65 536} catchments renumbered in level order, at T = 144 and
T = 8760 (a year of hourly rows; `quick` leaves it out).
Per case and operation: device-event time of one call, median of 7 after 2 warm-up calls, alternating in ONE process on the same
tensors with
  - the linear CatchmentNetwork.route / its adjoint with the coefficient gradient on the same network (every shape): the ratio to
    it is a finding, not a bar -- the Muskingum-Cunge row is a dependent chain of a logarithm, an exponential and four divisions
    where the linear row is two multiply-adds;
  - the plain torch statement (T = 144 only: it is T x levels x a dozen elementwise launches and a pow): for each row and level the
    clamp, the power law, the coefficients and the three-term update of the level's reaches, then index_add of their discharge
    into the inflow downstream; its gradient by autograd (torch.autograd.grad on the graph of one forward, built outside the
    timing).  The condition of DESIGN.md sections 12 - 15: at no shape where both were timed is the kernel's median above the torch
    statement's median by more than that statement's own max - min.
us_per_chunk is the call's time per level and chunk of 8 rows (LGAR_NET_CHUNK): what one lane's dependent chain over 8 rows costs
when the level is narrow.  One JSON line per result."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lgar_py_amd.network import MC_RMAX, MC_RMIN, CatchmentNetwork, muskingum_coefficients

args = sys.argv[1:]
quick = "quick" in args
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "r14", "network_mc_cost.jsonl")
REPS, WARM = 7, 2
DT = 1.0


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


def report(op, name, net, T, ker, lin, ref=None, **more):
    med, lmed = ker[len(ker) // 2], lin[len(lin) // 2]
    widths = np.diff(net.level_ptr)
    chunks = net.n_levels * ((T + 7) // 8)
    rec = {"mode": "network_mc_cost", "op": op, "network": name, "T": T, "B": net.B, "E": net.n_edges, "levels": net.n_levels,
           "in_degree_max": int(np.diff(net.up_ptr_host).max()), "width_max": int(widths.max()), "width_min": int(widths.min()),
           "us_median": med, "us_min": ker[0], "us_max": ker[-1], "reps": REPS, "us_per_chunk": med / chunks,
           "linear_us_median": lmed, "linear_us_min": lin[0], "linear_us_max": lin[-1], "linear_us_per_chunk": lmed / chunks,
           "ratio_to_linear": med / lmed, "library": os.environ.get("LGAR_LIB", "default")}
    if ref is not None:
        rmed = ref[len(ref) // 2]
        rec.update({"torch_us_median": rmed, "torch_us_min": ref[0], "torch_us_max": ref[-1], "kernel_over_torch": med / rmed,
                    "holds": bool(med <= rmed + (ref[-1] - ref[0]))})
    rec.update(more)
    emit(rec)


def level_order(down):
    """down renumbered so that index order = (level, old index) order"""
    down = np.asarray(down, dtype=np.int64)
    new_of = np.empty(len(down), dtype=np.int64)
    new_of[CatchmentNetwork(down, device="cpu").order_host] = np.arange(len(down))
    out = np.full(len(down), -1, dtype=np.int64)
    out[new_of] = np.where(down >= 0, new_of[np.maximum(down, 0)], -1)
    return out


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


def torch_statement(levels, x, kref, beta, X, qref, state):
    """y [T, B] by the plain statement (differentiable: no in-place operation on a tensor autograd needs)"""
    half = 0.5 * DT
    Iprev, Oprev = state[0], state[1]
    rows = []
    for t in range(x.shape[0]):
        I, y = x[t], torch.zeros_like(x[0])
        for bs, src, dst in levels:
            Op = Oprev[bs]
            K = kref[bs] * torch.pow(torch.clamp(Op / qref[bs], MC_RMIN, MC_RMAX), -beta[bs])
            KX = K * X[bs]
            u = K - KX
            D = u + half
            O = ((half - KX) / D * I[bs] + (half + KX) / D * Iprev[bs]) + (u - half) / D * Op
            y = y.index_copy(0, bs, O)
            if src is not None:
                I = I.index_add(0, dst, O[src])
        rows.append(y)
        Iprev, Oprev = I, y
    return torch.stack(rows)


rng = np.random.default_rng(0)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
gen = torch.Generator(device="cuda").manual_seed(0)
rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device="cuda", generator=gen)
for name in ("binary_tree", "river_forest"):
    for B in (64, 4096, 65536):
        if name == "binary_tree":
            down = np.array([-1] + [(b - 1) // 2 for b in range(1, B)], dtype=np.int64)
        else:
            down = np.array([-1] + [int(rng.integers(0, i)) if rng.random() >= 0.01 else -1 for i in range(1, B)], dtype=np.int64)
        net = CatchmentNetwork(level_order(down))
        kref, beta, X = 1.0 + 3.0 * rand(B), 0.2 + 0.4 * rand(B), 0.05 + 0.1 * rand(B)
        par = torch.stack([kref, beta, X, torch.ones_like(kref)]).contiguous()
        # qref of a reach: the mean discharge it sees (its upstream area x the mean lateral inflow), so rho stays around 1
        area = net.accumulate(torch.ones(1, B, dtype=torch.float64, device="cuda"))[0]
        par[3] = 0.5 * area
        coef = muskingum_coefficients(kref, X, DT).contiguous()
        state = torch.stack([0.5 * torch.ones_like(area), 0.5 * area]).contiguous()
        for T in (144,) if quick else (144, 8760):
            x, gy = rand(T, B), rand(T, B)
            y = net._forward_mc(x, par, DT, MC_RMIN, MC_RMAX, state, False)[0]
            yl = net.route(x, coef, carry=False, state=state)
            inside = float(((y / par[3] > MC_RMIN) & (y / par[3] < MC_RMAX)).double().mean())
            kernel_fwd = lambda: net._forward_mc(x, par, DT, MC_RMIN, MC_RMAX, state, False)
            kernel_bwd = lambda: net._backward_mc(gy, x, y, par, DT, MC_RMIN, MC_RMAX, state, True, True)
            linear_fwd = lambda: net.route(x, coef, carry=False, state=state)
            linear_bwd = lambda: net._backward(gy, coef, x, yl, state)
            if T == 144:
                levels = level_lists(net)
                with torch.no_grad():
                    yt = torch_statement(levels, x, par[0], par[1], par[2], par[3], state)
                err = float((yt - y).abs().max() / y.abs().max())
                leaves = [v.clone().requires_grad_(True) for v in (x, par[0], par[1], par[2], state)]
                graph = torch_statement(levels, leaves[0], leaves[1], leaves[2], leaves[3], par[3], leaves[4])

                def torch_fwd():
                    with torch.no_grad():
                        torch_statement(levels, x, par[0], par[1], par[2], par[3], state)

                ker, lin, ref = timed([kernel_fwd, linear_fwd, torch_fwd])
                report("forward", name, net, T, ker, lin, ref, torch_max_rel_diff=err, rows_inside=inside)
                ker, lin, ref = timed([kernel_bwd, linear_bwd, lambda: torch.autograd.grad(graph, leaves, gy, retain_graph=True)])
                report("adjoint+gpar+gstate", name, net, T, ker, lin, ref)
                del graph, leaves, yt, levels
            else:
                ker, lin = timed([kernel_fwd, linear_fwd])
                report("forward", name, net, T, ker, lin, rows_inside=inside)
                ker, lin = timed([kernel_bwd, linear_bwd])
                report("adjoint+gpar+gstate", name, net, T, ker, lin)
            del x, gy, y, yl
            torch.cuda.empty_cache()
