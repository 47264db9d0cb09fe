"""What the network with reaches and level-pool reservoirs costs: lgar_network_route_pool (forward, with the storage series) and
lgar_network_route_pool_grad (adjoint with gpar_mc, gpool and gstate in one call) over fp64 [T, B] matrices, up to two launches
per level of the network.
(dev tool)  usage: python tools/network_pool_cost.py [quick] [--out FILE]      (FILE: profiles/r15/network_pool_cost.jsonl by default)

Networks, as tools/network_mc_cost.py: a full binary tree in heap numbering and a random river-like forest (catchment i drains
into a random earlier one; 1 % outlets), each with B in {64, 4096, 65 536} catchments renumbered in level order, at T = 144 and
T = 8760 (a year of hourly rows; `quick` leaves it out), with 0 %, 1 % and 10 % of the nodes pools (chosen at random; at least one
where the share is not 0).
Per case and operation: device-event time of one call, median of 7 after 2 warm-up calls, alternating in ONE process on the same
tensors with
  - CatchmentNetwork route_mc / its adjoint on the same network with every node a reach (every shape): the ratio to it at 0 %
    pools is what the second entry point costs by itself, and (median - the 0 % median) / (levels that have both kinds) is what
    the second launch of a level costs; both are findings, not bars;
  - the plain torch statement (T = 144 only): for each row and level the reach update of tools/network_mc_cost.py and, for the
    level's pools, the clamp, torch.pow, the torch.where selects and the storage update, then index_add of the discharge into
    the inflow downstream; its gradient by autograd on the graph of one forward, built outside the timing.  The condition of
    DESIGN.md sections 12 - 17: at no shape where both were timed is the kernel's median above the torch statement's median by
    more than that statement's own max - min.
One JSON line per result."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lgar_py_amd.network import MC_RMAX, MC_RMIN, POOL_RMAX, POOL_RMIN, CatchmentNetwork, NetworkPools

args = sys.argv[1:]
quick = "quick" in args
OUT = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "r15", "network_pool_cost.jsonl")
REPS, WARM = 7, 2
DT = 1.0
SCALARS = (DT, MC_RMIN, MC_RMAX, POOL_RMIN, POOL_RMAX)


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


P0 = {}  # (op, network, B, T) -> the median at 0 % pools


def report(op, name, net, pools, share, T, ker, mc, ref=None, **more):
    med, mmed = ker[len(ker) // 2], mc[len(mc) // 2]
    both = int(((pools.pool_ptr > net.level_ptr[:-1]) & (pools.pool_ptr < net.level_ptr[1:])).sum())
    launches = int((pools.pool_ptr > net.level_ptr[:-1]).sum() + (pools.pool_ptr < net.level_ptr[1:]).sum())
    rec = {"mode": "network_pool_cost", "op": op, "network": name, "T": T, "B": net.B, "P": pools.P, "pool_share": share, "levels": net.n_levels,
           "levels_with_both_kinds": both, "launches": launches, "us_median": med, "us_min": ker[0], "us_max": ker[-1], "reps": REPS,
           "mc_us_median": mmed, "mc_us_min": mc[0], "mc_us_max": mc[-1], "ratio_to_route_mc": med / mmed,
           "library": os.environ.get("LGAR_LIB", "default")}
    key = (op, name, net.B, T)
    if share == 0.0:
        P0[key] = med
    elif key in P0 and both:
        rec["extra_us_per_level_with_both"] = (med - P0[key]) / both
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


def level_lists(net, pools):
    """per level and kind: the nodes, (pools: their slots,) the positions among them of those with a downstream node, and those
    downstream nodes"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = []
    for l in range(net.n_levels):
        kinds = []
        for a, b in ((net.level_ptr[l], pools.pool_ptr[l]), (pools.pool_ptr[l], net.level_ptr[l + 1])):
            bs = pools.order_host[a:b].astype(np.int64)
            if not bs.size:
                kinds.append(None)
                continue
            d = net.downstream_host[bs].astype(np.int64)
            has = np.nonzero(d >= 0)[0]
            kinds.append((dev(bs), dev(pools.pool_slot_host[bs].astype(np.int64)), dev(has) if has.size else None, dev(d[has]) if has.size else None))
        out.append(kinds)
    return out


def torch_statement(levels, x, kref, beta, X, qref, cq, m, s0, sref, smax, state):
    """y [T, B] by the plain statement (differentiable: no in-place operation on a tensor autograd needs)"""
    half = 0.5 * DT
    Iprev, Sprev = state[0], state[1]  # Sprev: Oprev at a reach, S at a pool
    cap = smax - s0
    rows = []
    for t in range(x.shape[0]):
        I, y, nxt = x[t], torch.zeros_like(x[0]), torch.zeros_like(x[0])
        for reaches, lakes in levels:
            if reaches is not None:
                bs, _, src, dst = reaches
                Op = Sprev[bs]
                K = kref[bs] * torch.pow(torch.clamp(Op / qref[bs], MC_RMIN, MC_RMAX), -beta[bs])
                KX = K * X[bs]
                u = K - KX
                D = u + half
                O = ((half - KX) / D * I[bs] + (half + KX) / D * Iprev[bs]) + (u - half) / D * Op
                y, nxt = y.index_copy(0, bs, O), nxt.index_copy(0, bs, O)
                if src is not None:
                    I = I.index_add(0, dst, O[src])
            if lakes is not None:
                bs, sl, src, dst = lakes
                a = Sprev[bs] - s0[sl]
                Ql = cq[sl] * torch.pow(torch.clamp(a / sref[sl], POOL_RMIN, POOL_RMAX), m[sl])
                av = a + half * (I[bs] + Iprev[bs])
                qa = av / DT
                Q = torch.where(Ql < qa, Ql, qa)
                Q = torch.where(Q < 0, torch.zeros_like(Q), Q)
                r = av - DT * Q
                ex = r - cap[sl]
                spill = ex > 0
                O = torch.where(spill, Q + ex / DT, Q)
                y, nxt = y.index_copy(0, bs, O), nxt.index_copy(0, bs, torch.where(spill, cap[sl], r) + s0[sl])
                if src is not None:
                    I = I.index_add(0, dst, O[src])
        rows.append(y)
        Iprev, Sprev = I, nxt
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
        # qref of a reach: the mean discharge it sees (its upstream area x the mean lateral inflow), so rho stays around 1
        area = net.accumulate(torch.ones(1, B, dtype=torch.float64, device="cuda"))[0]
        par = torch.stack([kref, beta, X, 0.5 * area]).contiguous()
        for share in (0.0, 0.01, 0.1):
            nodes = rng.permutation(B)[:max(1, int(round(share * B)))] if share else np.zeros(0, dtype=np.int64)
            pools = NetworkPools(net, nodes)
            P = pools.P
            at = torch.from_numpy(nodes.astype(np.int64)).cuda()
            # a pool releases the mean discharge it sees at a = sref, four hours of it, and spills just above that: the storage
            # hovers around smax and both branches are taken
            mean_q = 0.5 * area[at]
            ppar = torch.stack([mean_q, 1.2 + 0.6 * rand(P), 0.1 * mean_q, 4.0 * mean_q * DT, 4.1 * mean_q * DT]).contiguous()
            state = torch.stack([0.5 * torch.ones_like(area), 0.5 * area]).contiguous()
            state[1, at] = ppar[2] + ppar[3]
            for T in (144,) if quick else (144, 8760):
                x, gy = rand(T, B), rand(T, B)
                y, _, sg = net._forward_pool(x, pools, par, ppar, SCALARS, state, False, True)
                ym = net._forward_mc(x, par, DT, MC_RMIN, MC_RMAX, state, False)[0]
                spills = float((sg >= ppar[4] * (1.0 - 1e-12)).double().mean()) if P else 0.0
                kernel_fwd = lambda: net._forward_pool(x, pools, par, ppar, SCALARS, state, False, True)
                kernel_bwd = lambda: net._backward_pool(gy, x, y, sg, pools, par, ppar, SCALARS, state, True, True, True)
                mc_fwd = lambda: net._forward_mc(x, par, DT, MC_RMIN, MC_RMAX, state, False)
                mc_bwd = lambda: net._backward_mc(gy, x, ym, par, DT, MC_RMIN, MC_RMAX, state, True, True)
                if T == 144:
                    levels = level_lists(net, pools)
                    with torch.no_grad():
                        yt = torch_statement(levels, x, *par, *ppar, state)
                    err = float((yt - y).abs().max() / y.abs().max())
                    leaves = [v.clone().requires_grad_(True) for v in (x, par[0], par[1], par[2], ppar[0], ppar[1], ppar[2], ppar[4], state)]
                    graph = torch_statement(levels, leaves[0], leaves[1], leaves[2], leaves[3], par[3], leaves[4], leaves[5], leaves[6], ppar[3],
                                            leaves[7], leaves[8])
                    wanted = leaves if P else leaves[:4] + leaves[8:]

                    def torch_fwd():
                        with torch.no_grad():
                            torch_statement(levels, x, *par, *ppar, state)

                    ker, mc, ref = timed([kernel_fwd, mc_fwd, torch_fwd])
                    report("forward+storage", name, net, pools, share, T, ker, mc, ref, torch_max_rel_diff=err, rows_at_smax=spills)
                    ker, mc, ref = timed([kernel_bwd, mc_bwd, lambda: torch.autograd.grad(graph, wanted, gy, retain_graph=True)])
                    report("adjoint+gpar+gpool+gstate", name, net, pools, share, T, ker, mc, ref)
                    del graph, leaves, wanted, yt, levels
                else:
                    ker, mc = timed([kernel_fwd, mc_fwd])
                    report("forward+storage", name, net, pools, share, T, ker, mc, rows_at_smax=spills)
                    ker, mc = timed([kernel_bwd, mc_bwd])
                    report("adjoint+gpar+gpool+gstate", name, net, pools, share, T, ker, mc)
                del x, gy, y, ym, sg
                torch.cuda.empty_cache()
