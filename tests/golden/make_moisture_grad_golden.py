#!/usr/bin/env python3
"""Generate the soil-moisture gradient fixtures (tests/golden/moisture_grad/mgrad_<case>.npz) by running the LGAR-py reference itself.

As make_forcing_grad_golden.py: runs ONLY where the reference is present, imports it (and make_golden's recipe, and that script's
`clamp` shim) here and nowhere else, and commits nothing but the numbers it saves.  The five gradient cases that script names are
run again under enable_grad by the agent's call sequence.  At the recorded rows -- the state after every `every`-th row and after
the last -- the water of depth bins is built in torch from the model's own fronts,

    S_i = sum_j theta_j * (clamp(d_j, a, b) - clamp(t_j, a, b)),     t_j = d_{j-1} within a layer, else the layer's top,

for two bin sets (fixed edges [0, 5, 10, 30, 60, 100, Z + 50], and the column's own layers), and torch.autograd.grad gives
J = d S_i / d (alpha, n, ksat)[l] and dV of model.ending_volume: what lgar_soil_moisture_tangent is pinned to
(tests/test_moisture_tangent_host.py, tests/test_gpu_moisture_tangent.py).

The script asserts that the run is the one of the committed grad_* fixture (forcing equal, mean(runoff^2) equal to its loss),
that every parameter kind moves some bin (max |J| * parameter value >= 1e-6 cm), that the reference closes on itself
(|sum_i J_i - dV| <= 1e-9 max |dV| per kind over each covering bin set) and that no front whose depth depends on the parameters
lies exactly on an edge: torch.clamp passes gradients inclusively at ties, the library's definition is half-open (include/lgar.h),
and the fixtures must not depend on the difference.

Usage:  python tests/golden/make_moisture_grad_golden.py [case ...]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import numpy as np
import torch

import make_forcing_grad_golden as FG
import make_golden as MG

NAMES = FG.NAMES
EVERY = {"grad_synth0_12h": 3, "grad_manyfronts_60": 5}  # the others: 12
OUT = os.path.join(HERE, "moisture_grad")
KINDS = ("alpha", "n", "ksat")
CLOSURE = 1e-9


def every_of(name):
    return EVERY.get(name, 12)


def _fronts(model):
    """[(depth, theta, layer number)] top -> bottom"""
    out, layer = [], model.top_layer
    while layer is not None:
        out += [(wf.depth, wf.theta, int(wf.layer_num)) for wf in layer.wetting_fronts]
        layer = layer.next_layer
    return out


def _tensor(v):
    return v if torch.is_tensor(v) else torch.tensor(float(v))


def _bins(fronts, tops, edges):
    """S_i of every bin, and the (value, tensor) pairs of every depth and top that entered"""
    S = [torch.zeros(()) for _ in range(len(edges) - 1)]
    used = []
    prev_d, prev_k = None, -1
    for d, th, k in fronts:
        d, th = _tensor(d).reshape(()), _tensor(th).reshape(())
        t = prev_d if k == prev_k else torch.tensor(float(tops[k]))
        used += [d, t]
        for i in range(len(S)):
            a, b = float(edges[i]), float(edges[i + 1])
            S[i] = S[i] + th * (torch.clamp(d, min=a, max=b) - torch.clamp(t, min=a, max=b))
        prev_d, prev_k = d, k
    return S, used


def _jac(y, params):
    """d y / d (alpha, n, ksat)[l] as [3, L] (None -> 0)"""
    L = len(params[0])
    flat = [p for plist in params for p in plist]
    if not (torch.is_tensor(y) and y.requires_grad):
        return np.zeros((3, L))
    g = torch.autograd.grad(y, flat, retain_graph=True, allow_unused=True)
    return np.array([0.0 if v is None else float(v) for v in g]).reshape(3, L)


def run(name):
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(0)
    FG._shim_clamp()
    from dpLGAR.models.physics.MassBalance import MassBalance
    os.makedirs(OUT, exist_ok=True)
    kw = MG.CASES[name][1]
    cfg, x = FG._inputs(**kw)
    soil = kw["soil"]
    L = len(soil["thickness"])
    tops = np.concatenate([[0.0], np.cumsum(np.asarray(soil["thickness"], dtype=np.float64))])
    Z = float(tops[-1])
    edge_sets = {"fixed": np.array([0.0, 5.0, 10.0, 30.0, 60.0, 100.0, Z + 50.0]), "layers": tops.copy()}
    assert all((e[1:] > e[:-1]).all() for e in edge_sets.values()), name
    T = x.shape[0]
    every = every_of(name)
    rows = sorted(set(range(every - 1, T, every)) | {T - 1})
    model = MG.make_model(cfg, soil)
    params = (model.alpha, model.n, model.ksat)
    mb = MassBalance(cfg, model)
    runoffs = []
    rec = {k: dict(S=[], J=[]) for k in edge_sets}
    dV, V, nfr = [], [], []
    with torch.enable_grad():
        for i in range(T):
            runoff, _ = model(x[i])
            runoffs.append(runoff)
            if i in rows:
                fronts = _fronts(model)
                nfr.append(len(fronts))
                V.append(MG._f(model.ending_volume))
                dV.append(_jac(model.ending_volume, params))
                for key, edges in edge_sets.items():
                    S, used = _bins(fronts, tops, edges)
                    rec[key]["S"].append([float(s.detach()) for s in S])
                    rec[key]["J"].append([_jac(s, params) for s in S])
                    for v in used:  # a depth that depends on the parameters must not sit exactly on an edge
                        if float(v.detach()) in [float(e) for e in edges]:
                            assert not np.any(_jac(v, params)), "%s row %d: a moving front lies exactly on edge %r" % (name, i, float(v.detach()))
            mb.change_mass(model)
        y = torch.stack(runoffs)
        loss = torch.mean(y * y)
    old = np.load(os.path.join(HERE, name + ".npz"))
    assert np.array_equal(old["forcing"], x.detach().numpy()) and float(old["loss"]) == float(loss.detach()), name  # the same run
    dV = np.array(dV)                                       # [R, 3, L]
    pval = np.array([[float(p.detach()) for p in plist] for plist in params])  # [3, L]
    out = dict(rows=np.array(rows, dtype=np.int32), every=every, n_fronts=np.array(nfr, dtype=np.int32), forcing=x.detach().numpy(),
               dV=dV, V=np.array(V), loss=float(loss.detach()))
    report = []
    for key, edges in edge_sets.items():
        S, J = np.array(rec[key]["S"]), np.array(rec[key]["J"])  # [R, D], [R, D, 3, L]
        out.update({"edges_" + key: edges, "S_" + key: S, "J_" + key: J})
        assert np.allclose(S.sum(1), out["V"], rtol=1e-12, atol=0.0), name
        for ki, kind in enumerate(KINDS):
            moved = float(np.abs(J[:, :, ki, :] * pval[ki]).max())
            assert moved >= 1e-6, "%s: %s moves no bin of the %s set (%.3g cm)" % (name, kind, key, moved)
            miss = float(np.abs(J[:, :, ki, :].sum(1) - dV[:, ki, :]).max())
            scale = float(np.abs(dV[:, ki, :]).max())
            report.append("%s/%s closure %.2g" % (key, kind, miss / scale))
            assert miss <= CLOSURE * scale, "%s: the reference's own closure misses: %s %s %.3g of %.3g" % (name, key, kind, miss, scale)
    np.savez_compressed(os.path.join(OUT, "mgrad_" + name + ".npz"), **out)
    return "%s: T=%d rows=%s fronts<=%d  %s" % (name, T, rows, max(nfr), "  ".join(report))


if __name__ == "__main__":
    for nm in sys.argv[1:] or NAMES:
        print(run(nm), flush=True)
