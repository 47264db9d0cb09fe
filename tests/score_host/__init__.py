"""TEST INFRASTRUCTURE ONLY: the host build of the catchment-score header (lgar_py_amd/csrc/lgar_score.hpp, compiled for the
host with -DLGAR_DEVSIM) and its front-end.  score_host.hpp holds the host-side launchers of the three entry points;
score_host.cpp is the stand-alone program around them (run() below; also built with AddressSanitizer + UBSan), libscorehost.so
the same header as a shared library (library(): what SimCatchmentScore puts behind the product's calling surface).  The numpy
statement of the definition (include/lgar.h, lgar_catchment_moments / lgar_catchment_moments_grad) --
moments_ref and grad_ref, plain loops over blocks and rows -- and the data of the tests' cases live here too.
The build, the program's call records (tests/_hostprog.hpp) and same_bits are tests/_hostbuild.py's: UNIT below.
Never imported by the product package.
"""
import ctypes as C
import os

import numpy as np

import _hostbuild
from _hostbuild import Out, same_bits  # noqa: F401
from lgar_py_amd.scores import CatchmentScore

_HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK, NMOM = 64, 7  # LGAR_SCORE_BLOCK, LGAR_SCORE_NMOM
SHAPE_B = (1, 63, 64, 65, 257)
SHAPE_TO = (0, 1, 63, 64, 65, 129)
SHAPE_WINDOW = (1, 3, 12)
GAPS = ("none", "random", "missing", "one_valid", "block", "inf")


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------
def agg_ref(sim, window):
    """s[j] = (((0.0 + sim[j r]) + sim[j r + 1]) + ...) / (double)r"""
    sim = np.asarray(sim, dtype=np.float64)
    To, B = sim.shape[0] // window, sim.shape[1]
    assert sim.shape[0] == To * window
    s = np.zeros((To, B))
    with np.errstate(all="ignore"):
        for i in range(window):
            s = s + sim[i::window]
        return s / float(window)


def fold_ref(x, valid):
    """The gated fold over the rows: blocks of 64 rows, a block partial from +0.0 over its valid rows in increasing j (an invalid
    row adds nothing), the result from +0.0 over the block partials in increasing k."""
    To, B = valid.shape
    x = np.broadcast_to(x, (To, B))
    res = np.zeros(B)
    with np.errstate(all="ignore"):
        for k in range((To + BLOCK - 1) // BLOCK):
            part = np.zeros(B)
            for j in range(k * BLOCK, min(k * BLOCK + BLOCK, To)):
                part = np.where(valid[j], part + x[j], part)
            res = res + part
    return res


def moments_ref(sim, obs, window=1):
    """moments [7, B] of sim [To * window, B] against obs [To, B]: two passes, means first."""
    o = np.asarray(obs, dtype=np.float64)
    valid = np.isfinite(o)
    s = agg_ref(sim, window)
    with np.errstate(all="ignore"):
        n = fold_ref(np.ones_like(o), valid)
        mo, ms = fold_ref(o, valid) / n, fold_ref(s, valid) / n
        d_o, d_s, e = o - mo[None, :], s - ms[None, :], s - o
        return np.stack([n, mo, ms, fold_ref(d_o * d_o, valid), fold_ref(d_s * d_s, valid), fold_ref(d_o * d_s, valid), fold_ref(e * e, valid)])


def grad_ref(sim, obs, window, moments, coef):
    """grad_sim [To * window, B]: g = ((c0 / n + (2 c1)(s - ms)) + c2 (o - mo)) + (2 c3)(s - o), g / (double)r on each of the r rows
    under a valid observation row, +0.0 under a gap."""
    o = np.asarray(obs, dtype=np.float64)
    valid = np.isfinite(o)
    s = agg_ref(sim, window)
    n, mo, ms = (moments[i][None, :] for i in range(3))
    c0, c1, c2, c3 = (np.asarray(coef, dtype=np.float64)[i][None, :] for i in range(4))
    with np.errstate(all="ignore"):
        g = ((c0 / n + (2.0 * c1) * (s - ms)) + c2 * (o - mo)) + (2.0 * c3) * (s - o)
        return np.repeat(np.where(valid, g / float(window), 0.0), window, axis=0)


# ---- the plain torch statement and the bar of a gradient compared with its autograd ---------------------------------------------
U = 2.0 ** -53  # unit roundoff of fp64


def plain_moments(sim, obs, window):
    """The masked plain torch statement: isfinite mask, where, two masked passes.  sim [To * window, B], obs [To, B] -> [7, B];
    differentiable with respect to sim.  (No catchment may be empty: its means are 0 / 0.)"""
    import torch
    To, B = obs.shape
    valid = torch.isfinite(obs)
    o = torch.where(valid, obs, torch.zeros_like(obs))
    s = sim.reshape(To, window, B).mean(dim=1)
    zero = torch.zeros_like(s)
    n = valid.sum(dim=0).to(torch.float64)
    mo, ms = o.sum(dim=0) / n, torch.where(valid, s, zero).sum(dim=0) / n
    d_o, d_s, e = torch.where(valid, o - mo, zero), torch.where(valid, s - ms, zero), torch.where(valid, s - o, zero)
    return torch.stack([n, mo, ms, (d_o * d_o).sum(dim=0), (d_s * d_s).sum(dim=0), (d_o * d_s).sum(dim=0), (e * e).sum(dim=0)])


def gradient_bar(per_catchment, sim, obs, window, moments):
    """The bar on |d F / d sim, kernels - torch autograd of plain_moments|, F = the sum over catchments of
    per_catchment(moments of the catchment, [7, 1]) -> [1]; sim [To * window, B], obs [To, B], moments [7, B]: CPU fp64 tensors,
    no empty catchment.  Returns a numpy [To * window, B] array, 0 under gaps.

    Both sides evaluate g = c0 / n + 2 c1 (s - ms) + c2 (o - mo) + 2 c3 (s - o) with c = d F / d (ms, sss, sos, see) at moments
    that are the same sums in two orders.  A moment is a sum of n terms, each the result of at most window + 5 rounded
    operations (the window's adds and its division, two subtractions, a product), so each side is within
    dm_k = (n + window + 5) u sum |terms| of the exact value to first order (Higham 3.1; the shift of the centred sums under an
    error of the means is of second order: they are stationary in them), and the two sides within 2 dm_k of each other.  That
    forward error of the sums reaches g through the metric's sensitivity at these inputs, J[j, b, k] = d g[j, b] / d moment_k
    (autograd of the formula itself, second derivatives of the metric included); evaluating g is at most window + 12 more
    rounded operations on either side, on terms of magnitude A = |c0 / n| + 2 |c1 (s - ms)| + |c2 (o - mo)| + 2 |c3 (s - o)|:
        bar[j, b] = sum_k |J[j, b, k]| 2 dm_k[b] + 2 (window + 12) u A[j, b],     each of the window's rows gets bar / window."""
    import torch
    To, B = obs.shape
    valid = torch.isfinite(obs)
    o = torch.where(valid, obs, torch.zeros_like(obs))
    s = torch.from_numpy(agg_ref(sim.numpy(), window))
    n, mo, ms = moments[0], moments[1], moments[2]
    absfold = lambda x: torch.where(valid, x.abs(), torch.zeros_like(x)).sum(dim=0)
    terms = torch.stack([torch.zeros_like(n), absfold(o) / n, absfold(s) / n, moments[3], moments[4], absfold((o - mo) * (s - ms)), moments[6]])
    dm = (n + window + 5) * U * terms

    def g_of(mom, b):
        if not mom.requires_grad:
            mom = mom.clone().requires_grad_(True)
        c, = torch.autograd.grad(per_catchment(mom[:, None]).sum(), mom, create_graph=True)
        return (c[2] / mom[0] + 2.0 * c[4] * (s[:, b] - mom[2])) + c[5] * (o[:, b] - mom[1]) + 2.0 * c[6] * (s[:, b] - o[:, b]), c

    bar = torch.zeros(To, B, dtype=torch.float64)
    for b in range(B):
        J = torch.autograd.functional.jacobian(lambda x: g_of(x, b)[0], moments[:, b].clone())  # [To, 7]
        c = g_of(moments[:, b].clone(), b)[1].detach()
        A = (c[2] / n[b]).abs() + 2 * (c[4] * (s[:, b] - ms[b])).abs() + (c[5] * (o[:, b] - mo[b])).abs() + 2 * (c[6] * (s[:, b] - o[:, b])).abs()
        bar[:, b] = (J.abs() * 2 * dm[:, b][None, :]).sum(dim=1) + 2 * (window + 12) * U * A
    return np.repeat(torch.where(valid, bar, torch.zeros_like(bar)).numpy() / window, window, axis=0)


# ---- data ------------------------------------------------------------------------------------------------------------------
def mixed_data(rng, To, B, window, gaps):
    """sim [To * window, B] and obs [To, B] of mixed signs over several decades with -0.0 in sim, coef [4, B], and the gap pattern
    `gaps`: none; random (20 %); missing (catchment B // 2 wholly missing, 20 % elsewhere); one_valid (catchment B // 2 has
    exactly one valid row); block (rows 64 .. 127, one whole block, missing in catchment B - 1; To <= 64: its only block);
    inf (+inf and -inf as gaps beside NaN)."""
    def draw(*shape):
        return (rng.random(shape) - 0.4) * 10.0 ** rng.integers(-3, 3, shape)
    sim, obs, coef = draw(To * window, B), draw(To, B), draw(4, B)
    if To:
        sim[0, B // 2] = -0.0
        sim[To * window - 1, 0] = -0.0
    if gaps in ("random", "missing", "inf"):
        obs[rng.random((To, B)) < 0.2] = np.nan
    if gaps == "missing":
        obs[:, B // 2] = np.nan
    if gaps == "one_valid" and To:
        keep = obs[To // 2, B // 2]
        obs[:, B // 2] = np.nan
        obs[To // 2, B // 2] = keep
    if gaps == "block":
        obs[(BLOCK if To > BLOCK else 0):2 * BLOCK, B - 1] = np.nan
    if gaps == "inf" and To:
        obs[rng.random((To, B)) < 0.1] = np.inf
        obs[rng.random((To, B)) < 0.1] = -np.inf
        obs[0, 0] = np.inf
        obs[To - 1, B - 1] = -np.inf
    return sim, obs, coef


# ---- the host build --------------------------------------------------------------------------------------------------------
UNIT = _hostbuild.HostUnit(_HERE, "score_host", "scorehost", ["lgar_score.hpp"], "catchment-score")


def library():
    """libscorehost.so: scorehost_<entry point>(the arguments of include/lgar.h without the stream), loaded once."""
    i32, vp = C.c_int32, C.c_void_p
    return UNIT.library({"catchment_moments_workspace": [i32, i32], "catchment_moments": [vp, vp, i32, i32, i32, vp, vp],
                         "catchment_moments_grad": [vp, vp, i32, i32, i32, vp, vp, vp]}, {"catchment_moments_workspace": C.c_int64})


def run(cases, sanitize=False):
    """ONE run of the host program over every case: ("moments", sim, obs, window) gives moments [7, B];
    ("grad", sim, obs, window, moments, coef) gives grad_sim [To * window, B]."""
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    calls, results = [], []
    for op, sim, obs, window, *rest in cases:
        sim, obs = f64(sim), f64(obs)
        To, B = obs.shape
        assert sim.shape == (To * window, B) and op in ("moments", "grad")
        if op == "grad":
            moments, coef = f64(rest[0]), f64(rest[1])
            assert moments.shape == (NMOM, B) and coef.shape == (4, B)
            results.append(Out(np.float64, To * window, B))
            calls.append((1, (To, B, window), (), (sim, obs, moments, coef, results[-1])))
        else:
            results.append(Out(np.float64, NMOM, B))
            calls.append((0, (To, B, window), (), (sim, obs, results[-1])))
    UNIT.run_calls(calls, sanitize)
    return [r.value for r in results]


class SimCatchmentScore(CatchmentScore):
    """lgar_py_amd.scores.CatchmentScore (device="cpu") with the host build of the score kernels in the library's place."""

    def __init__(self, observations, window=1, warmup=0):
        super().__init__(observations, window=window, warmup=warmup, device="cpu")

    def _open(self):
        # (the workspace function has no stream)
        return _hostbuild.AsHipLibrary(("", "scorehost", library), hook=lambda name, fn: fn if name.endswith("_workspace") else None)
