"""TEST INFRASTRUCTURE ONLY: the numpy definition of the soil-moisture output, and the calls of the host program (post_host.run)
that run lgar_py_amd/csrc/lgar_moisture.hpp -- the per-column function of the GPU kernel -- over the same front tables.  Never
imported by the product package.
"""
import os

import numpy as np

from _hostbuild import ROOT
from lgar_py_amd._capi import MOIST_WHAT
from post_host import Out, dtype_code, same_bits  # noqa: F401


def _clip(x, a, b):
    x = np.where(x < a, a, x)
    return np.where(x > b, b, x)


def profile_ref(depth, theta, layer, n_fronts, thickness, edges=None, what="theta", sensitivity=False):
    """The definition (include/lgar.h, lgar_soil_moisture) as a numpy loop over front tables laid out like LgarEngine.fronts():
    depth / theta / layer [F, N], n_fronts [N], thickness [L, N]; edges [D + 1], or None for each column's own layers.
    Returns fp64 [D, N] ([L, N]): front by front, bin by bin, plain fp64 multiplies and adds in the kernel's order.
    sensitivity=True: instead of the profile, B = sum_j theta_j (|w_j| + |d_j| + |t_j|) per bin (w_j the clipped width) -- a relative
    error eps on every depth and theta moves a bin's storage by at most eps * B to first order (clip is 1-Lipschitz); for
    what="theta" B is divided by the bin's in-column width."""
    depth, theta, thickness = (np.asarray(a).astype(np.float64) for a in (depth, theta, thickness))
    L, N = thickness.shape
    cols = np.arange(N)
    top = np.zeros((L + 1, N))
    for l in range(L):
        top[l + 1] = top[l] + thickness[l]
    E = top if edges is None else np.repeat(np.asarray(edges, dtype=np.float64)[:, None], N, axis=1)
    D = E.shape[0] - 1
    S, prev_d, prev_k = np.zeros((D, N)), np.zeros(N), np.full(N, -1)
    for j in range(int(np.max(n_fronts, initial=0))):
        live = j < n_fronts
        k = np.minimum(np.asarray(layer[j]).astype(np.int64) & 0x7F, L - 1)
        t = np.where(k == prev_k, prev_d, top[k, cols])
        for i in range(D):
            w = _clip(depth[j], E[i], E[i + 1]) - _clip(t, E[i], E[i + 1])
            term = np.abs(theta[j]) * (np.abs(w) + np.abs(depth[j]) + np.abs(t)) if sensitivity else theta[j] * w
            S[i] = np.where(live, S[i] + term, S[i])
        prev_d, prev_k = np.where(live, depth[j], prev_d), np.where(live, k, prev_k)
    if what == "storage":
        return S
    w = _clip(top[L][None, :], E[:-1], E[1:]) - E[:-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w > 0, S / w, np.nan)


def tables(name, dtype=np.float64):
    """The reference's front table at every recorded step before its crash, one step per column: arrays laid out like
    LgarEngine.fronts() plus thickness [L, T], the total thickness Z and the recorded ending_volume [T]."""
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    crash = int(g["crash_step"])
    T = crash if crash >= 0 else g["forcing"].shape[0]
    lay = g["front_layer"][:T].T
    t = dict(depth=np.ascontiguousarray(g["fronts"][:T, :, 0].T.astype(dtype)),
             theta=np.ascontiguousarray(g["fronts"][:T, :, 1].T.astype(dtype)),
             layer=lay, flags=np.where(lay >= 0, lay, 0).astype(np.uint8), n_fronts=g["nfronts"][:T].astype(np.int32),
             thickness=np.repeat(g["thickness"].astype(dtype)[:, None], T, axis=1))
    F = min(t["depth"].shape[0], 32)  # (manyfronts_pulse_84 records 40 slots, 31 in use)
    assert int(t["n_fronts"].max()) <= F
    for k in ("depth", "theta", "layer", "flags"):
        t[k] = np.ascontiguousarray(t[k][:F])
    t["Z"] = float(np.cumsum(g["thickness"].astype(np.float64))[-1])
    t["volume"] = g["acc"][:T, 9]
    return t


def case(c):
    """c: a dict with depth / theta [F, N] (float32 or float64: the case's dtype), flags uint8 [F, N], n_fronts [N], thickness
    [L, N], edges ([D + 1] or None = layer bins), what.  The case of post_host.run that gives the [D, N] array in the case's dtype."""
    dt = np.asarray(c["depth"]).dtype
    F, N = c["depth"].shape
    L = c["thickness"].shape[0]
    edges = None if c.get("edges") is None else np.asarray(c["edges"], dtype=np.float64)
    out = Out(dt, L if edges is None else len(edges) - 1, N)
    arrays = [np.asarray(c[key]).astype(typ) for key, typ in (("thickness", dt), ("depth", dt), ("theta", dt), ("flags", np.uint8), ("n_fronts", np.int32))]
    return [("soil_moisture", [dtype_code(dt), L, F, N, out.shape[0], MOIST_WHAT[c["what"]]], arrays + [edges, out])], out
