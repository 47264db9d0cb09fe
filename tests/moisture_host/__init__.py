"""TEST INFRASTRUCTURE ONLY: the numpy definition of the soil-moisture output and the front-end of the stand-alone host program
(tests/moisture_host/moisture_host.cpp) that runs lgar_py_amd/csrc/lgar_moisture.hpp -- the per-column function of the GPU
kernel -- compiled for the host with -DLGAR_DEVSIM.  Never imported by the product package.
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

import _hostbuild
from _hostbuild import CSRC, ROOT

_HERE = os.path.dirname(os.path.abspath(__file__))
WHAT = {"theta": 0, "storage": 1}


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


def same_bits(a, b):
    """Bit-for-bit equality of two float arrays (NaNs must sit in the same places)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(u)[~na] == b.view(u)[~nb]).all())


def program(sanitize=False):
    """The host program, built on first use with the ROCm clang (sanitize: AddressSanitizer + UBSan, any finding aborts)."""
    return _hostbuild.build(os.path.join(_HERE, "moisture_host_san" if sanitize else "moisture_host"),
                            os.path.join(_HERE, "moisture_host.cpp"),
                            [os.path.join(CSRC, "lgar_moisture.hpp"), os.path.join(ROOT, "include", "lgar.h")],
                            _hostbuild.SANITIZE if sanitize else [], "the soil-moisture host program")


def run_cases(cases, sanitize=False):
    """cases: dicts with depth / theta [F, N] (float32 or float64: the case's dtype), flags uint8 [F, N], n_fronts [N],
    thickness [L, N], edges ([D + 1] or None = layer bins), what.  Returns one [D, N] array per case, in the case's dtype."""
    exe = program(sanitize)
    blob, shapes = [struct.pack("i", len(cases))], []
    for c in cases:
        dt = np.asarray(c["depth"]).dtype
        assert dt in (np.float32, np.float64)
        F, N = c["depth"].shape
        L = c["thickness"].shape[0]
        layer_bins = c.get("edges") is None
        nb = L if layer_bins else len(c["edges"]) - 1
        blob.append(struct.pack("7i", int(dt == np.float64), L, F, N, nb, int(layer_bins), WHAT[c["what"]]))
        for key, typ in (("thickness", dt), ("depth", dt), ("theta", dt), ("flags", np.uint8), ("n_fronts", np.int32)):
            blob.append(np.ascontiguousarray(np.asarray(c[key]).astype(typ)).tobytes())
        if not layer_bins:
            blob.append(np.asarray(c["edges"], dtype=np.float64).tobytes())
        shapes.append((dt, nb, N))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(b"".join(blob))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0 and not p.stderr.strip(), (p.returncode, p.stderr[-4000:])
        raw = open(fout, "rb").read()
    res, at = [], 0
    for dt, nb, N in shapes:
        n = nb * N * np.dtype(dt).itemsize
        res.append(np.frombuffer(raw[at:at + n], dtype=dt).reshape(nb, N).copy())
        at += n
    assert at == len(raw)
    return res
