"""TEST INFRASTRUCTURE ONLY: the numpy statement of the catchment routing (include/lgar.h, lgar_catchment_route /
lgar_catchment_route_grad) -- the queue recurrence itself, row after row -- and the front-end of the
stand-alone host program (tests/route_host/route_host.cpp) that runs lgar_py_amd/csrc/lgar_route.hpp -- the fold without a
dependence between rows, the hand-over and the gradient accumulation of the GPU kernels -- compiled for the host with
-DLGAR_DEVSIM.  Never imported by the product package.
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

import _hostbuild
from _hostbuild import CSRC, ROOT

_HERE = os.path.dirname(os.path.abspath(__file__))
KMAX = 64  # LGAR_ROUTE_KMAX
SHAPE_B = (1, 63, 64, 65, 257)
SHAPE_K = (1, 2, 5, 8, 64)


def shape_T(K):
    return sorted({0, 1, K - 1, K, K + 1, 11})


def _per_catchment(g, B):
    """ordinates in the device layout, [K] (shared) or [K, B], as [K, B]"""
    g = np.asarray(g, dtype=np.float64)
    return np.repeat(g[:, None], B, axis=1) if g.ndim == 1 else g


def route_ref(x, g, q_in=None):
    """The definition as it is written: for every row t, q[i] += g[i] * x[t] for all i (one rounded product, one rounded add),
    y[t] = q[0], the queue shifts down and +0.0 enters at the top.  x [T, B], g [K] or [K, B], q_in [K, B] or None = zeros.
    Returns (y [T, B], q_out [K, B])."""
    x = np.asarray(x, dtype=np.float64)
    T, B = x.shape
    G = _per_catchment(g, B)
    K = G.shape[0]
    q = np.zeros((K, B)) if q_in is None else np.array(q_in, dtype=np.float64).reshape(K, B)
    y = np.zeros((T, B))
    with np.errstate(all="ignore"):
        for t in range(T):
            q = q + G * x[t][None, :]
            y[t] = q[0]
            q[:-1] = q[1:]
            q[-1] = 0.0
    return y, q


def adjoint_ref(gy, g):
    """gx[t] = the fold of g[k] * gy[t + k] from k = min(K - 1, T - 1 - t) down to 0 from +0.0: the recurrence over the rows in
    reverse order with a zero queue."""
    gy = np.asarray(gy, dtype=np.float64)
    return route_ref(gy[::-1], g)[0][::-1].copy()


def ordinate_grad_ref(x, gy, K):
    """gg[k, b] = sum_{t = k}^{T - 1} gy[t, b] * x[t - k, b], from +0.0 in increasing t, plain fp64 products and adds."""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    T, B = x.shape
    gg = np.zeros((K, B))
    with np.errstate(all="ignore"):
        for t in range(T):
            k = np.arange(min(t, K - 1) + 1)
            gg[k] = gg[k] + gy[t][None, :] * x[t - k]
    return gg


def dense_conv(x, g):
    """The convolution by numpy's own arithmetic in another order (k upward), for bounds: y[t] = sum_k g[k] x[t - k]."""
    T, B = x.shape
    G = _per_catchment(g, B)
    y = np.zeros((T, B))
    for k in range(min(G.shape[0], T)):
        y[k:] += G[k][None, :] * x[:T - k]
    return y


def same_bits(a, b):
    """Bit-for-bit equality of two fp64 arrays (NaNs must sit in the same places)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float64 or b.dtype != np.float64:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint64)[~na] == b.view(np.uint64)[~nb]).all())


def mixed_data(rng, T, B, K, per):
    """x, gy [T, B], g ([K, B] or [K]) and q_in [K, B] of mixed signs over several decades, with a NaN and a -0.0 in x (in its
    first and last rows where there are any) and a -0.0 ordinate."""
    def draw(*shape):
        return (rng.random(shape) - 0.4) * 10.0 ** rng.integers(-3, 3, shape)
    x, gy, q_in = draw(T, B), draw(T, B), draw(K, B)
    g = draw(K, B) if per else draw(K)
    if T:
        x[0, B // 2] = -0.0
        x[T - 1, 0] = np.nan
        if T > 2:
            x[1, B - 1] = -0.0
    if per:
        g[K - 1, ::3] = -0.0
    q_in[0, B - 1] = -0.0
    return x, gy, g, q_in


def program(sanitize=False):
    """The host program, built on first use with the ROCm clang (sanitize: AddressSanitizer + UBSan, any finding aborts)."""
    return _hostbuild.build(os.path.join(_HERE, "route_host_san" if sanitize else "route_host"),
                            os.path.join(_HERE, "route_host.cpp"),
                            [os.path.join(CSRC, "lgar_route.hpp"), os.path.join(ROOT, "include", "lgar.h")],
                            _hostbuild.SANITIZE if sanitize else [], "the catchment-routing host program")


MODES = {"forward": 0, "reverse": 1, "grad": 2}


def run_cases(cases, sanitize=False):
    """cases: dicts with mode ("forward", "reverse" or "grad"), x [T, B]; forward / reverse: g ([K] shared or [K, B]) and, forward
    only, optionally q_in [K, B]; grad: gy [T, B] and K.  Returns per case (y, q_out), (y, None) or (g_out, None)."""
    exe = program(sanitize)
    blob, shapes = [struct.pack("i", len(cases))], []
    for c in cases:
        x = np.ascontiguousarray(c["x"], dtype=np.float64)
        T, B = x.shape
        mode = MODES[c["mode"]]
        if mode == 2:
            K, per, q_in = int(c["K"]), 0, None
        else:
            g = np.ascontiguousarray(c["g"], dtype=np.float64)
            K, per, q_in = g.shape[0], int(g.ndim == 2), c.get("q_in")
            assert g.ndim == 1 or g.shape == (K, B)
        blob.append(struct.pack("6i", mode, T, B, K, per, int(q_in is not None)))
        blob.append(x.tobytes())
        if mode == 2:
            gy = np.ascontiguousarray(c["gy"], dtype=np.float64)
            assert gy.shape == (T, B)
            blob.append(gy.tobytes())
        else:
            blob.append(g.tobytes())
            if q_in is not None:
                q_in = np.ascontiguousarray(q_in, dtype=np.float64)
                assert q_in.shape == (K, B)
                blob.append(q_in.tobytes())
        shapes.append((mode, T, B, K))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(b"".join(blob))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0 and not p.stderr.strip(), (p.returncode, p.stderr[-4000:])
        raw = open(fout, "rb").read()
    res, at = [], 0

    def take(*shape):
        nonlocal at
        n = int(np.prod(shape)) * 8
        a = np.frombuffer(raw[at:at + n], dtype=np.float64).reshape(shape).copy()
        at += n
        return a

    for mode, T, B, K in shapes:
        if mode == 0:
            res.append((take(T, B), take(K, B)))
        elif mode == 1:
            res.append((take(T, B), None))
        else:
            res.append((take(K, B), None))
    assert at == len(raw)
    return res
