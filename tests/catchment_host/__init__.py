"""TEST INFRASTRUCTURE ONLY: the numpy statement of the catchment sums (include/lgar.h, lgar_catchment_sums; DESIGN.md section
10) and the front-end of the stand-alone host program (tests/catchment_host/catchment_host.cpp) that runs
lgar_py_amd/csrc/lgar_catchment.hpp -- the per-lane accumulation and combine order of the GPU kernel -- compiled for the host
with -DLGAR_DEVSIM.  Never imported by the product package.
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

import _hostbuild
from _hostbuild import CSRC, ROOT

_HERE = os.path.dirname(os.path.abspath(__file__))
FAULT_MASK = 0x7F  # LGAR_ST_FAULT_MASK
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)  # members per catchment: around the lane count and the partial count; N = 2121
# ... and beyond 1024 members, where a lane of the one-row kernel takes whole blocks of 16 loads (1024 members a block): two
# blocks and a ragged tail, exactly one block, one block and one member, just short of a block
BIG_SIZES = (2500, 1024, 1025, 1023)
_LANE = np.arange(64)


def members_of(offsets, order, b, n_columns):
    """Column indices of catchment b in map order, by the memory-safety rule of the definition: offsets clamped into [0, len]
    (len = the order array's length, or n_columns without one), an end not beyond its start = empty."""
    length = n_columns if order is None else len(order)
    if n_columns <= 0:
        length = 0
    lo = min(max(int(offsets[b]), 0), length)
    hi = min(max(int(offsets[b + 1]), 0), length)
    pos = np.arange(lo, max(hi, lo), dtype=np.int64)
    return pos if order is None else np.asarray(order, dtype=np.int64)[pos]


def combine(terms, keep):
    """terms [T, n] fp64, keep [n] bool -> [T]: the 256 partials (p = i mod 256, each from +0.0 in increasing i, a skipped member
    adds nothing), the pair sums q_l = (s_l + s_{l+64}) + (s_{l+128} + s_{l+192}) and the xor butterfly; q_0."""
    T, n = terms.shape
    s = np.zeros((T, 256))
    for i0 in range(0, n, 256):
        k = min(256, n - i0)
        with np.errstate(all="ignore"):
            added = s[:, :k] + terms[:, i0:i0 + k]
        s[:, :k] = np.where(keep[None, i0:i0 + k], added, s[:, :k])
    q = (s[:, 0:64] + s[:, 64:128]) + (s[:, 128:192] + s[:, 192:256])
    for off in (32, 16, 8, 4, 2, 1):
        q = q + q[:, _LANE ^ off]
    return q[:, 0]


def sums_ref(series, offsets, order=None, weights=None, status=None):
    """The definition as a plain loop: series [T, N] (float32 or float64), offsets [B + 1], order (column indices) or None,
    weights [N] in the series' dtype or None, status int32 [N] or None.  Returns (fp64 [T, B], fp64 [B] weight sums)."""
    series = np.asarray(series)
    T, N = series.shape
    B = len(offsets) - 1
    out, wsum = np.zeros((T, B)), np.zeros(B)
    for b in range(B):
        c = members_of(offsets, order, b, N)
        keep = (c >= 0) & (c < N)
        at = np.where(keep, c, 0)
        if N == 0:
            continue
        if status is not None:
            keep &= (np.asarray(status)[at] & FAULT_MASK) == 0
        w = np.ones(len(c)) if weights is None else np.asarray(weights)[at].astype(np.float64)
        with np.errstate(all="ignore"):
            out[:, b] = combine(w[None, :] * series[:, at].astype(np.float64), keep)
        wsum[b] = combine(w[None, :], keep)[0]
    return out, wsum


def spread_ref(grad, ids, weights, status, dtype):
    """out[t, c] = grad[t, ids[c]] * (double)w[c] rounded once to dtype; 0 for ids outside [0, B) and flagged columns."""
    grad = np.asarray(grad, dtype=np.float64)
    T, B = grad.shape
    ids = np.asarray(ids, dtype=np.int64)
    live = (ids >= 0) & (ids < B)
    if status is not None:
        live &= (np.asarray(status) & FAULT_MASK) == 0
    w = np.ones(len(ids)) if weights is None else np.asarray(weights).astype(np.float64)
    out = np.zeros((T, len(ids)), dtype=dtype)
    if B:
        out[:, live] = (grad[:, ids[live]] * w[None, live]).astype(dtype)
    return out


def sized_ids(sizes=SIZES, permute=None):
    """Catchment ids for catchments of the given sizes, contiguous (non-decreasing) or, with a seed, randomly permuted."""
    ids = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    return ids if permute is None else ids[np.random.default_rng(permute).permutation(len(ids))]


def csr_of(ids, B):
    """(offsets int32 [B + 1], order int32 or None) of an id per column: what CatchmentMap must produce -- a stable sort by
    id, -1 = no catchment, order None when the ids are non-decreasing with no -1."""
    ids = np.asarray(ids, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(ids[ids >= 0], minlength=B))]).astype(np.int32)
    if (ids >= 0).all() and (np.diff(ids) >= 0).all():
        return offsets, None
    order = np.array([c for b in range(B) for c in np.nonzero(ids == b)[0]], dtype=np.int32)
    return offsets, order


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
    return _hostbuild.build(os.path.join(_HERE, "catchment_host_san" if sanitize else "catchment_host"),
                            os.path.join(_HERE, "catchment_host.cpp"),
                            [os.path.join(CSRC, "lgar_catchment.hpp"), os.path.join(ROOT, "include", "lgar.h")],
                            _hostbuild.SANITIZE if sanitize else [], "the catchment-sums host program")


def run_cases(cases, sanitize=False):
    """cases: dicts with series [T, N] (float32 or float64: the case's dtype), offsets [B + 1], and optionally order, weights
    [N], status [N], rows_per_wave (1, or 4: the kernel's row groups of many-catchment jobs), and for the spread ids [N] + grad
    [TG, B].  Returns per case (sums [T, B], weight_sums [B], spread
    [TG, N] in the case's dtype or None)."""
    exe = program(sanitize)
    blob, shapes = [struct.pack("i", len(cases))], []
    for c in cases:
        series = np.asarray(c["series"])
        dt = series.dtype
        assert dt in (np.float32, np.float64)
        T, N = series.shape
        B = len(c["offsets"]) - 1
        order, w, st, grad = c.get("order"), c.get("weights"), c.get("status"), c.get("grad")
        TG = 0 if grad is None else np.asarray(grad).shape[0]
        blob.append(struct.pack("9i", int(dt == np.float64), T, N, B, -1 if order is None else len(order), int(w is not None),
                                int(st is not None), TG, int(c.get("rows_per_wave", 1))))
        blob.append(np.ascontiguousarray(series).tobytes())
        blob.append(np.asarray(c["offsets"], dtype=np.int32).tobytes())
        if order is not None:
            blob.append(np.asarray(order, dtype=np.int32).tobytes())
        if w is not None:
            assert np.asarray(w).dtype == dt
            blob.append(np.ascontiguousarray(w).tobytes())
        if st is not None:
            blob.append(np.asarray(st, dtype=np.int32).tobytes())
        if TG:
            blob.append(np.asarray(c["ids"], dtype=np.int32).tobytes())
            blob.append(np.ascontiguousarray(np.asarray(grad, dtype=np.float64)).tobytes())
        shapes.append((dt, T, N, B, TG))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(b"".join(blob))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0 and not p.stderr.strip(), (p.returncode, p.stderr[-4000:])
        raw = open(fout, "rb").read()
    res, at = [], 0

    def take(dtype, *shape):
        nonlocal at
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = np.frombuffer(raw[at:at + n], dtype=dtype).reshape(shape).copy()
        at += n
        return a

    for dt, T, N, B, TG in shapes:
        res.append((take(np.float64, T, B), take(np.float64, B), take(dt, TG, N) if TG else None))
    assert at == len(raw)
    return res
