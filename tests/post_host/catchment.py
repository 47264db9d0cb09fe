"""TEST INFRASTRUCTURE ONLY: the numpy statement of the catchment sums (include/lgar.h, lgar_catchment_sums; DESIGN.md section
10), and the calls of the host program (post_host.run) that run lgar_py_amd/csrc/lgar_catchment.hpp -- the per-lane
accumulation and combine order of the GPU kernel -- over the same data.  Never imported by the product package.
"""
import numpy as np

from post_host import Out, dtype_code, same_bits  # noqa: F401

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


def case(c):
    """c: a dict with series [T, N] (float32 or float64: the case's dtype), offsets [B + 1], and optionally order, weights [N],
    status [N], rows_per_wave (1, or 4: the kernel's row groups of many-catchment jobs), and for the spread ids [N] + grad
    [TG, B].  The case of post_host.run that gives (sums [T, B], weight_sums [B], spread [TG, N] in the case's dtype or None)."""
    series = np.asarray(c["series"])
    dt = series.dtype
    T, N = series.shape
    B = len(c["offsets"]) - 1
    i32 = lambda a: None if a is None else np.asarray(a, dtype=np.int32)
    order, w, st, grad = i32(c.get("order")), c.get("weights"), i32(c.get("status")), c.get("grad")
    assert w is None or np.asarray(w).dtype == dt
    sums, wsum, spread = Out(np.float64, T, B), Out(np.float64, B), None
    calls = [("catchment_sums", [dtype_code(dt), T, N, B, 0 if order is None else len(order), int(c.get("rows_per_wave", 1))],
              [series, i32(c["offsets"]), order, w, st, sums, wsum])]
    if grad is not None and len(grad):
        grad = np.asarray(grad, dtype=np.float64)
        spread = Out(dt, grad.shape[0], N)
        calls.append(("catchment_spread", [dtype_code(dt), grad.shape[0], B, N], [grad, i32(c["ids"]), w, st, spread]))
    return calls, (sums, wsum, spread)
