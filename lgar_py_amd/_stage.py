"""What the catchment stages (baseflow, snow, network, scores) share on the host: the argument checks with their one wording each,
the parameter blocks, the tail of a backward pass and the carried state.  Plain functions: a stage calls what it needs and keeps
its own launches.  Private: not exported from the package.
"""
import math

import numpy as np
import torch

from ._capi import LgarError


def time_step(dt_h):
    try:
        dt = float(dt_h)
    except (TypeError, ValueError) as err:
        raise LgarError("dt_h must be a number of hours (%s)" % err)
    if not math.isfinite(dt) or dt <= 0.0:
        raise LgarError("dt_h must be finite and > 0 hours (got %r)" % (dt_h,))
    return dt


def ratio_range(lo, hi, names):
    """(lo, hi) as floats, the range a ratio is held to: 2^-60 <= lo <= hi <= 2^60; names: what the two are called."""
    try:
        a, b = float(lo), float(hi)
    except (TypeError, ValueError) as err:
        raise LgarError("%s, %s must be numbers (%s)" % (*names, err))
    if not (2.0 ** -60 <= a <= b <= 2.0 ** 60):
        raise LgarError("%s, %s must satisfy 2^-60 <= %s <= %s <= 2^60 (got %r, %r)" % (*names, *names, lo, hi))
    return a, b


def matrix(x, what, B, device, rows=None, shown=None):
    """A fp64 [T, B] (rows=None) or [rows, B] tensor on `device`, detached and contiguous; anything else raises.  shown: the
    device as the message names it (the caller's own spelling), default `device`."""
    if (not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != B or x.dtype != torch.float64 or x.device != device
            or (rows is not None and x.shape[0] != rows)):
        raise LgarError("%s must be a fp64 [%s, %d] tensor on %s" % (what, "T" if rows is None else rows, B, shown or device))
    if x.shape[0] >= 2 ** 31:
        raise LgarError("at most 2^31 - 1 rows")
    return x.detach().contiguous()


def state_block(x, what, shape, device, note=""):
    """A fp64 tensor of exactly `shape` on `device`, detached and contiguous; note: what its rows are, for the message."""
    if not isinstance(x, torch.Tensor) or tuple(x.shape) != tuple(shape) or x.dtype != torch.float64 or x.device != device:
        raise LgarError("%s must be a fp64 [%s] tensor%s on %s" % (what, ", ".join("%d" % n for n in shape), note, device))
    return x.detach().contiguous()


def rows_on_device(names, values, n, device, shown=None):
    """Every value as a fp64 tensor on `device`, [n] or 0-d (a number becomes 0-d: the caller expands, and still sees which
    were scalars); anything else raises."""
    rows = []
    for name, v in zip(names, values):
        if not isinstance(v, torch.Tensor):
            try:
                v = torch.tensor(float(v), dtype=torch.float64, device=device)
            except (TypeError, ValueError) as err:
                raise LgarError("%s must be a fp64 [%d] tensor or a scalar (%s)" % (name, n, err))
        if v.dtype != torch.float64 or v.device != device or v.dim() > 1 or (v.dim() == 1 and v.shape[0] != n):
            raise LgarError("%s must be a fp64 [%d] tensor or a scalar on %s" % (name, n, shown or device))
        rows.append(v)
    return rows


def block_on_host(names, values, n_given, noun):
    """(par [k, n] fp64 numpy, n) from k values that are [n] tensors, sequences or scalars; n_given: n for scalars only (None:
    the vectors say); noun: what the n entries are ("catchment", "cell")."""
    cols = []
    for name, v in zip(names, values):
        if isinstance(v, torch.Tensor):
            if v.dtype != torch.float64:
                raise LgarError("%s must be fp64 (got %s)" % (name, v.dtype))
            v = v.detach().cpu().numpy()
        try:
            v = np.asarray(v, dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise LgarError("%s must be numbers (%s)" % (name, err))
        if v.ndim > 1:
            raise LgarError("%s must be a scalar or [B], one entry per %s (got shape %s)" % (name, noun, tuple(v.shape)))
        cols.append(v)
    sizes = {int(v.shape[0]) for v in cols if v.ndim == 1}
    if n_given is not None:
        sizes.add(int(n_given))
    if len(sizes) != 1:
        raise LgarError("%s must agree on one number of %ss: [B] each, or scalars with n_catchments= (got %s)"
                        % (", ".join(names), noun, sorted(sizes) or "scalars only"))
    n = sizes.pop()
    if not 0 <= n < 2 ** 31:
        raise LgarError("0 .. 2^31 - 1 %ss (got %d)" % (noun, n))
    return np.stack([np.broadcast_to(v, (n,)) for v in cols]).astype(np.float64), n


def check_rules(par, rules, mask=None, of="", where=None):
    """par: [k, n] numpy; rules: per row (name, ok, text), ok(row, par) -> bool [n] (it sees the whole block: a rule may compare
    rows).  The first entry of a row that breaks its rule raises, rows in order.  mask: bool [n], the entries that are read at
    all; of: what the entries belong to (" of a reach"); where(i): a note on entry i."""
    for row, (name, ok, text) in zip(par, rules):
        bad = np.nonzero(~ok(row, par) if mask is None else ~ok(row, par) & mask)[0]
        if bad.size:
            i = bad[0]
            raise LgarError("%s[%d] = %r%s: every %s%s must be %s" % (name, i, float(row[i]), where(i) if where else "", name, of, text))


def scalar_grads(block, needs, was_scalar):
    """The gradients of k parameters from the [k, n] block a backward launch wrote (None when no parameter needs one): row k, summed
    where the parameter was a scalar, None where it needs none."""
    return [(block[k].sum() if was_scalar[k] else block[k]) if need else None for k, need in enumerate(needs)]


def carried(states, carry, key, state, forward, at=-1):
    """The outputs of forward(state_in, want_state), entry `at` of which is state_out.  carry: starts from `state` if given, else
    from states[key] (absent: None, zeros), and keeps state_out there; otherwise starts from `state` and keeps nothing."""
    if not carry:
        return forward(state, False)
    out = forward(states.get(key) if state is None else state, True)
    states[key] = out[at]
    return out
