"""Catchment baseflow: a groundwater store per catchment, fed by percolation, with its adjoint and parameter gradients.

Percolation leaves the bottom of every column; summed per catchment (catchment_sum) it recharges groundwater, and groundwater
returns to the channel as baseflow -- between events the whole hydrograph.  CatchmentBaseflow holds the three parameters of the
exponential storage-discharge reservoir (cgw, expon, smax: the store coupled below this infiltration scheme in NextGen / CFE),
validates them once on the host and runs the kernels of csrc/lgar_baseflow.hip (lgar_catchment_baseflow /
lgar_catchment_baseflow_grad, include/lgar.h; DESIGN.md section 15 has the definition): one launch per call, the same bits
whatever B, the launch or the run.  There is no CPU fallback: a store can be BUILT for device="cpu" (its host logic needs no
GPU), every call needs the library and a GPU.

    autograd.lgar_series -> catchment_sum -> catchment_route(runoff) + catchment_baseflow(percolation) -> network_route
        -> catchment_moments -> loss
"""
import math

import numpy as np
import torch

from . import _capi
from ._capi import LgarError, ptr


def _time_step(dt_h):
    try:
        dt = float(dt_h)
    except (TypeError, ValueError) as err:
        raise LgarError("dt_h must be a number of hours (%s)" % err)
    if not math.isfinite(dt) or dt <= 0.0:
        raise LgarError("dt_h must be finite and > 0 hours (got %r)" % (dt_h,))
    return dt


def _matrix(x, what, B, device, rows=None):
    """A fp64 [T, B] (rows=None) or [rows, B] tensor on `device`, detached and contiguous; anything else raises."""
    if (not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != B or x.dtype != torch.float64 or x.device != device
            or (rows is not None and x.shape[0] != rows)):
        raise LgarError("%s must be a fp64 [%s, %d] tensor on %s" % (what, "T" if rows is None else rows, B, device))
    if x.shape[0] >= 2 ** 31:
        raise LgarError("at most 2^31 - 1 rows")
    return x.detach().contiguous()


def _vector(x, what, B, device):
    if not isinstance(x, torch.Tensor) or x.dim() != 1 or x.shape[0] != B or x.dtype != torch.float64 or x.device != device:
        raise LgarError("%s must be a fp64 [%d] tensor on %s" % (what, B, device))
    return x.detach().contiguous()


def _forward(lib, device, r, par, dt_h, state_in, want_state, want_storage):
    """(q, s or None, state_out or None) of one lgar_catchment_baseflow call."""
    T, B = int(r.shape[0]), int(r.shape[1])
    q = torch.empty(T, B, dtype=torch.float64, device=device)
    s = torch.empty(T, B, dtype=torch.float64, device=device) if want_storage else None
    state_out = torch.empty(B, dtype=torch.float64, device=device) if want_state else None
    _capi.launch(lib, "catchment_baseflow", device, r.data_ptr(), T, B, par.data_ptr(), dt_h, ptr(state_in), ptr(state_out),
                 q.data_ptr(), ptr(s))
    return q, s, state_out


def _backward(lib, device, gq, gs, r, s, par, dt_h, state_in, want_par, want_state):
    """(gr, gpar or None, gstate or None) of one lgar_catchment_baseflow_grad call."""
    T, B = int(r.shape[0]), int(r.shape[1])
    gr = torch.empty(T, B, dtype=torch.float64, device=device)
    gpar = torch.empty(3, B, dtype=torch.float64, device=device) if want_par else None
    gstate = torch.empty(B, dtype=torch.float64, device=device) if want_state else None
    _capi.launch(lib, "catchment_baseflow_grad", device, gq.data_ptr(), ptr(gs), r.data_ptr(), s.data_ptr(), T, B, par.data_ptr(),
                 dt_h, ptr(state_in), gr.data_ptr(), ptr(gpar), ptr(gstate))
    return gr, gpar, gstate


class CatchmentBaseflow:
    """cgw, expon, smax: [B] tensors, sequences, or scalars with n_catchments= (all catchments alike); dt_h: the row step in
    hours.  cgw is the discharge coefficient (depth per hour), expon the exponent, smax the storage scale (depth), in the depth
    unit of the recharge.  Validated once, on the host: every value finite, cgw >= 0, expon > 0, smax > 0, dt_h > 0; anything
    else raises LgarError.  .par is the fp64 [3, B] parameter block on the device, .B the number of catchments."""

    def __init__(self, cgw, expon, smax, dt_h, device="cuda:0", n_catchments=None):
        self.dt_h = _time_step(dt_h)
        cols = []
        for name, v in (("cgw", cgw), ("expon", expon), ("smax", smax)):
            if isinstance(v, torch.Tensor):
                if v.dtype != torch.float64:
                    raise LgarError("%s must be fp64 (got %s)" % (name, v.dtype))
                v = v.detach().cpu().numpy()
            try:
                v = np.asarray(v, dtype=np.float64)
            except (TypeError, ValueError) as err:
                raise LgarError("%s must be numbers (%s)" % (name, err))
            if v.ndim > 1:
                raise LgarError("%s must be a scalar or [B], one entry per catchment (got shape %s)" % (name, tuple(v.shape)))
            cols.append((name, v))
        sizes = {int(v.shape[0]) for _, v in cols if v.ndim == 1}
        if n_catchments is not None:
            sizes.add(int(n_catchments))
        if len(sizes) != 1:
            raise LgarError("cgw, expon, smax must agree on one number of catchments: [B] each, or scalars with n_catchments= (got %s)"
                            % (sorted(sizes) or "scalars only",))
        B = sizes.pop()
        if not 0 <= B < 2 ** 31:
            raise LgarError("0 .. 2^31 - 1 catchments (got %d)" % B)
        par = np.stack([np.broadcast_to(v, (B,)) for _, v in cols]).astype(np.float64)
        for k, (name, ok, rule) in enumerate((("cgw", par[0] >= 0.0, ">= 0"), ("expon", par[1] > 0.0, "> 0"), ("smax", par[2] > 0.0, "> 0"))):
            bad = np.nonzero(~(np.isfinite(par[k]) & ok))[0]
            if bad.size:
                raise LgarError("%s[%d] = %r: every %s must be finite and %s" % (name, bad[0], float(par[k][bad[0]]), name, rule))
        self.B = B
        self.device = torch.device(device)
        self.par = torch.from_numpy(np.ascontiguousarray(par)).to(self.device)
        self._states = {}  # key -> [B] carried storage (absent: zeros)

    # ------------------------------------------------------------------------------------------
    @classmethod
    def _open(cls, device):
        """The library the store runs on (what the test suite's host build of the kernels replaces)."""
        return _capi.open_library(device, "the catchment baseflow runs on a ROCm GPU: there is no CPU fallback (device %s)")

    def run(self, recharge, carry=True, key=None, state=None, storage=False):
        """recharge: fp64 [T, B] (the catchment sums of percolation) on the store's device -> fp64 [T, B] baseflow, or
        (baseflow, storage) with storage=True.  carry=True: the [B] storage stays on the device between calls, as
        CatchmentNetwork.route keeps its state: chunked calls equal one call bit for bit (one state per `key`); `state` (a [B]
        tensor) replaces the carried state first.  carry=False: starts from `state` (or None = zeros) and keeps nothing."""
        r = _matrix(recharge, "recharge", self.B, self.device)
        state = None if state is None else _vector(state, "state", self.B, self.device)
        state_in = (self._states.get(key) if state is None else state) if carry else state
        q, s, state_out = _forward(self._open(self.device), self.device, r, self.par, self.dt_h, state_in, bool(carry), bool(storage))
        if carry:
            self._states[key] = state_out
        return (q, s) if storage else q

    def reset(self):
        """Forget every carried state."""
        self._states = {}

    def state_of(self, key=None):
        """The carried [B] storage of `key`, or None before the first carried call."""
        return self._states.get(key)

    # ------------------------------------------------------------------------------------------
    @classmethod
    def function(cls, recharge, cgw, expon, smax, dt_h, state=None, return_storage=False):
        """catchment_baseflow (below) on the library this class opens."""
        if not isinstance(recharge, torch.Tensor) or recharge.dim() != 2 or recharge.dtype != torch.float64:
            raise LgarError("recharge must be a fp64 [T, B] tensor")
        B, device = int(recharge.shape[1]), recharge.device
        pars = []
        for name, v in (("cgw", cgw), ("expon", expon), ("smax", smax)):
            if not isinstance(v, torch.Tensor):
                try:
                    v = torch.tensor(float(v), dtype=torch.float64, device=device)
                except (TypeError, ValueError) as err:
                    raise LgarError("%s must be a fp64 [%d] tensor or a scalar (%s)" % (name, B, err))
            if v.dtype != torch.float64 or v.device != device or v.dim() > 1 or (v.dim() == 1 and v.shape[0] != B):
                raise LgarError("%s must be a fp64 [%d] tensor or a scalar on %s" % (name, B, device))
            pars.append(v)
        if state is not None:
            _vector(state, "state", B, device)
        out = _CatchmentBaseflow.apply(recharge, pars[0], pars[1], pars[2], state, _time_step(dt_h), bool(return_storage), cls)
        return out if return_storage else out[0]


class _CatchmentBaseflow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, recharge, cgw, expon, smax, state, dt_h, return_storage, owner):
        B, device = int(recharge.shape[1]), recharge.device
        r = _matrix(recharge, "recharge", B, device)
        par = torch.stack([p.detach().expand(B) for p in (cgw, expon, smax)]).contiguous()
        st = None if state is None else state.detach().contiguous()
        needs = any(ctx.needs_input_grad[:5])
        q, s, _ = _forward(owner._open(device), device, r, par, dt_h, st, False, return_storage or needs)
        ctx.owner, ctx.dt_h, ctx.has_state, ctx.return_storage = owner, dt_h, state is not None, return_storage
        ctx.scalar = tuple(p.dim() == 0 for p in (cgw, expon, smax))
        if needs:
            ctx.save_for_backward(r, par, s, *(() if st is None else (st,)))
        if return_storage:
            return q, s
        return (q,)

    @staticmethod
    def backward(ctx, gq, gs=None):
        r, par, s = ctx.saved_tensors[:3]
        st = ctx.saved_tensors[3] if ctx.has_state else None
        B, device = int(r.shape[1]), r.device
        gq = _matrix(gq.contiguous(), "gq", B, device, int(r.shape[0]))
        gs = _matrix(gs.contiguous(), "gs", B, device, int(r.shape[0])) if ctx.return_storage else None
        want_par, want_state = any(ctx.needs_input_grad[1:4]), ctx.has_state and ctx.needs_input_grad[4]
        gr, gpar, gstate = _backward(ctx.owner._open(device), device, gq, gs, r, s, par, ctx.dt_h, st, want_par, want_state)
        gp = [None, None, None]
        for k in range(3):
            if ctx.needs_input_grad[1 + k]:
                gp[k] = gpar[k].sum() if ctx.scalar[k] else gpar[k]
        return gr if ctx.needs_input_grad[0] else None, gp[0], gp[1], gp[2], gstate, None, None, None


def catchment_baseflow(recharge, cgw, expon, smax, dt_h, state=None, return_storage=False):
    """Differentiable baseflow of the exponential groundwater store: recharge fp64 [T, B] -> baseflow [T, B], or (baseflow,
    storage) with return_storage=True.  cgw, expon, smax: fp64 [B] tensors or scalars (a scalar's gradient is summed over the
    catchments); state: the initial storage, [B] (None: zeros).  recharge, each of the three parameters and state receive
    gradients when they require one -- one backward launch gives all of them.  No stateful carry is used or kept.  Parameter
    values are not validated here (CatchmentBaseflow validates once; an optimiser keeps cgw >= 0, expon > 0, smax > 0 by its
    own transform): the kernels give the IEEE result for whatever they are handed.  Add the result to
    catchments.catchment_route(runoff sums) ahead of network.network_route."""
    return CatchmentBaseflow.function(recharge, cgw, expon, smax, dt_h, state, return_storage)
