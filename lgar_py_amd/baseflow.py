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
import numpy as np
import torch

from . import _capi, _stage
from ._capi import LgarError, ptr

PAR_NAMES = ("cgw", "expon", "smax")
_RULES = (("cgw", lambda v, par: np.isfinite(v) & (v >= 0.0), "finite and >= 0"), ("expon", lambda v, par: np.isfinite(v) & (v > 0.0), "finite and > 0"),
          ("smax", lambda v, par: np.isfinite(v) & (v > 0.0), "finite and > 0"))


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
        self.dt_h = _stage.time_step(dt_h)
        par, self.B = _stage.block_on_host(PAR_NAMES, (cgw, expon, smax), n_catchments, "catchment")
        _stage.check_rules(par, _RULES)
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
        r = _stage.matrix(recharge, "recharge", self.B, self.device)
        state = None if state is None else _stage.state_block(state, "state", (self.B,), self.device)
        q, s, _ = _stage.carried(self._states, carry, key, state, lambda state_in, want_state: _forward(
            self._open(self.device), self.device, r, self.par, self.dt_h, state_in, want_state, bool(storage)))
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
        pars = _stage.rows_on_device(PAR_NAMES, (cgw, expon, smax), B, device)
        if state is not None:
            _stage.state_block(state, "state", (B,), device)
        out = _CatchmentBaseflow.apply(recharge, *pars, state, _stage.time_step(dt_h), bool(return_storage), cls)
        return out if return_storage else out[0]


class _CatchmentBaseflow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, recharge, cgw, expon, smax, state, dt_h, return_storage, owner):
        B, device = int(recharge.shape[1]), recharge.device
        r = _stage.matrix(recharge, "recharge", B, device)
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
        gq = _stage.matrix(gq.contiguous(), "gq", B, device, int(r.shape[0]))
        gs = _stage.matrix(gs.contiguous(), "gs", B, device, int(r.shape[0])) if ctx.return_storage else None
        want_par, want_state = any(ctx.needs_input_grad[1:4]), ctx.has_state and ctx.needs_input_grad[4]
        gr, gpar, gstate = _backward(ctx.owner._open(device), device, gq, gs, r, s, par, ctx.dt_h, st, want_par, want_state)
        gp = _stage.scalar_grads(gpar, ctx.needs_input_grad[1:4], ctx.scalar)
        return gr if ctx.needs_input_grad[0] else None, *gp, gstate, None, None, None


def catchment_baseflow(recharge, cgw, expon, smax, dt_h, state=None, return_storage=False):
    """Differentiable baseflow of the exponential groundwater store: recharge fp64 [T, B] -> baseflow [T, B], or (baseflow,
    storage) with return_storage=True.  cgw, expon, smax: fp64 [B] tensors or scalars (a scalar's gradient is summed over the
    catchments); state: the initial storage, [B] (None: zeros).  recharge, each of the three parameters and state receive
    gradients when they require one -- one backward launch gives all of them.  No stateful carry is used or kept.  Parameter
    values are not validated here (CatchmentBaseflow validates once; an optimiser keeps cgw >= 0, expon > 0, smax > 0 by its
    own transform): the kernels give the IEEE result for whatever they are handed.  Add the result to
    catchments.catchment_route(runoff sums) ahead of network.network_route."""
    return CatchmentBaseflow.function(recharge, cgw, expon, smax, dt_h, state, return_storage)
