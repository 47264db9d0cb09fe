"""Catchment canopy: an interception store per forcing cell AHEAD of the snowpack and the columns, with its adjoint, its parameter
gradients and its forward-mode tangent.

Rain wets the canopy first.  What the canopy holds evaporates at the potential rate and never reaches the soil, and the energy
spent on it is no longer available to the columns' AET: the store is the one stage that moves BOTH series the columns read.
CatchmentCanopy holds the three parameters (cmax: the depth of water the canopy holds per unit of relative leaf area; fe: the
wet-canopy evaporation factor; cover: the vegetated fraction of the cell), validates them once on the host and runs the kernels
of csrc/lgar_canopy.hip (lgar_catchment_canopy / _grad / _tangent, include/lgar.h; DESIGN.md section 21 has the definition): one
launch per call, the same bits whatever B, the launch or the run.  There is no CPU fallback: a store can be BUILT for
device="cpu" (its host logic needs no GPU), every call needs the library and a GPU.

    precip, pet [T, B] (, lai [T, B]) -> catchment_canopy -> water [T, B] -> (catchment_snow ->) LgarEngine.forward(water, pet_out, ..)
                                                          \\-> pet_out [T, B] ------------------------------------------^

Reverse mode (catchment_canopy) hands gradients on from its outputs to its inputs, its parameters and its state.  The forward-mode
way reaches a loss on the columns' output: catchment_canopy_directions packs d water and d pet_out along the parameters as the
forcing.ForcingDirections that autograd.lgar_series(forcing_directions=) integrates, and catchment_snow_directions(upstream=fd)
composes them with the snowpack's.  Out of scope: phase-aware interception (the store sees total precipitation), stem flow, a
drainage law, PET masking under a pack (a torch one-liner on pet_out).
"""
import numpy as np
import torch

from . import _capi, _stage
from ._capi import LgarError, ptr

PAR_NAMES = ("cmax", "fe", "cover")
NPAR = len(PAR_NAMES)
_RULES = (("cmax", lambda v, par: np.isfinite(v) & (v >= 0.0), "finite and >= 0"),
          ("fe", lambda v, par: np.isfinite(v) & (v >= 0.0), "finite and >= 0"),
          ("cover", lambda v, par: np.isfinite(v) & (v >= 0.0) & (v <= 1.0), "finite and in 0 .. 1"))


def _state(x, what, B, device):
    return _stage.state_block(x, what, (1, B), device, " (the depth held)")


def _new(device, *shape):
    return torch.empty(*shape, dtype=torch.float64, device=device)


def _forward(lib, device, p, e, lai, par, dt_h, state_in, want_state, want_store):
    """(w, pet_out, store or None, evap or None, state_out or None) of one lgar_catchment_canopy call."""
    T, B = int(p.shape[0]), int(p.shape[1])
    w, pet = _new(device, T, B), _new(device, T, B)
    store, evap = (_new(device, T, B), _new(device, T, B)) if want_store else (None, None)
    state_out = _new(device, 1, B) if want_state else None
    _capi.launch(lib, "catchment_canopy", device, p.data_ptr(), e.data_ptr(), ptr(lai), T, B, par.data_ptr(), dt_h, ptr(state_in),
                 ptr(state_out), w.data_ptr(), pet.data_ptr(), ptr(store), ptr(evap))
    return w, pet, store, evap, state_out


def _backward(lib, device, gw, gpet, gstore, gevap, p, e, lai, store, par, dt_h, state_in, want_lai, want_par, want_state):
    """(gp, ge, glai or None, gpar or None, gstate or None) of one lgar_catchment_canopy_grad call."""
    T, B = int(p.shape[0]), int(p.shape[1])
    gp, ge = _new(device, T, B), _new(device, T, B)
    glai = _new(device, T, B) if want_lai else None
    gpar = _new(device, NPAR, B) if want_par else None
    gstate = _new(device, 1, B) if want_state else None
    _capi.launch(lib, "catchment_canopy_grad", device, gw.data_ptr(), gpet.data_ptr(), ptr(gstore), ptr(gevap), p.data_ptr(), e.data_ptr(),
                 ptr(lai), ptr(store), T, B, par.data_ptr(), dt_h, ptr(state_in), gp.data_ptr(), ge.data_ptr(), ptr(glai), ptr(gpar), ptr(gstate))
    return gp, ge, glai, gpar, gstate


class CatchmentCanopy:
    """cmax, fe, cover: [B] tensors, sequences, or scalars with n_catchments= (all cells alike); dt_h: the row step in hours.  The
    canopy of a cell holds up to cmax * lai of the fraction `cover` of the precipitation; the rest of that fraction drips, the
    other 1 - cover falls through.  What is held evaporates at fe * cover * PET, and the PET left to the columns is PET less that
    evaporation, never below zero.  Validated once, on the host: every value finite, cmax >= 0, fe >= 0, 0 <= cover <= 1, dt_h > 0;
    anything else raises LgarError.  .par is the fp64 [3, B] parameter block on the device, .B the number of forcing cells."""

    def __init__(self, cmax, fe, cover, dt_h, device="cuda:0", n_catchments=None):
        self.dt_h = _stage.time_step(dt_h)
        par, self.B = _stage.block_on_host(PAR_NAMES, (cmax, fe, cover), n_catchments, "cell")
        _stage.check_rules(par, _RULES)
        self.device = torch.device(device)
        self.par = torch.from_numpy(np.ascontiguousarray(par)).to(self.device)
        self._states = {}  # key -> [1, B] carried store (absent: zeros)

    # ------------------------------------------------------------------------------------------
    @classmethod
    def _open(cls, device):
        """The library the store runs on (what the test suite's host build of the kernels replaces)."""
        return _capi.open_library(device, "the catchment canopy runs on a ROCm GPU: there is no CPU fallback (device %s)")

    def _series(self, precip, pet, lai):
        p = _stage.matrix(precip, "precip", self.B, self.device)
        e = _stage.matrix(pet, "pet", self.B, self.device, int(p.shape[0]))
        lai = None if lai is None else _stage.matrix(lai, "lai", self.B, self.device, int(p.shape[0]))
        return p, e, lai

    def run(self, precip, pet, lai=None, carry=True, key=None, state=None, store=False):
        """precip, pet: fp64 [T, B] on the store's device (rates in the unit of the engine's forcing); lai: fp64 [T, B] relative
        leaf area or None (= 1) -> (water, pet_out), fp64 [T, B] each, or (water, pet_out, store, evap) with store=True.
        carry=True: the [1, B] depth held stays on the device between calls, as CatchmentSnow.run keeps its pack: chunked calls
        equal one call bit for bit (one state per `key`); `state` (a [1, B] tensor) replaces the carried state first.
        carry=False: starts from `state` (or None = a dry canopy) and keeps nothing."""
        p, e, lai = self._series(precip, pet, lai)
        state = None if state is None else _state(state, "state", self.B, self.device)
        w, pet_out, st, ev, _ = _stage.carried(self._states, carry, key, state, lambda state_in, want_state: _forward(
            self._open(self.device), self.device, p, e, lai, self.par, self.dt_h, state_in, want_state, bool(store)))
        return (w, pet_out, st, ev) if store else (w, pet_out)

    def tangent(self, precip, pet, n_dirs, lai=None, dp=None, de=None, dlai=None, dpar=None, state=None, dstate=None, out=None,
                out_pet=None, k0=0, store=False, want_state=False, want_pet=True):
        """The forward-mode tangent of run() along n_dirs = D directions at once (lgar_catchment_canopy_tangent): the raw call.
        precip, pet, lai [T, B] and state ([1, B] or None = dry) are run()'s (nothing is carried here).  Input tangents, None =
        zeros: dp, de, dlai [D, T, B]; dpar [D, 3, B] (the rows of .par); dstate [D, B].  out / out_pet: None = a new zero
        [T, B, k0 + D] block, or a contiguous fp64 [T, B, ld] tensor with ld >= k0 + D (both of one ld): direction k of d water
        is written to out[:, :, k0 + k], of d pet_out to out_pet[:, :, k0 + k], and nothing else is touched -- the [T, B, G] blocks
        LgarEngine.tangent takes as d_precip and d_pet.  want_pet=False: d pet_out is not computed (out_pet is returned as None).
        Returns (out, out_pet, dstore, devap, dstate_out): the store's and the evaporation's tangents [D, T, B] with store=True and
        the end state's [D, B] with want_state=True, else None."""
        p, e, lai = self._series(precip, pet, lai)
        T, B, D = int(p.shape[0]), self.B, int(n_dirs)
        state = None if state is None else _state(state, "state", B, self.device)

        def block(x, what, shape):
            if x is None:
                return None
            if (not isinstance(x, torch.Tensor) or tuple(x.shape) != shape or x.dtype != torch.float64 or x.device != p.device
                    or not x.is_contiguous()):
                raise LgarError("%s must be a contiguous fp64 %s tensor on %s" % (what, list(shape), self.device))
            return x
        dp, de, dlai = block(dp, "dp", (D, T, B)), block(de, "de", (D, T, B)), block(dlai, "dlai", (D, T, B))
        dpar, dstate = block(dpar, "dpar", (D, NPAR, B)), block(dstate, "dstate", (D, B))
        k0 = int(k0)
        if D < 0 or k0 < 0:
            raise LgarError("n_dirs and k0 must be >= 0")

        def target(x, what):
            if x is None:
                return torch.zeros(T, B, k0 + D, dtype=torch.float64, device=self.device)
            if (not isinstance(x, torch.Tensor) or x.dim() != 3 or tuple(x.shape[:2]) != (T, B) or x.shape[2] < k0 + D
                    or x.dtype != torch.float64 or x.device != p.device or not x.is_contiguous()):
                raise LgarError("%s must be a contiguous fp64 [%d, %d, ld] tensor on %s with ld >= k0 + D = %d" % (what, T, B, self.device, k0 + D))
            return x
        out = target(out, "out")
        out_pet = target(out_pet, "out_pet") if want_pet else None
        if out_pet is not None and out_pet.shape[2] != out.shape[2]:
            raise LgarError("out and out_pet must have one ld (got %d and %d)" % (out.shape[2], out_pet.shape[2]))
        dstore, devap = (_new(self.device, D, T, B), _new(self.device, D, T, B)) if store else (None, None)
        dstate_out = _new(self.device, D, B) if want_state else None
        _capi.launch(self._open(self.device), "catchment_canopy_tangent", self.device, p.data_ptr(), e.data_ptr(), ptr(lai), T, B,
                     self.par.data_ptr(), self.dt_h, ptr(state), D, ptr(dp), ptr(de), ptr(dlai), ptr(dpar), ptr(dstate), out.data_ptr(),
                     ptr(out_pet), int(out.shape[2]), k0, ptr(dstore), ptr(devap), ptr(dstate_out))
        return out, out_pet, dstore, devap, dstate_out

    def reset(self):
        """Forget every carried state."""
        self._states = {}

    def state_of(self, key=None):
        """The carried [1, B] depth held of `key`, or None before the first carried call."""
        return self._states.get(key)

    # ------------------------------------------------------------------------------------------
    @classmethod
    def function(cls, precip, pet, cmax, fe, cover, dt_h, lai=None, state=None, return_store=False):
        """catchment_canopy (below) on the library this class opens."""
        if not isinstance(precip, torch.Tensor) or precip.dim() != 2 or precip.dtype != torch.float64:
            raise LgarError("precip must be a fp64 [T, B] tensor")
        B, device = int(precip.shape[1]), precip.device
        for what, x in (("pet", pet), ("lai", lai)):
            if x is not None and (not isinstance(x, torch.Tensor) or x.shape != precip.shape or x.dtype != torch.float64 or x.device != device):
                raise LgarError("%s must be a fp64 [%d, %d] tensor on %s" % (what, precip.shape[0], B, device))
        if pet is None:
            raise LgarError("pet must be a fp64 [%d, %d] tensor on %s" % (precip.shape[0], B, device))
        pars = _stage.rows_on_device(PAR_NAMES, (cmax, fe, cover), B, device)
        if state is not None:
            _state(state, "state", B, device)
        out = _CatchmentCanopy.apply(precip, pet, lai, *pars, state, _stage.time_step(dt_h), bool(return_store), cls)
        return out if return_store else out[:2]


class _CatchmentCanopy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, precip, pet, lai, cmax, fe, cover, state, dt_h, return_store, owner):
        B, device = int(precip.shape[1]), precip.device
        p = _stage.matrix(precip, "precip", B, device)
        e = _stage.matrix(pet, "pet", B, device, int(p.shape[0]))
        la = None if lai is None else _stage.matrix(lai, "lai", B, device, int(p.shape[0]))
        pars = (cmax, fe, cover)
        par = torch.stack([v.detach().expand(B) for v in pars]).contiguous()
        st = None if state is None else state.detach().contiguous()
        needs = any(ctx.needs_input_grad[:4 + NPAR])
        w, pet_out, store, evap, _ = _forward(owner._open(device), device, p, e, la, par, dt_h, st, False, return_store or needs)
        ctx.owner, ctx.dt_h, ctx.has_lai, ctx.has_state, ctx.return_store = owner, dt_h, la is not None, state is not None, return_store
        ctx.scalar = tuple(v.dim() == 0 for v in pars)
        if needs:
            ctx.save_for_backward(p, e, par, store, *(() if la is None else (la,)), *(() if st is None else (st,)))
        if return_store:
            return w, pet_out, store, evap
        return w, pet_out

    @staticmethod
    def backward(ctx, gw, gpet, gstore=None, gevap=None):
        p, e, par, store = ctx.saved_tensors[:4]
        rest = list(ctx.saved_tensors[4:])
        la = rest.pop(0) if ctx.has_lai else None
        st = rest.pop(0) if ctx.has_state else None
        T, B, device = int(p.shape[0]), int(p.shape[1]), p.device
        gw = _stage.matrix(gw.contiguous(), "gw", B, device, T)
        gpet = _stage.matrix(gpet.contiguous(), "gpet", B, device, T)
        gstore = _stage.matrix(gstore.contiguous(), "gstore", B, device, T) if ctx.return_store else None
        gevap = _stage.matrix(gevap.contiguous(), "gevap", B, device, T) if ctx.return_store else None
        need = ctx.needs_input_grad
        want_lai, want_par, want_state = ctx.has_lai and need[2], any(need[3:3 + NPAR]), ctx.has_state and need[3 + NPAR]
        gp, ge, glai, gpar, gstate = _backward(ctx.owner._open(device), device, gw, gpet, gstore, gevap, p, e, la, store, par, ctx.dt_h, st,
                                               want_lai, want_par, want_state)
        gs = _stage.scalar_grads(gpar, need[3:3 + NPAR], ctx.scalar)
        return (gp if need[0] else None, ge if need[1] else None, glai, *gs, gstate, None, None, None)


def catchment_canopy(precip, pet, cmax, fe, cover, dt_h, lai=None, state=None, return_store=False):
    """Differentiable canopy interception: precip, pet fp64 [T, B] -> (water, pet_out) [T, B] each, or (water, pet_out, store,
    evap) with return_store=True.  cmax, fe, cover: fp64 [B] tensors or scalars (a scalar's gradient is summed over the cells);
    lai: fp64 [T, B] relative leaf area (None: 1); state: the depth held at the start, [1, B] (None: dry).  precip, pet, lai, each
    of the three parameters and state receive gradients when they require one -- one backward launch gives all of them.  No
    stateful carry is used or kept.  Parameter values are not validated here (CatchmentCanopy validates once; an optimiser keeps
    cmax, fe >= 0 and cover in 0 .. 1 by its own transform): the kernels give the IEEE result for whatever they are handed.

    The store is ahead of the snowpack and sees total precipitation; PET under a pack is still the caller's one-liner on pet_out.
    To calibrate the canopy on runoff or discharge use catchment_canopy_directions with lgar_series(forcing_directions=)."""
    return CatchmentCanopy.function(precip, pet, cmax, fe, cover, dt_h, lai, state, return_store)


def catchment_canopy_directions(precip, pet, cmax, fe, cover, dt_h, lai=None, state=None, owner=CatchmentCanopy):
    """(water, pet_out, fd): the two [T, B] series of the canopy (plain tensors) and the forcing.ForcingDirections that carry a loss
    on the columns' output back to the canopy parameters: autograd.lgar_series(..., water, pet_out, forcing_directions=fd), or
    catchment_snow_directions(water, ..., upstream=fd) where a snowpack lies between.  precip, pet (, lai): fp64 [T, B]; the three
    parameters: fp64 [B] tensors or scalars; there is one direction per parameter that requires grad (in the order cmax, fe,
    cover), fd.params are those tensors, fd.d_precip[k] = d water / d params[k] and fd.d_pet[k] = d pet_out / d params[k], from
    ONE tangent launch (lgar_catchment_canopy_tangent).  state: the depth held at the start [1, B], a constant.  The parameters
    are validated as CatchmentCanopy validates them."""
    from .forcing import ForcingDirections
    if not isinstance(precip, torch.Tensor) or precip.dim() != 2:
        raise LgarError("precip must be a fp64 [T, B] tensor")
    B, device = int(precip.shape[1]), precip.device
    pars = tuple(torch.as_tensor(v) for v in (cmax, fe, cover))
    canopy = owner(*[v.detach().to("cpu", torch.float64).expand(B).contiguous() for v in pars], dt_h, device=device)
    lai = None if lai is None else lai.detach()
    water, pet_out = canopy.run(precip.detach(), pet.detach(), lai, carry=False, state=state)
    wanted = [j for j, v in enumerate(pars) if v.requires_grad]
    D = len(wanted)
    if D == 0:
        return water, pet_out, ForcingDirections((), None, None)
    dpar = torch.zeros(D, NPAR, B, dtype=torch.float64, device=device)
    for k, j in enumerate(wanted):
        dpar[k, j] = 1.0
    dw, dpet = canopy.tangent(precip.detach(), pet.detach(), D, lai=lai, dpar=dpar, state=state)[:2]  # [T, B, D] each
    return water, pet_out, ForcingDirections(tuple(pars[j] for j in wanted), d_precip=dw.permute(2, 0, 1).contiguous(),
                                             d_pet=dpet.permute(2, 0, 1).contiguous())
