"""Catchment snowpack: a temperature-index store per forcing cell AHEAD of the columns, with its adjoint and parameter gradients.

Where winter precipitation falls as snow it lies for weeks and reaches the soil as melt.  CatchmentSnow holds the seven
parameters of the classic temperature-index routine (tlo, thi: the linear rain / snow transition; tm, cfmax: degree-day melt;
cfr: refreezing of held liquid; cwh: the liquid holding capacity; sfcf: the snowfall correction), validates them once on the
host and runs the kernels of csrc/lgar_snow.hip (lgar_catchment_snow / lgar_catchment_snow_grad, include/lgar.h; DESIGN.md
section 19 has the definition): one launch per call, the same bits whatever B, the launch or the run.  Its result is the [T, B]
water input LgarEngine.forward(water, pet, forcing_map=...) takes in the place of precipitation; its pack series (ice + liq) is
what a user scores against snow-water-equivalent records (scores.CatchmentScore).  There is no CPU fallback: a store can be BUILT
for device="cpu" (its host logic needs no GPU), every call needs the library and a GPU.

    precip, temp [T, B] -> catchment_snow -> water [T, B] -> LgarEngine.forward(water, pet, forcing_map=...) -> ...
                                          \\-> ice + liq [T, B] -> catchment_moments(SWE observations) -> loss

PET under snow is the caller's concern: the store does not touch it (for example pet * ((ice + liq) == 0) switches it off under
a pack).  A reverse-mode forcing gradient THROUGH the columns does not exist yet: catchment_snow hands gradients on from its own
outputs (water, ice, liq) to its inputs, and the columns give none with respect to their forcing, so through catchment_snow a loss
on runoff does not reach the snow parameters -- a loss on the pack series does.  The forward-mode way does: CatchmentSnow.tangent
(lgar_catchment_snow_tangent) gives d water along the parameters, catchment_snow_directions packs it as the
forcing.ForcingDirections that autograd.lgar_series(forcing_directions=) integrates beside the soil directions (DESIGN.md
section 20).
"""
import numpy as np
import torch

from . import _capi, _stage
from ._capi import LgarError, ptr

PAR_NAMES = ("tlo", "thi", "tm", "sfcf", "cfmax", "cfr", "cwh")
NPAR = len(PAR_NAMES)
_RULES = tuple((name, lambda v, par: np.isfinite(v), "finite") if k < 3 else (name, lambda v, par: np.isfinite(v) & (v >= 0.0), "finite and >= 0")
               for k, name in enumerate(PAR_NAMES))


def _state(x, what, B, device):
    return _stage.state_block(x, what, (2, B), device, " (ice, liq)")


def _forward(lib, device, p, ta, par, dt_h, state_in, want_state, want_pack):
    """(w, ice or None, liq or None, state_out or None) of one lgar_catchment_snow call."""
    T, B = int(p.shape[0]), int(p.shape[1])
    w = torch.empty(T, B, dtype=torch.float64, device=device)
    ice = torch.empty(T, B, dtype=torch.float64, device=device) if want_pack else None
    liq = torch.empty(T, B, dtype=torch.float64, device=device) if want_pack else None
    state_out = torch.empty(2, B, dtype=torch.float64, device=device) if want_state else None
    _capi.launch(lib, "catchment_snow", device, p.data_ptr(), ta.data_ptr(), T, B, par.data_ptr(), dt_h, ptr(state_in), ptr(state_out),
                 w.data_ptr(), ptr(ice), ptr(liq))
    return w, ice, liq, state_out


def _backward(lib, device, gw, gice, gliq, p, ta, ice, liq, par, dt_h, state_in, want_ta, want_par, want_state):
    """(gp, gta or None, gpar or None, gstate or None) of one lgar_catchment_snow_grad call."""
    T, B = int(p.shape[0]), int(p.shape[1])
    gp = torch.empty(T, B, dtype=torch.float64, device=device)
    gta = torch.empty(T, B, dtype=torch.float64, device=device) if want_ta else None
    gpar = torch.empty(NPAR, B, dtype=torch.float64, device=device) if want_par else None
    gstate = torch.empty(2, B, dtype=torch.float64, device=device) if want_state else None
    _capi.launch(lib, "catchment_snow_grad", device, gw.data_ptr(), ptr(gice), ptr(gliq), p.data_ptr(), ta.data_ptr(), ptr(ice), ptr(liq),
                 T, B, par.data_ptr(), dt_h, ptr(state_in), gp.data_ptr(), ptr(gta), ptr(gpar), ptr(gstate))
    return gp, gta, gpar, gstate


class CatchmentSnow:
    """tlo, thi, tm, sfcf, cfmax, cfr, cwh: [B] tensors, sequences, or scalars with n_catchments= (all cells alike); dt_h: the row
    step in hours.  Below tlo all precipitation is snow, above thi all is rain, linear between; snowfall is multiplied by sfcf;
    cfmax (depth per degree per hour) melts ice above tm; cfr * cfmax refreezes held liquid below tm; the pack holds liquid up to
    cwh * ice.  Validated once, on the host: every value finite, tlo <= thi, sfcf, cfmax, cfr, cwh >= 0, dt_h > 0; anything else
    raises LgarError.  .par is the fp64 [7, B] parameter block on the device, .B the number of forcing cells."""

    def __init__(self, tlo, thi, tm, sfcf, cfmax, cfr, cwh, dt_h, device="cuda:0", n_catchments=None):
        self.dt_h = _stage.time_step(dt_h)
        par, self.B = _stage.block_on_host(PAR_NAMES, (tlo, thi, tm, sfcf, cfmax, cfr, cwh), n_catchments, "cell")
        _stage.check_rules(par, _RULES)
        bad = np.nonzero(~(par[0] <= par[1]))[0]
        if bad.size:
            raise LgarError("tlo[%d] = %r > thi[%d] = %r: the transition needs tlo <= thi" % (bad[0], float(par[0][bad[0]]), bad[0], float(par[1][bad[0]])))
        self.device = torch.device(device)
        self.par = torch.from_numpy(np.ascontiguousarray(par)).to(self.device)
        self._states = {}  # key -> [2, B] carried pack (absent: zeros)

    # ------------------------------------------------------------------------------------------
    @classmethod
    def _open(cls, device):
        """The library the store runs on (what the test suite's host build of the kernels replaces)."""
        return _capi.open_library(device, "the catchment snowpack runs on a ROCm GPU: there is no CPU fallback (device %s)")

    def run(self, precip, temp, carry=True, key=None, state=None, pack=False):
        """precip, temp: fp64 [T, B] on the store's device (precipitation rate in the unit of the engine's forcing, air
        temperature) -> fp64 [T, B] water input rate, or (water, ice, liq) with pack=True.  carry=True: the [2, B] pack stays on
        the device between calls, as CatchmentBaseflow.run keeps its storage: chunked calls equal one call bit for bit (one state
        per `key`); `state` (a [2, B] tensor: ice, liq) replaces the carried state first.  carry=False: starts from `state` (or
        None = no pack) and keeps nothing."""
        p = _stage.matrix(precip, "precip", self.B, self.device)
        ta = _stage.matrix(temp, "temp", self.B, self.device, int(p.shape[0]))
        state = None if state is None else _state(state, "state", self.B, self.device)
        w, ice, liq, _ = _stage.carried(self._states, carry, key, state, lambda state_in, want_state: _forward(
            self._open(self.device), self.device, p, ta, self.par, self.dt_h, state_in, want_state, bool(pack)))
        return (w, ice, liq) if pack else w

    def tangent(self, precip, temp, n_dirs, dp=None, dta=None, dpar=None, state=None, dstate=None, out=None, k0=0, pack=False,
                want_state=False):
        """The forward-mode tangent of run() along n_dirs = D directions at once (lgar_catchment_snow_tangent): the raw call.
        precip, temp [T, B] and state ([2, B] or None = no pack) are run()'s (nothing is carried here).  Input tangents, None =
        zeros: dp, dta [D, T, B]; dpar [D, 7, B] (the rows of .par); dstate [D, 2, B].  out: None = a new zero [T, B, k0 + D] block,
        or a contiguous fp64 [T, B, ld] tensor with ld >= k0 + D: direction k is written to out[:, :, k0 + k] and nothing else is
        touched -- the [T, B, G] block LgarEngine.tangent takes as d_precip.  Returns (out, dice, dliq, dstate_out): the pack's
        tangents [D, T, B] with pack=True and the end state's [D, 2, B] with want_state=True, else None."""
        p = _stage.matrix(precip, "precip", self.B, self.device)
        T, B, D = int(p.shape[0]), self.B, int(n_dirs)
        ta = _stage.matrix(temp, "temp", B, self.device, T)
        state = None if state is None else _state(state, "state", B, self.device)

        def block(x, what, shape):
            if x is None:
                return None
            if (not isinstance(x, torch.Tensor) or tuple(x.shape) != shape or x.dtype != torch.float64 or x.device != p.device
                    or not x.is_contiguous()):
                raise LgarError("%s must be a contiguous fp64 %s tensor on %s" % (what, list(shape), self.device))
            return x
        dp, dta = block(dp, "dp", (D, T, B)), block(dta, "dta", (D, T, B))
        dpar, dstate = block(dpar, "dpar", (D, NPAR, B)), block(dstate, "dstate", (D, 2, B))
        k0 = int(k0)
        if D < 0 or k0 < 0:
            raise LgarError("n_dirs and k0 must be >= 0")
        if out is None:
            out = torch.zeros(T, B, k0 + D, dtype=torch.float64, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dim() != 3 or tuple(out.shape[:2]) != (T, B) or out.shape[2] < k0 + D
              or out.dtype != torch.float64 or out.device != p.device or not out.is_contiguous()):
            raise LgarError("out must be a contiguous fp64 [%d, %d, ld] tensor on %s with ld >= k0 + D = %d" % (T, B, self.device, k0 + D))
        z = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=self.device)
        dice, dliq = (z(D, T, B), z(D, T, B)) if pack else (None, None)
        dstate_out = z(D, 2, B) if want_state else None
        _capi.launch(self._open(self.device), "catchment_snow_tangent", self.device, p.data_ptr(), ta.data_ptr(), T, B, self.par.data_ptr(),
                     self.dt_h, ptr(state), D, ptr(dp), ptr(dta), ptr(dpar), ptr(dstate), out.data_ptr(), int(out.shape[2]), k0, ptr(dice),
                     ptr(dliq), ptr(dstate_out))
        return out, dice, dliq, dstate_out

    def reset(self):
        """Forget every carried state."""
        self._states = {}

    def state_of(self, key=None):
        """The carried [2, B] pack (ice, liq) of `key`, or None before the first carried call."""
        return self._states.get(key)

    # ------------------------------------------------------------------------------------------
    @classmethod
    def function(cls, precip, temp, tlo, thi, tm, sfcf, cfmax, cfr, cwh, dt_h, state=None, return_pack=False):
        """catchment_snow (below) on the library this class opens."""
        if not isinstance(precip, torch.Tensor) or precip.dim() != 2 or precip.dtype != torch.float64:
            raise LgarError("precip must be a fp64 [T, B] tensor")
        B, device = int(precip.shape[1]), precip.device
        if not isinstance(temp, torch.Tensor) or temp.shape != precip.shape or temp.dtype != torch.float64 or temp.device != device:
            raise LgarError("temp must be a fp64 [%d, %d] tensor on %s" % (precip.shape[0], B, device))
        pars = _stage.rows_on_device(PAR_NAMES, (tlo, thi, tm, sfcf, cfmax, cfr, cwh), B, device)
        if state is not None:
            _state(state, "state", B, device)
        out = _CatchmentSnow.apply(precip, temp, *pars, state, _stage.time_step(dt_h), bool(return_pack), cls)
        return out if return_pack else out[0]


class _CatchmentSnow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, precip, temp, tlo, thi, tm, sfcf, cfmax, cfr, cwh, state, dt_h, return_pack, owner):
        B, device = int(precip.shape[1]), precip.device
        p = _stage.matrix(precip, "precip", B, device)
        ta = _stage.matrix(temp, "temp", B, device, int(p.shape[0]))
        pars = (tlo, thi, tm, sfcf, cfmax, cfr, cwh)
        par = torch.stack([v.detach().expand(B) for v in pars]).contiguous()
        st = None if state is None else state.detach().contiguous()
        needs = any(ctx.needs_input_grad[:3 + NPAR])
        w, ice, liq, _ = _forward(owner._open(device), device, p, ta, par, dt_h, st, False, return_pack or needs)
        ctx.owner, ctx.dt_h, ctx.has_state, ctx.return_pack = owner, dt_h, state is not None, return_pack
        ctx.scalar = tuple(v.dim() == 0 for v in pars)
        if needs:
            ctx.save_for_backward(p, ta, par, ice, liq, *(() if st is None else (st,)))
        if return_pack:
            return w, ice, liq
        return (w,)

    @staticmethod
    def backward(ctx, gw, gice=None, gliq=None):
        p, ta, par, ice, liq = ctx.saved_tensors[:5]
        st = ctx.saved_tensors[5] if ctx.has_state else None
        T, B, device = int(p.shape[0]), int(p.shape[1]), p.device
        gw = _stage.matrix(gw.contiguous(), "gw", B, device, T)
        gice = _stage.matrix(gice.contiguous(), "gice", B, device, T) if ctx.return_pack else None
        gliq = _stage.matrix(gliq.contiguous(), "gliq", B, device, T) if ctx.return_pack else None
        need = ctx.needs_input_grad
        want_par, want_state = any(need[2:2 + NPAR]), ctx.has_state and need[2 + NPAR]
        gp, gta, gpar, gstate = _backward(ctx.owner._open(device), device, gw, gice, gliq, p, ta, ice, liq, par, ctx.dt_h, st, need[1],
                                          want_par, want_state)
        gs = _stage.scalar_grads(gpar, need[2:2 + NPAR], ctx.scalar)
        return (gp if need[0] else None, gta, *gs, gstate, None, None, None)


def catchment_snow(precip, temp, tlo, thi, tm, sfcf, cfmax, cfr, cwh, dt_h, state=None, return_pack=False):
    """Differentiable temperature-index snowpack: precip, temp fp64 [T, B] -> water input [T, B], or (water, ice, liq) with
    return_pack=True.  tlo, thi, tm, sfcf, cfmax, cfr, cwh: fp64 [B] tensors or scalars (a scalar's gradient is summed over the
    cells); state: the initial pack, [2, B] = ice, liq (None: no pack).  precip, temp, each of the seven parameters and state
    receive gradients when they require one -- one backward launch gives all of them.  No stateful carry is used or kept.
    Parameter values are not validated here (CatchmentSnow validates once; an optimiser keeps tlo <= thi and the four
    non-negative ones by its own transform): the kernels give the IEEE result for whatever they are handed.

    PET under snow is the caller's concern, for example pet * ((ice + liq) == 0).  A reverse-mode forcing gradient through the
    columns does not exist yet: the gradient of `water` is consumed here, but LgarEngine / lgar_series give none with respect to
    their forcing, so through this function the snow parameters are calibrated on the pack series (CatchmentScore of ice + liq
    against snow-water-equivalent records); to calibrate them on runoff or discharge use catchment_snow_directions with
    lgar_series(forcing_directions=).  A lapse rate or elevation bands are a shift of `temp` per cell in torch: temp receives its gradient."""
    return CatchmentSnow.function(precip, temp, tlo, thi, tm, sfcf, cfmax, cfr, cwh, dt_h, state, return_pack)


def catchment_snow_directions(precip, temp, tlo, thi, tm, sfcf, cfmax, cfr, cwh, dt_h, state=None, owner=CatchmentSnow, upstream=None):
    """(water, fd): the water input [T, B] of the snowpack (a plain tensor) and the forcing.ForcingDirections that carry a loss on
    the columns' output back to the snow parameters: autograd.lgar_series(..., water, pet, forcing_directions=fd).  precip, temp:
    fp64 [T, B]; the seven parameters: fp64 [B] tensors or scalars; there is one direction per parameter that requires grad (in
    the order tlo .. cwh), fd.params are those tensors and fd.d_precip[k] = d water / d params[k], from ONE tangent launch
    (lgar_catchment_snow_tangent).  state: the initial pack [2, B], a constant.  The parameters are validated as CatchmentSnow
    validates them.  PET is not touched: fd has no d_pet.

    upstream: None, or the ForcingDirections u of a stage AHEAD of the snowpack (canopy.catchment_canopy_directions), whose
    d_precip is the tangent of this call's `precip`.  Then ONE snow-tangent launch runs over u.K + D directions: the upstream
    rows enter through dp with a zero dpar, the snow rows are as before; fd.params = u.params + the snow's, fd.d_precip runs along
    all of them, and fd.d_pet = u.d_pet padded with zero rows for the snow parameters (None if u has none): the snowpack does not
    touch PET."""
    from .forcing import ForcingDirections
    pars = (tlo, thi, tm, sfcf, cfmax, cfr, cwh)
    if not isinstance(precip, torch.Tensor) or precip.dim() != 2:
        raise LgarError("precip must be a fp64 [T, B] tensor")
    B, device = int(precip.shape[1]), precip.device
    pars = tuple(torch.as_tensor(v) for v in pars)
    snow = owner(*[v.detach().to("cpu", torch.float64).expand(B).contiguous() for v in pars], dt_h, device=device)
    water = snow.run(precip.detach(), temp.detach(), carry=False, state=state)
    wanted = [j for j, v in enumerate(pars) if v.requires_grad]
    D, T = len(wanted), int(precip.shape[0])
    if upstream is not None and upstream.K:
        return water, _composed(snow, upstream, precip.detach(), temp.detach(), state, tuple(pars[j] for j in wanted), wanted)
    if D == 0:
        return water, ForcingDirections((), None, None)
    dpar = torch.zeros(D, NPAR, B, dtype=torch.float64, device=device)
    for k, j in enumerate(wanted):
        dpar[k, j] = 1.0
    dw = snow.tangent(precip.detach(), temp.detach(), D, dpar=dpar, state=state)[0]  # [T, B, D]
    return water, ForcingDirections(tuple(pars[j] for j in wanted), d_precip=dw.permute(2, 0, 1).contiguous())


def _composed(snow, u, precip, temp, state, params, wanted):
    """The directions of catchment_snow_directions behind an upstream stage u: u.K rows that enter through dp, then one row per
    wanted snow parameter through dpar, in one tangent launch."""
    from .forcing import ForcingDirections
    T, B, D = int(precip.shape[0]), int(precip.shape[1]), len(wanted)
    K = u.K + D
    if u.d_precip is None or tuple(u.d_precip.shape) != (u.K, T, B):
        raise LgarError("upstream.d_precip must be the [%d, %d, %d] tangent of precip" % (u.K, T, B))
    dp = torch.zeros(K, T, B, dtype=torch.float64, device=precip.device)
    dp[:u.K] = u.d_precip.to(precip.device, torch.float64)
    dpar = torch.zeros(K, NPAR, B, dtype=torch.float64, device=precip.device)
    for k, j in enumerate(wanted):
        dpar[u.K + k, j] = 1.0
    dw = snow.tangent(precip, temp, K, dp=dp, dpar=dpar, state=state)[0]  # [T, B, K]
    d_pet = None
    if u.d_pet is not None:
        d_pet = torch.zeros(K, T, B, dtype=torch.float64, device=precip.device)
        d_pet[:u.K] = u.d_pet.to(precip.device, torch.float64)
    return ForcingDirections(tuple(u.params) + tuple(params), d_precip=dw.permute(2, 0, 1).contiguous(), d_pet=d_pet)
