"""Catchment network: linear Muskingum channel routing between catchments, its adjoint and its coefficient gradient.

A gauge measures the discharge at an outlet: the catchment's own routed runoff plus everything that arrives from the
catchments upstream, delayed and attenuated by the channels.  CatchmentNetwork holds the reach graph (one reach = the channel of
one catchment; `downstream[b]` is the catchment b drains into, -1 for an outlet), validates it once on the host, sorts it into
levels and runs the kernels of csrc/lgar_network.hip (lgar_network_route / lgar_network_route_grad, include/lgar.h; DESIGN.md
section 14 has the definition): one launch per level, the same bits whatever B, the launch or the run.  There is no CPU
fallback: a network can be BUILT for device="cpu" (its host logic needs no GPU), every call needs the library and a GPU.
route_mc / network_route_mc are the same walk with flow-dependent reaches (Muskingum-Cunge: K = kref (Oprev / qref)^(-beta),
csrc/lgar_network_mc.hip, lgar_network_route_mc / lgar_network_route_mc_grad).

    autograd.lgar_series -> catchment_sum -> catchment_route -> network_route -> catchment_moments -> loss
"""
import math

import numpy as np
import torch

from . import _capi
from ._capi import LgarError, ptr


def muskingum_coefficients(K_h, X, dt_h):
    """The coefficients of linear Muskingum routing, [3, B] = c0, c1, c2 (or [3] for scalar K_h and X: one reach, or all alike):
        c0 = (dt/2 - K X) / D,   c1 = (dt/2 + K X) / D,   c2 = (K - K X - dt/2) / D,   D = K - K X + dt/2
    K_h: the storage constant of a reach in hours (its travel time), X: the weight of the inflow in the storage (0 .. 0.5),
    dt_h: the row step in hours.  Plain differentiable torch in fp64: K_h and X receive gradients.  c0 + c1 + c2 = 1 (mass is
    conserved).  The coefficients are non-negative iff 2 K X <= dt <= 2 K (1 - X); that condition is NOT enforced: the kernels
    take coefficients of any sign."""
    K = torch.as_tensor(K_h, dtype=torch.float64)
    X = torch.as_tensor(X, dtype=torch.float64, device=K.device)
    K, X = torch.broadcast_tensors(K, X)
    half, KX = 0.5 * float(dt_h), K * X
    D = K - KX + half
    return torch.stack([(half - KX) / D, (half + KX) / D, (K - KX - half) / D])


def manning_reach_parameters(length_m, slope, n_manning, width_m, qref_m3s):
    """(kref_h, beta) of a reach for route_mc / network_route_mc from its geometry: the kinematic celerity of a wide rectangular
    channel under Manning's formula is c(Q) = (5/3) n^(-3/5) S^(3/10) W^(-2/5) Q^(2/5), so the travel time length / c falls as
    Q^(-2/5):
        beta = 0.4,   kref = length / (3600 (5/3) n^(-3/5) slope^(3/10) width^(-2/5) qref^(2/5))      hours, at discharge qref
    length_m and width_m in metres, slope dimensionless, qref_m3s in m^3/s: the discharge routed with these parameters must be in
    m^3/s too (qref is handed to the routing in the unit of its x).  Plain differentiable torch in fp64; the arguments broadcast."""
    f64 = lambda v: torch.as_tensor(v, dtype=torch.float64)
    length = f64(length_m)
    slope, n, width, qref = (f64(v).to(length.device) for v in (slope, n_manning, width_m, qref_m3s))
    celerity = (5.0 / 3.0) * n ** -0.6 * slope ** 0.3 * width ** -0.4 * qref ** 0.4
    kref = length / (3600.0 * celerity)
    return kref, torch.full_like(kref, 0.4)


MC_RMIN, MC_RMAX = 1.0 / 64.0, 64.0  # the default range Oprev / qref is held to
_MC_RULES = (("kref", lambda v: v > 0.0, "> 0"), ("beta", lambda v: v >= 0.0, ">= 0"), ("X", lambda v: (v >= 0.0) & (v <= 0.5), "in 0 .. 0.5"),
             ("qref", lambda v: v > 0.0, "> 0"))


def _mc_scalars(dt_h, rmin, rmax):
    """dt_h, rmin, rmax as floats; what lgar_network_route_mc would refuse raises here, with the reason."""
    try:
        dt, lo, hi = float(dt_h), float(rmin), float(rmax)
    except (TypeError, ValueError) as err:
        raise LgarError("dt_h, rmin, rmax must be numbers (%s)" % err)
    if not math.isfinite(dt) or dt <= 0.0:
        raise LgarError("dt_h must be finite and > 0 hours (got %r)" % (dt_h,))
    if not (2.0 ** -60 <= lo <= hi <= 2.0 ** 60):
        raise LgarError("rmin, rmax must satisfy 2^-60 <= rmin <= rmax <= 2^60 (got %r, %r)" % (rmin, rmax))
    return dt, lo, hi


class CatchmentNetwork:
    """downstream: [B] integers, downstream[b] = the catchment b drains into, -1 for an outlet.  Validated once, on the host: an id
    outside -1 .. B - 1, a catchment that drains into itself or a cycle raises LgarError.
    level[b] = 0 without upstream, else 1 + the largest level upstream; order = the catchments by (level, index); level_ptr
    delimits the levels inside order (kept on the host: the library reads it to launch); up_ptr / up_idx = the direct upstream
    catchments of every b as CSR lists, ascending within a list -- the order in which their discharge is added."""

    def __init__(self, downstream, device="cuda:0"):
        try:
            d = downstream.detach().cpu().numpy() if isinstance(downstream, torch.Tensor) else np.asarray(downstream)
            if d.dtype.kind not in "iu":
                raise TypeError("dtype %s" % d.dtype)
            d = d.astype(np.int64)
        except (TypeError, ValueError, RuntimeError) as err:
            raise LgarError("downstream must be [B] integers, -1 for an outlet (%s)" % err)
        if d.ndim != 1:
            raise LgarError("downstream must be [B], one entry per catchment (got shape %s)" % (tuple(d.shape),))
        B = int(d.shape[0])
        if B >= 2 ** 31:
            raise LgarError("at most 2^31 - 1 catchments (got %d)" % B)
        idx = np.arange(B, dtype=np.int64)
        bad = np.nonzero((d < -1) | (d >= B))[0]
        if bad.size:
            raise LgarError("downstream[%d] = %d is no catchment: ids are 0 .. %d, -1 marks an outlet" % (bad[0], d[bad[0]], B - 1))
        loops = np.nonzero(d == idx)[0]
        if loops.size:
            raise LgarError("catchment %d drains into itself" % loops[0])
        has = d >= 0
        src = idx[has]
        by_down = np.argsort(d[has], kind="stable")  # ascending source index within one downstream
        up_idx = src[by_down]
        counts = np.bincount(d[has], minlength=B)
        up_ptr = np.concatenate([[0], np.cumsum(counts)])
        # Kahn's waves: wave k releases the catchments whose upstream were all released before it, one of them by wave k - 1,
        # so the wave number is the level
        level = np.full(B, -1, dtype=np.int64)
        waiting = counts.copy()
        front, k = np.nonzero(waiting == 0)[0], 0
        while front.size:
            level[front] = k
            into = d[front]
            into = into[into >= 0]
            np.subtract.at(waiting, into, 1)
            into = np.unique(into)
            front, k = into[waiting[into] == 0], k + 1
        stuck = np.nonzero(level < 0)[0]
        if stuck.size:
            # every catchment never released has one upstream never released: walking up from one of them must come round
            b, seen = int(stuck[0]), set()
            while b not in seen:
                seen.add(b)
                ups = up_idx[up_ptr[b]:up_ptr[b + 1]]
                b = int(ups[level[ups] < 0][0])
            raise LgarError("the network has a cycle through catchment %d: a catchment must not drain into its own upstream" % b)
        self.B, self.n_levels, self.n_edges = B, k, int(up_idx.size)
        self.levels = level.astype(np.int32)
        self.downstream_host = d.astype(np.int32)
        self.order_host = np.lexsort((idx, level)).astype(np.int32)
        self.level_ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.bincount(level, minlength=k))]), dtype=np.int32)
        self.up_ptr_host, self.up_idx_host = up_ptr.astype(np.int32), up_idx.astype(np.int32)
        self.device = torch.device(device)
        self.down, self.order, self.up_ptr, self.up_idx = (torch.from_numpy(a).to(self.device) for a in
                                                           (self.downstream_host, self.order_host, self.up_ptr_host, self.up_idx_host))
        self._states = {}  # key -> [2, B] carried state (absent: zeros)
        self._mc_states = {}  # the same for route_mc: a key space of its own

    def upstream_of(self, b):
        """The direct upstream catchments of b, ascending (int32 array)."""
        if not 0 <= b < self.B:
            raise LgarError("catchment %r is not one of 0 .. %d" % (b, self.B - 1))
        return self.up_idx_host[self.up_ptr_host[b]:self.up_ptr_host[b + 1]].copy()

    # ------------------------------------------------------------------------------------------
    def _open(self):
        """The library the network runs on (what the test suite's host build of the kernels replaces)."""
        return _capi.open_library(self.device, "the catchment network runs on a ROCm GPU: there is no CPU fallback (network device %s)")

    def _matrix(self, x, what, rows=None):
        if (not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != self.B or x.dtype != torch.float64
                or x.device != self.order.device or (rows is not None and x.shape[0] != rows)):
            raise LgarError("%s must be a fp64 [%s, %d] tensor on %s" % (what, "T" if rows is None else rows, self.B, self.device))
        if x.shape[0] >= 2 ** 31:
            raise LgarError("at most 2^31 - 1 rows")
        return x.detach().contiguous()

    def _coef(self, coef):
        if isinstance(coef, torch.Tensor) and coef.dim() == 1 and coef.shape[0] == 3:  # one reach's coefficients for all
            coef = coef[:, None].expand(3, self.B)
        return self._matrix(coef, "coef", 3)

    def _state(self, state):
        return None if state is None else self._matrix(state, "state", 2)

    def _forward(self, x, coef, state_in, want_state):
        lib = self._open()
        T = int(x.shape[0])
        y = torch.empty(T, self.B, dtype=torch.float64, device=self.device)
        state_out = torch.empty(2, self.B, dtype=torch.float64, device=self.device) if want_state else None
        _capi.launch(lib, "network_route", self.device, x.data_ptr(), T, self.B, coef.data_ptr(), self.up_ptr.data_ptr(),
                     self.up_idx.data_ptr() if self.n_edges else None, self.n_edges, self.order.data_ptr(), self.level_ptr.ctypes.data,
                     self.n_levels, ptr(state_in), ptr(state_out), y.data_ptr())
        return y, state_out

    def _backward(self, gy, coef, x=None, y=None, state=None):
        """(gx, gc): gc is None unless x and y are given."""
        lib = self._open()
        T = int(gy.shape[0])
        gx = torch.empty(T, self.B, dtype=torch.float64, device=self.device)
        gc = torch.empty(3, self.B, dtype=torch.float64, device=self.device) if x is not None else None
        _capi.launch(lib, "network_route_grad", self.device, gy.data_ptr(), T, self.B, coef.data_ptr(), self.down.data_ptr(),
                     self.order.data_ptr(), self.level_ptr.ctypes.data, self.n_levels, gx.data_ptr(), ptr(x), ptr(y),
                     self.up_ptr.data_ptr() if x is not None else None,
                     self.up_idx.data_ptr() if x is not None and self.n_edges else None, self.n_edges, ptr(state), ptr(gc))
        return gx, gc

    def _mc_par(self, kref, beta, X, qref, validate):
        """The fp64 [4, B] parameter block on the device from [B] tensors or scalars (broadcast).  validate: every value finite,
        kref > 0, beta >= 0, 0 <= X <= 0.5, qref > 0, checked on the host."""
        rows = []
        for (name, ok, rule), v in zip(_MC_RULES, (kref, beta, X, qref)):
            if not isinstance(v, torch.Tensor):
                try:
                    v = torch.tensor(float(v), dtype=torch.float64, device=self.device)
                except (TypeError, ValueError) as err:
                    raise LgarError("%s must be a fp64 [%d] tensor or a scalar (%s)" % (name, self.B, err))
            if v.dtype != torch.float64 or v.device != self.order.device or v.dim() > 1 or (v.dim() == 1 and v.shape[0] != self.B):
                raise LgarError("%s must be a fp64 [%d] tensor or a scalar on %s" % (name, self.B, self.device))
            if validate:
                host = v.detach().cpu().numpy().reshape(-1)
                bad = np.nonzero(~(np.isfinite(host) & ok(host)))[0]
                if bad.size:
                    raise LgarError("%s[%d] = %r: every %s must be finite and %s" % (name, bad[0], float(host[bad[0]]), name, rule))
            rows.append(v.detach().expand(self.B))
        return torch.stack(rows).contiguous()

    def _forward_mc(self, x, par, dt_h, rmin, rmax, state_in, want_state):
        lib = self._open()
        T = int(x.shape[0])
        y = torch.empty(T, self.B, dtype=torch.float64, device=self.device)
        state_out = torch.empty(2, self.B, dtype=torch.float64, device=self.device) if want_state else None
        _capi.launch(lib, "network_route_mc", self.device, x.data_ptr(), T, self.B, par.data_ptr(), dt_h, rmin, rmax, self.up_ptr.data_ptr(),
                     self.up_idx.data_ptr() if self.n_edges else None, self.n_edges, self.order.data_ptr(), self.level_ptr.ctypes.data,
                     self.n_levels, ptr(state_in), ptr(state_out), y.data_ptr())
        return y, state_out

    def _backward_mc(self, gy, x, y, par, dt_h, rmin, rmax, state, want_par, want_state):
        """(gx, gpar [3, B] or None, gstate [2, B] or None) of one lgar_network_route_mc_grad call."""
        lib = self._open()
        T = int(gy.shape[0])
        gx = torch.empty(T, self.B, dtype=torch.float64, device=self.device)
        gpar = torch.empty(3, self.B, dtype=torch.float64, device=self.device) if want_par else None
        gstate = torch.empty(2, self.B, dtype=torch.float64, device=self.device) if want_state else None
        _capi.launch(lib, "network_route_mc_grad", self.device, gy.data_ptr(), T, self.B, par.data_ptr(), dt_h, rmin, rmax,
                     self.down.data_ptr(), self.order.data_ptr(), self.level_ptr.ctypes.data, self.n_levels, gx.data_ptr(), x.data_ptr(),
                     y.data_ptr(), self.up_ptr.data_ptr(), self.up_idx.data_ptr() if self.n_edges else None, self.n_edges, ptr(state),
                     ptr(gpar), ptr(gstate))
        return gx, gpar, gstate

    # ------------------------------------------------------------------------------------------
    def route(self, x, coef, carry=True, key=None, state=None):
        """x: fp64 [T, B] lateral inflow (routed catchment runoff) on the network's device, coef: fp64 [3, B] (or [3]: all reaches
        alike) -> fp64 [T, B], the discharge at every catchment's outlet.  carry=True: the [2, B] state (the last inflow and
        discharge of every reach) stays on the device between calls, as CatchmentRouting keeps its queue: chunked calls equal one
        call bit for bit (one state per `key`); `state` (a [2, B] tensor) replaces the carried state first.  carry=False: starts
        from `state` (or None = zeros) and keeps nothing."""
        x, coef, state = self._matrix(x, "x"), self._coef(coef), self._state(state)
        if carry:
            y, self._states[key] = self._forward(x, coef, self._states.get(key) if state is None else state, True)
            return y
        return self._forward(x, coef, state, False)[0]

    def route_mc(self, x, kref, beta, X, qref, dt_h, rmin=MC_RMIN, rmax=MC_RMAX, carry=True, key=None, state=None):
        """route() with flow-dependent reaches (Muskingum-Cunge): in every row the storage constant of a reach is
        K = kref (Oprev / qref)^(-beta), Oprev its own previous discharge held to rmin .. rmax times qref, and the row's Muskingum
        coefficients are those of (K, X, dt_h).  kref (hours, the travel time at discharge qref), beta (the celerity exponent; 0.4
        for Manning in a wide channel, manning_reach_parameters), X (the Muskingum weight) and qref (the unit of x): fp64 [B]
        tensors on the network's device, or scalars that are broadcast.  Validated once per call, on the host: finite, kref > 0,
        beta >= 0, 0 <= X <= 0.5, qref > 0, dt_h > 0, 2^-60 <= rmin <= rmax <= 2^60.  beta = 0 is route() with
        muskingum_coefficients(kref, X, dt_h), bit for bit.  The coefficients of a row are non-negative iff
        2 K X <= dt_h <= 2 K (1 - X) for that row's K; that is NOT enforced.  Variable-K Muskingum does not conserve volume
        exactly in transients.  carry / key / state: as route(), in a key space of its own; chunked calls equal one call bit for
        bit."""
        dt_h, rmin, rmax = _mc_scalars(dt_h, rmin, rmax)
        x, par, state = self._matrix(x, "x"), self._mc_par(kref, beta, X, qref, True), self._state(state)
        if carry:
            y, self._mc_states[key] = self._forward_mc(x, par, dt_h, rmin, rmax, self._mc_states.get(key) if state is None else state, True)
            return y
        return self._forward_mc(x, par, dt_h, rmin, rmax, state, False)[0]

    def mc_state_of(self, key=None):
        """The carried [2, B] state of route_mc's `key`, or None before the first carried call."""
        return self._mc_states.get(key)

    def reset(self):
        """Forget every carried state."""
        self._states = {}
        self._mc_states = {}

    def state_of(self, key=None):
        """The carried [2, B] state of `key` (row 0: the last inflow, row 1: the last discharge), or None before the first
        carried call."""
        return self._states.get(key)

    def accumulate(self, x):
        """Plain upstream accumulation: coef = (1, 0, 0), no carry.  y[t][b] = the sum of x[t] over b and everything upstream of
        it, in the pinned order of the definition."""
        one = torch.zeros(3, self.B, dtype=torch.float64, device=self.device)
        one[0] = 1.0
        return self.route(x, one, carry=False)

    def adjoint(self, gy, coef):
        """The adjoint of route() with respect to x (the carried state is a constant): gy fp64 [T, B] -> gx [T, B]."""
        return self._backward(self._matrix(gy, "gy"), self._coef(coef))[0]

    def coef_grad(self, x, y, gy, coef, state=None):
        """The gradient of sum(gy * route(x, coef, state)) with respect to coef, [3, B]; y = that route's result.  The terms of a
        reach are added in decreasing t (a fixed order)."""
        gy = self._matrix(gy, "gy")
        T = int(gy.shape[0])
        return self._backward(gy, self._coef(coef), self._matrix(x, "x", T), self._matrix(y, "y", T), self._state(state))[1]


class _NetworkRoute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, coef, network, state):
        ctx.network, ctx.state, ctx.coef_shape = network, state, tuple(coef.shape)
        y = network.route(x, coef, carry=False, state=state)
        ctx.save_for_backward(x, coef, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, coef, y = ctx.saved_tensors
        net = ctx.network
        gy = net._matrix(gy.contiguous(), "gy", int(x.shape[0]))
        if ctx.needs_input_grad[1]:
            gx, gc = net._backward(gy, net._coef(coef), net._matrix(x, "x"), y, net._state(ctx.state))
            if ctx.coef_shape == (3,):
                gc = gc.sum(dim=1)
        else:
            gx, gc = net._backward(gy, net._coef(coef))
        return gx, gc, None, None


def network_route(x, network, coef, state=None):
    """Differentiable network.route(x, coef): fp64 [T, B] -> [T, B].  x receives CatchmentNetwork.adjoint, coef ([3, B], e.g. from
    muskingum_coefficients) its gradient when it requires one.  No stateful carry is used or kept: the routing starts from
    `state` ([2, B], a constant: nothing flows back into it) or from zeros.  Composes with catchments.catchment_route before it
    and scores.catchment_moments behind it."""
    if not isinstance(network, CatchmentNetwork):
        raise LgarError("network_route takes a CatchmentNetwork")
    if not isinstance(coef, torch.Tensor):
        raise LgarError("coef must be a fp64 [3, %d] tensor on %s" % (network.B, network.device))
    return _NetworkRoute.apply(x, coef, network, state)


class _NetworkRouteMC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kref, beta, X, state, qref, network, dt_h, rmin, rmax):
        xm = network._matrix(x, "x")
        par = network._mc_par(kref, beta, X, qref, False)
        st = network._state(state)
        y = network._forward_mc(xm, par, dt_h, rmin, rmax, st, False)[0]
        ctx.network, ctx.scalars, ctx.has_state = network, (dt_h, rmin, rmax), st is not None
        ctx.scalar = tuple(not isinstance(p, torch.Tensor) or p.dim() == 0 for p in (kref, beta, X))
        ctx.save_for_backward(xm, y, par, *(() if st is None else (st,)))
        return y

    @staticmethod
    def backward(ctx, gy):
        xm, y, par = ctx.saved_tensors[:3]
        st = ctx.saved_tensors[3] if ctx.has_state else None
        net = ctx.network
        gy = net._matrix(gy.contiguous(), "gy", int(xm.shape[0]))
        want_state = ctx.has_state and ctx.needs_input_grad[4]
        gx, gpar, gstate = net._backward_mc(gy, xm, y, par, *ctx.scalars, st, any(ctx.needs_input_grad[1:4]), want_state)
        gp = [None, None, None]
        for k in range(3):
            if ctx.needs_input_grad[1 + k]:
                gp[k] = gpar[k].sum() if ctx.scalar[k] else gpar[k]
        return gx if ctx.needs_input_grad[0] else None, gp[0], gp[1], gp[2], gstate, None, None, None, None, None


def network_route_mc(x, network, kref, beta, X, qref, dt_h, rmin=MC_RMIN, rmax=MC_RMAX, state=None):
    """Differentiable network.route_mc(x, kref, beta, X, qref, dt_h): fp64 [T, B] -> [T, B].  x, kref, beta, X ([B] tensors, or
    scalars: a scalar's gradient is summed over the reaches) and state ([2, B], the initial Iprev, Oprev; None: zeros) receive
    gradients when they require one -- one backward launch sequence gives all of them; qref is a constant.  No stateful carry is
    used or kept.  Parameter values are not validated here (route_mc validates; an optimiser keeps kref > 0, beta >= 0,
    0 <= X <= 0.5 by its own transform): the kernels give the IEEE result for whatever they are handed.  The gradient is that of
    the clamped statement: a reach whose Oprev / qref sits outside rmin .. rmax hands nothing back through K in that row."""
    if not isinstance(network, CatchmentNetwork):
        raise LgarError("network_route_mc takes a CatchmentNetwork")
    dt_h, rmin, rmax = _mc_scalars(dt_h, rmin, rmax)
    return _NetworkRouteMC.apply(x, kref, beta, X, state, qref, network, dt_h, rmin, rmax)
