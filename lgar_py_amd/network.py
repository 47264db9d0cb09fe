"""Catchment network: linear Muskingum channel routing between catchments, its adjoint and its coefficient gradient.

A gauge measures the discharge at an outlet: the catchment's own routed runoff plus everything that arrives from the
catchments upstream, delayed and attenuated by the channels.  CatchmentNetwork holds the reach graph (one reach = the channel of
one catchment; `downstream[b]` is the catchment b drains into, -1 for an outlet), validates it once on the host, sorts it into
levels and runs the kernels of csrc/lgar_network.hip (lgar_network_route / lgar_network_route_grad, include/lgar.h; DESIGN.md
section 14 has the definition): one launch per level, the same bits whatever B, the launch or the run.  There is no CPU
fallback: a network can be BUILT for device="cpu" (its host logic needs no GPU), every call needs the library and a GPU.

    autograd.lgar_series -> catchment_sum -> catchment_route -> network_route -> catchment_moments -> loss
"""
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

    def reset(self):
        """Forget every carried state."""
        self._states = {}

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
