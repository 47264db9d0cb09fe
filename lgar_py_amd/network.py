"""Catchment network: linear Muskingum channel routing between catchments, its adjoint and its coefficient gradient.

A gauge measures the discharge at an outlet: the catchment's own routed runoff plus everything that arrives from the
catchments upstream, delayed and attenuated by the channels.  CatchmentNetwork holds the reach graph (one reach = the channel of
one catchment; `downstream[b]` is the catchment b drains into, -1 for an outlet), validates it once on the host, sorts it into
levels and runs the kernels of csrc/lgar_network.hip (lgar_network_route / lgar_network_route_grad, include/lgar.h; DESIGN.md
section 14 has the definition): one launch per level, the same bits whatever B, the launch or the run.  There is no CPU
fallback: a network can be BUILT for device="cpu" (its host logic needs no GPU), every call needs the library and a GPU.
route_mc / network_route_mc are the same walk with flow-dependent reaches (Muskingum-Cunge: K = kref (Oprev / qref)^(-beta),
csrc/lgar_network_mc.hip, lgar_network_route_mc / lgar_network_route_mc_grad).
route_pool / network_route_pool add a second node kind, level-pool reservoirs at the nodes a NetworkPools names
(csrc/lgar_network_pool.hip, lgar_network_route_pool / lgar_network_route_pool_grad).

    autograd.lgar_series -> catchment_sum -> catchment_route -> network_route -> catchment_moments -> loss
"""
import numpy as np
import torch

from . import _capi, _stage
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


def weir_pool_parameters(area_m2, crest_length_m, weir_coefficient, href_m=1.0):
    """(cq, m, sref) of a pool for route_pool / network_route_pool whose outlet is a free overfall (a weir of crest length L and
    coefficient Cw, Q = Cw L h^1.5 in m^3/s with the head h in metres) and whose surface area does not change with the level, so
    that the active storage is a = area h:
        m = 1.5,   cq = Cw L href^1.5   (m^3/s, the release at head href),   sref = area href / 3600   (the storage at head href)
    The routed discharge must be in m^3/s and the row step in hours, as for manning_reach_parameters: storages are then in
    (m^3/s) h, which is why the area is divided by 3600.  s0 is the storage at the crest and smax the storage at which the pool
    spills: both are the caller's.  Plain differentiable torch in fp64; the arguments broadcast."""
    f64 = lambda v: torch.as_tensor(v, dtype=torch.float64)
    area = f64(area_m2)
    length, cw, href = (f64(v).to(area.device) for v in (crest_length_m, weir_coefficient, href_m))
    area, length, cw, href = torch.broadcast_tensors(area, length, cw, href)
    return cw * length * href ** 1.5, torch.full_like(area, 1.5), area * href / 3600.0


MC_RMIN, MC_RMAX = 1.0 / 64.0, 64.0  # the default range Oprev / qref is held to
POOL_RMIN, POOL_RMAX = 2.0 ** -20, 2.0 ** 20  # the default range (S - s0) / sref is held to
# (name, rule over (row, whole block), the rule in words) per row of a parameter block: _stage.check_rules
_POOL_RULES = (("cq", lambda v, par: np.isfinite(v) & (v >= 0.0), "finite and >= 0"), ("m", lambda v, par: np.isfinite(v) & (v >= 0.0), "finite and >= 0"),
               ("s0", lambda v, par: np.isfinite(v), "finite"), ("sref", lambda v, par: np.isfinite(v) & (v > 0.0), "finite and > 0"),
               ("smax", lambda v, par: v >= par[2], ">= s0 (+inf: the pool never spills)"))
_MC_RULES = (("kref", lambda v, par: np.isfinite(v) & (v > 0.0), "finite and > 0"), ("beta", lambda v, par: np.isfinite(v) & (v >= 0.0), "finite and >= 0"),
             ("X", lambda v, par: np.isfinite(v) & (v >= 0.0) & (v <= 0.5), "finite and in 0 .. 0.5"),
             ("qref", lambda v, par: np.isfinite(v) & (v > 0.0), "finite and > 0"))
_MC_NAMES, _POOL_NAMES = tuple(r[0] for r in _MC_RULES), tuple(r[0] for r in _POOL_RULES)


def _mc_scalars(dt_h, rmin, rmax):
    """dt_h, rmin, rmax as floats; what lgar_network_route_mc would refuse raises here, with the reason."""
    try:
        float(dt_h), float(rmin), float(rmax)
    except (TypeError, ValueError) as err:
        raise LgarError("dt_h, rmin, rmax must be numbers (%s)" % err)
    return (_stage.time_step(dt_h), *_stage.ratio_range(rmin, rmax, ("rmin", "rmax")))


def _pool_scalars(dt_h, rmin, rmax, prmin, prmax):
    """_mc_scalars and prmin, prmax as floats; what lgar_network_route_pool would refuse raises here, with the reason."""
    return (*_mc_scalars(dt_h, rmin, rmax), *_stage.ratio_range(prmin, prmax, ("prmin", "prmax")))


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
        self._pool_states = {}  # and for route_pool: (Iprev, Oprev) at a reach, (Iprev, S) at a pool

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
        return _stage.matrix(x, what, self.B, self.order.device, rows, shown=self.device)

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
        for k, v in enumerate((kref, beta, X, qref)):  # (one by one: a bad value of kref is reported before a bad type of beta)
            rows += _stage.rows_on_device(_MC_NAMES[k:k + 1], (v,), self.B, self.order.device, shown=self.device)
            if validate:
                _stage.check_rules(rows[k].detach().cpu().numpy().reshape(1, -1), _MC_RULES[k:k + 1])
        return torch.stack([v.detach().expand(self.B) for v in rows]).contiguous()

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

    def _pool_blocks(self, pools, reach, pool, validate):
        """(par_mc [4, B], par_pool [5, P]) on the device from reach = (kref, beta, X, qref) ([B] tensors or scalars) and
        pool = (cq, m, s0, sref, smax) ([P] tensors or scalars).  validate: on the host, and only where a value is read -- route_mc's
        rules at the reaches; at the pools cq >= 0, m >= 0, sref > 0, smax >= s0, everything but smax finite."""
        if not isinstance(pools, NetworkPools) or pools.network is not self:
            raise LgarError("pools must be a NetworkPools of this network")
        try:
            kref, beta, X, qref = reach
            values = tuple(pool)
            assert len(values) == 5
        except (TypeError, ValueError, AssertionError):
            raise LgarError("reach must be (kref, beta, X, qref) and pool (cq, m, s0, sref, smax)")
        par_mc = self._mc_par(kref, beta, X, qref, False)
        rows = _stage.rows_on_device(_POOL_NAMES, values, pools.P, self.order.device, shown=self.device)
        par_pool = torch.stack([v.detach().expand(pools.P) for v in rows]).contiguous()
        if validate:
            _stage.check_rules(par_mc.cpu().numpy(), _MC_RULES, mask=~pools.is_pool, of=" of a reach")
            _stage.check_rules(par_pool.cpu().numpy(), _POOL_RULES, where=lambda i: " (pool at catchment %d)" % pools.nodes_host[i])
        return par_mc, par_pool

    def _forward_pool(self, x, pools, par_mc, par_pool, scalars, state_in, want_state, want_storage):
        """(y [T, B], state_out [2, B] or None, storage [T, P] or None) of one lgar_network_route_pool call; scalars = dt_h, rmin,
        rmax, prmin, prmax."""
        lib = self._open()
        T, P = int(x.shape[0]), pools.P
        y = torch.empty(T, self.B, dtype=torch.float64, device=self.device)
        state_out = torch.empty(2, self.B, dtype=torch.float64, device=self.device) if want_state else None
        storage = torch.empty(T, P, dtype=torch.float64, device=self.device) if want_storage else None
        _capi.launch(lib, "network_route_pool", self.device, x.data_ptr(), T, self.B, par_mc.data_ptr(), par_pool.data_ptr() if P else None, P,
                     *scalars, self.up_ptr.data_ptr(), self.up_idx.data_ptr() if self.n_edges else None, self.n_edges, pools.order.data_ptr(),
                     self.level_ptr.ctypes.data, pools.pool_ptr.ctypes.data, self.n_levels, pools.pool_slot.data_ptr() if P else None,
                     ptr(state_in), ptr(state_out), y.data_ptr(), storage.data_ptr() if want_storage and T and P else None)
        return y, state_out, storage

    def _backward_pool(self, gy, x, y, storage, pools, par_mc, par_pool, scalars, state, want_par, want_pool, want_state):
        """(gx, gpar_mc [3, B] or None, gpool [4, P] or None, gstate [2, B] or None) of one lgar_network_route_pool_grad call."""
        lib = self._open()
        T, P = int(gy.shape[0]), pools.P
        gx = torch.empty(T, self.B, dtype=torch.float64, device=self.device)
        gpar = torch.empty(3, self.B, dtype=torch.float64, device=self.device) if want_par else None
        gpool = torch.empty(4, P, dtype=torch.float64, device=self.device) if want_pool else None
        gstate = torch.empty(2, self.B, dtype=torch.float64, device=self.device) if want_state else None
        _capi.launch(lib, "network_route_pool_grad", self.device, gy.data_ptr(), T, self.B, par_mc.data_ptr(), par_pool.data_ptr() if P else None,
                     P, *scalars, self.down.data_ptr(), pools.order.data_ptr(), self.level_ptr.ctypes.data, pools.pool_ptr.ctypes.data,
                     self.n_levels, pools.pool_slot.data_ptr() if P else None, gx.data_ptr(), x.data_ptr(), y.data_ptr(),
                     storage.data_ptr() if T and P else None, self.up_ptr.data_ptr(), self.up_idx.data_ptr() if self.n_edges else None,
                     self.n_edges, ptr(state), ptr(gpar), gpool.data_ptr() if want_pool and P else None, ptr(gstate))
        return gx, gpar, gpool, gstate

    # ------------------------------------------------------------------------------------------
    def route(self, x, coef, carry=True, key=None, state=None):
        """x: fp64 [T, B] lateral inflow (routed catchment runoff) on the network's device, coef: fp64 [3, B] (or [3]: all reaches
        alike) -> fp64 [T, B], the discharge at every catchment's outlet.  carry=True: the [2, B] state (the last inflow and
        discharge of every reach) stays on the device between calls, as CatchmentRouting keeps its queue: chunked calls equal one
        call bit for bit (one state per `key`); `state` (a [2, B] tensor) replaces the carried state first.  carry=False: starts
        from `state` (or None = zeros) and keeps nothing."""
        x, coef, state = self._matrix(x, "x"), self._coef(coef), self._state(state)
        return _stage.carried(self._states, carry, key, state, lambda state_in, want_state: self._forward(x, coef, state_in, want_state))[0]

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
        return _stage.carried(self._mc_states, carry, key, state,
                              lambda state_in, want_state: self._forward_mc(x, par, dt_h, rmin, rmax, state_in, want_state))[0]

    def mc_state_of(self, key=None):
        """The carried [2, B] state of route_mc's `key`, or None before the first carried call."""
        return self._mc_states.get(key)

    def route_pool(self, x, pools, reach, pool, dt_h, rmin=MC_RMIN, rmax=MC_RMAX, prmin=POOL_RMIN, prmax=POOL_RMAX, carry=True, key=None,
                   state=None, return_storage=False):
        """route_mc() on a network some of whose nodes are level-pool reservoirs (lakes).  pools: a NetworkPools of this network
        (which nodes are pools); reach = (kref, beta, X, qref), route_mc's parameters, read at the reaches only; pool = (cq, m, s0,
        sref, smax): fp64 [P] tensors on the network's device in the order of pools.nodes, or scalars that are broadcast.  A pool
        with storage S holds the active storage a = S - s0 above its dead storage s0 and releases Ql = cq (a / sref)^m (a / sref held
        to prmin .. prmax), at most what would drain it to s0 within the row and never less than zero; what does not fit below smax
        spills in the same row (smax = +inf: never).  The volume in over a row is dt_h (I + Iprev) / 2 and the volume is conserved:
        S_t - S_(t-1) = dt_h (I_t + I_(t-1)) / 2 - dt_h O_t.  Storages are in the unit of x times hours.  Validated once per call,
        on the host, only where a value is read: route_mc's rules at the reaches; at the pools everything but smax finite,
        cq >= 0, m >= 0, sref > 0, smax >= s0; dt_h > 0 and both ranges within 2^-60 .. 2^60.  The release is explicit (it is taken
        at the storage the row starts from): where cq dt_h is large against sref the storage can overshoot its equilibrium and the
        release oscillates from row to row.  That is NOT policed: choose dt_h below sref / (m cq) or so.  Without pools the result
        is route_mc's, bit for bit.  carry / key / state: as route_mc(), in a key space of its own, the [2, B] state holding
        (Iprev, Oprev) at a reach and (Iprev, S) at a pool; chunked calls equal one call bit for bit.  return_storage: also the
        [T, P] storage series, (y, storage)."""
        scalars = _pool_scalars(dt_h, rmin, rmax, prmin, prmax)
        par_mc, par_pool = self._pool_blocks(pools, reach, pool, True)
        x, state = self._matrix(x, "x"), self._state(state)
        y, _, storage = _stage.carried(self._pool_states, carry, key, state, lambda state_in, want_state: self._forward_pool(
            x, pools, par_mc, par_pool, scalars, state_in, want_state, return_storage), at=1)
        return (y, storage) if return_storage else y

    def pool_state_of(self, key=None):
        """The carried [2, B] state of route_pool's `key`, or None before the first carried call."""
        return self._pool_states.get(key)

    def reset(self):
        """Forget every carried state."""
        self._states = {}
        self._mc_states = {}
        self._pool_states = {}

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


class NetworkPools:
    """Which nodes of a CatchmentNetwork are level-pool reservoirs.  nodes: [P] distinct catchment ids (P = 0 is allowed); pool
    parameters and the storage series are in the order of `nodes`.  Validated once, on the host.  Builds what
    lgar_network_route_pool needs without touching the network's own arrays: order = the catchments by (level, is_pool, index), so
    that inside every level the reaches come first; pool_ptr[n_levels] (host) = where a level's pools start in that order;
    pool_slot[B] (device) = the index of a pool in `nodes`, -1 at a reach."""

    def __init__(self, network, nodes):
        if not isinstance(network, CatchmentNetwork):
            raise LgarError("NetworkPools takes a CatchmentNetwork")
        try:
            n = nodes.detach().cpu().numpy() if isinstance(nodes, torch.Tensor) else np.asarray(nodes)
            if n.size == 0:
                n = n.astype(np.int64)
            if n.dtype.kind not in "iu":
                raise TypeError("dtype %s" % n.dtype)
            n = n.astype(np.int64)
        except (TypeError, ValueError, RuntimeError) as err:
            raise LgarError("nodes must be [P] integers, the catchments that are pools (%s)" % err)
        if n.ndim != 1:
            raise LgarError("nodes must be [P], one entry per pool (got shape %s)" % (tuple(n.shape),))
        B = network.B
        bad = np.nonzero((n < 0) | (n >= B))[0]
        if bad.size:
            raise LgarError("nodes[%d] = %d is no catchment: ids are 0 .. %d" % (bad[0], n[bad[0]], B - 1))
        uniq, counts = np.unique(n, return_counts=True)
        if (counts > 1).any():
            raise LgarError("catchment %d is named twice in nodes: a pool is named once" % uniq[counts > 1][0])
        self.network, self.P = network, int(n.shape[0])
        self.nodes_host = n.astype(np.int32)
        self.is_pool = np.zeros(B, dtype=bool)
        self.is_pool[n] = True
        level = network.levels.astype(np.int64)
        self.order_host = np.lexsort((np.arange(B), self.is_pool, level)).astype(np.int32)
        reaches = np.bincount(level[~self.is_pool], minlength=network.n_levels)
        self.pool_ptr = np.ascontiguousarray(network.level_ptr[:network.n_levels] + reaches, dtype=np.int32)
        self.pool_slot_host = np.full(B, -1, dtype=np.int32)
        self.pool_slot_host[n] = np.arange(self.P, dtype=np.int32)
        self.order, self.pool_slot = (torch.from_numpy(a).to(network.device) for a in (self.order_host, self.pool_slot_host))


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
        gp = _stage.scalar_grads(gpar, ctx.needs_input_grad[1:4], ctx.scalar)
        return gx if ctx.needs_input_grad[0] else None, *gp, gstate, None, None, None, None, None


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


class _NetworkRoutePool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kref, beta, X, cq, m, s0, smax, state, qref, sref, network, pools, scalars):
        xm = network._matrix(x, "x")
        par_mc, par_pool = network._pool_blocks(pools, (kref, beta, X, qref), (cq, m, s0, sref, smax), False)
        st = network._state(state)
        y, _, storage = network._forward_pool(xm, pools, par_mc, par_pool, scalars, st, False, True)
        ctx.network, ctx.pools, ctx.scalars, ctx.has_state = network, pools, scalars, st is not None
        ctx.scalar = tuple(not isinstance(p, torch.Tensor) or p.dim() == 0 for p in (kref, beta, X, cq, m, s0, smax))
        ctx.save_for_backward(xm, y, storage, par_mc, par_pool, *(() if st is None else (st,)))
        return y

    @staticmethod
    def backward(ctx, gy):
        xm, y, storage, par_mc, par_pool = ctx.saved_tensors[:5]
        st = ctx.saved_tensors[5] if ctx.has_state else None
        net = ctx.network
        gy = net._matrix(gy.contiguous(), "gy", int(xm.shape[0]))
        want_state = ctx.has_state and ctx.needs_input_grad[8]
        gx, gpar, gpool, gstate = net._backward_pool(gy, xm, y, storage, ctx.pools, par_mc, par_pool, ctx.scalars, st,
                                                     any(ctx.needs_input_grad[1:4]), any(ctx.needs_input_grad[4:8]), want_state)
        need = ctx.needs_input_grad
        gp = _stage.scalar_grads(gpar, need[1:4], ctx.scalar[:3]) + _stage.scalar_grads(gpool, need[4:8], ctx.scalar[3:])
        return (gx if need[0] else None, *gp, gstate, None, None, None, None, None)


def network_route_pool(x, network, pools, reach, pool, dt_h, rmin=MC_RMIN, rmax=MC_RMAX, prmin=POOL_RMIN, prmax=POOL_RMAX, state=None):
    """Differentiable network.route_pool(x, pools, reach, pool, dt_h): fp64 [T, B] -> [T, B].  x, kref, beta, X ([B] tensors or
    scalars), cq, m, s0, smax ([P] tensors or scalars; a scalar's gradient is summed over the nodes it was broadcast to) and state
    ([2, B]; None: zeros) receive gradients when they require one -- one backward launch sequence gives all of them; qref and sref
    are constants.  A reach parameter receives +0.0 at a pool.  No stateful carry is used or kept.  Parameter values are not
    validated here (route_pool validates).  The gradient is that of the clamped statement with its regimes held fixed: nothing
    flows back through a release that the range, an empty pool or a spill has cut off.  The storage series is kept for the
    backward pass but not returned: a loss on it is not supported (route_pool(return_storage=True) gives the series)."""
    if not isinstance(network, CatchmentNetwork):
        raise LgarError("network_route_pool takes a CatchmentNetwork")
    scalars = _pool_scalars(dt_h, rmin, rmax, prmin, prmax)
    try:
        kref, beta, X, qref = reach
        cq, m, s0, sref, smax = pool
    except (TypeError, ValueError):
        raise LgarError("reach must be (kref, beta, X, qref) and pool (cq, m, s0, sref, smax)")
    return _NetworkRoutePool.apply(x, kref, beta, X, cq, m, s0, smax, state, qref, sref, network, pools, scalars)
