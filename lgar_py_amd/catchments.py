"""Catchment sums: the [T, B] matrix of per-catchment sums of a stored [T, N] series, and its adjoint.

A NextGen-style job is thousands of catchments, each a handful to a few thousand columns (soil classes x sub-areas, area
weighted); what is compared with observations is catchment runoff.  CatchmentMap turns one catchment id per column into the CSR
map of lgar_catchment_sums (include/lgar.h; DESIGN.md section 10 has the definition), once, and runs the two kernels of
csrc/lgar_catchment.hip over device tensors.  There is no CPU fallback: a map can be BUILT for device="cpu" (its host logic
needs no GPU), sums() and spread() need the library and a GPU.

CatchmentRouting routes such a [T, B] matrix through one unit hydrograph per catchment (lgar_catchment_route, include/lgar.h;
DESIGN.md section 12), with the adjoint and the gradient with respect to the ordinates; catchment_route is the differentiable
form.
"""
import numpy as np
import torch

from . import _capi
from ._capi import LgarError, ptr
from .forcing import ForcingMap


_DTYPES = "catchment sums take float32 or float64 (got %s)"


class CatchmentMap:
    """ids: one integer per column, the catchment it belongs to (0 .. B - 1), or -1 for none; n_catchments: B (default: the
    largest id + 1); weights: [N] finite numbers (area fractions, say) or None = 1.

    Catchment b's members are the columns with id b in increasing column order (a stable sort by id): `order` holds them
    catchment after catchment and offsets[b] .. offsets[b + 1] bound catchment b in it.  Where the ids are already non-decreasing
    with no -1, order is None: every catchment is a contiguous stretch of columns and the kernel reads lane-contiguous instead of
    gathering.  The map is checked on the host and uploaded once.  B, N and sizes ([B] members per catchment, host int64) say
    what it holds."""

    def __init__(self, ids, n_catchments=None, weights=None, device="cuda:0"):
        ids_in = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        if ids_in.ndim != 1:
            raise LgarError("ids must be one catchment id per column, [N] (got shape %s)" % (tuple(ids_in.shape),))
        if ids_in.dtype.kind not in "iu":
            raise LgarError("ids must be integers (got %s): a catchment id is an index, -1 = none" % ids_in.dtype)
        N = int(ids_in.shape[0])
        if N >= 2 ** 31:
            raise LgarError("at most 2^31 - 1 columns (got %d)" % N)
        if ids_in.dtype.kind == "u" and N and int(ids_in.max()) >= 2 ** 31:
            raise LgarError("catchment ids must be below 2^31")
        ids64 = ids_in.astype(np.int64)
        top = int(ids64.max()) + 1 if N else 0
        B = top if n_catchments is None else int(n_catchments)
        if B < 0 or B >= 2 ** 31:
            raise LgarError("n_catchments must be in 0 .. 2^31 - 1 (got %d)" % B)
        if N and (int(ids64.min()) < -1 or top > B):
            raise LgarError("catchment ids must be -1 (none) or 0 .. %d; got %d .. %d" % (B - 1, int(ids64.min()), top - 1))
        self.N, self.B = N, B
        member = ids64 >= 0
        self.sizes = np.bincount(ids64[member], minlength=B).astype(np.int64)
        offsets = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(self.sizes, out=offsets[1:])
        contiguous = bool(member.all()) and bool((ids64[1:] >= ids64[:-1]).all())
        order = None if contiguous else np.argsort(ids64, kind="stable")[N - int(member.sum()):].astype(np.int32)
        self.ids_host, self.offsets_host, self.order_host = ids64.astype(np.int32), offsets.astype(np.int32), order
        w = None
        if weights is not None:
            try:
                # (a python sequence is read as fp64: torch.as_tensor alone would make it float32)
                w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.asarray(weights, dtype=np.float64))
                w = w.detach().to("cpu", torch.float64).contiguous()
            except (TypeError, ValueError, RuntimeError) as err:
                raise LgarError("weights must be [N] numbers (%s)" % err)
            if tuple(w.shape) != (N,):
                raise LgarError("weights must be [%d], one per column (got shape %s)" % (N, tuple(w.shape)))
            if not bool(torch.isfinite(w).all()):
                raise LgarError("weights must be finite")
        self.weights_host = w
        self.device = torch.device(device)
        up = lambda a: None if a is None else torch.from_numpy(a).to(self.device)
        self.ids, self.offsets, self.order = up(self.ids_host), up(self.offsets_host), up(self.order_host)
        self._weights = {}  # dtype -> [N] device tensor (the kernels read the weights in the series' element type)

    def weights(self, dtype):
        """The weights on the device, rounded to `dtype` ((double)w[c] in the definition is this value); None without."""
        if self.weights_host is None:
            return None
        if dtype not in self._weights:
            self._weights[dtype] = self.weights_host.to(self.device, dtype).contiguous()
        return self._weights[dtype]

    def forcing_map(self):
        """The forcing.ForcingMap of the ids (made once): every column reads the forcing column of its own catchment, so [T, B]
        forcing goes into LgarEngine.forward / autograd.lgar_series as it is.  A column of no catchment (id -1) has no forcing
        and cannot run: that raises."""
        if getattr(self, "_forcing_map", None) is None:
            if self.N and int(self.ids_host.min()) < 0:
                raise LgarError("%d columns belong to no catchment (id -1): a column without forcing cannot run"
                                % int((self.ids_host < 0).sum()))
            self._forcing_map = ForcingMap(self.ids_host, n_forcing=self.B, device=self.device)
        return self._forcing_map

    # ------------------------------------------------------------------------------------------
    def _open(self):
        """The library sums() and spread() run on (what the test suite's device-code simulator replaces)."""
        return _capi.open_library(self.device, "catchment sums run on a ROCm GPU: there is no CPU fallback (map device %s)")

    def _status(self, status):
        if status is None:
            return None
        if (not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or tuple(status.shape) != (self.N,)
                or status.device != self.ids.device or not status.is_contiguous()):
            raise LgarError("status must be a contiguous int32 [%d] tensor on %s" % (self.N, self.device))
        return status

    def sums(self, series, status=None, out=None, weight_sums=False):
        """series: a contiguous [R, N] float32 / float64 tensor on the map's device (a stored [T, N] series; a [D, N]
        soil-moisture block is one as well) -> fp64 [R, B], out[r, b] = the sum over catchment b's members of weight x value in
        the fixed order of the definition: the same bits whatever B, the other catchments, the members' place in the launch or
        the run.  status: int32 [N] (an engine's status): columns with a fault bit are skipped in every row, whatever their
        rows hold.  out: optional contiguous fp64 [R, B] buffer; it is written, not added to.  weight_sums=True: returns
        (sums, fp64 [B] sums of the weights of the members that were not skipped) -- sums / weight_sums is the mean over the
        valid columns."""
        lib = self._open()
        if (not isinstance(series, torch.Tensor) or series.dim() != 2 or series.shape[1] != self.N
                or series.device != self.ids.device or not series.is_contiguous()):
            raise LgarError("series must be a contiguous [R, %d] tensor on %s" % (self.N, self.device))
        code = _capi.dtype_code(series.dtype, _DTYPES % (series.dtype,))
        R = int(series.shape[0])
        if R >= 2 ** 31:
            raise LgarError("at most 2^31 - 1 rows")
        status = self._status(status)
        if out is None:
            out = torch.empty(R, self.B, dtype=torch.float64, device=self.device)
        elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != (R, self.B) or out.dtype != torch.float64
              or out.device != self.ids.device or not out.is_contiguous()):
            raise LgarError("out must be a contiguous fp64 [%d, %d] tensor on %s" % (R, self.B, self.device))
        wsum = torch.empty(self.B, dtype=torch.float64, device=self.device) if weight_sums else None
        w = self.weights(series.dtype)
        _capi.launch(lib, "catchment_sums", self.device, series.data_ptr(), R, self.N, self.offsets.data_ptr(), self.B,
                     ptr(self.order), 0 if self.order is None else int(self.order.numel()), ptr(w), ptr(status), out.data_ptr(),
                     ptr(wsum), code)
        return (out, wsum) if weight_sums else out

    def spread(self, grad, dtype, status=None):
        """The adjoint of sums(): grad [R, B] (converted to fp64) -> [R, N] tensor of `dtype`,
        out[r, c] = grad[r, ids[c]] * weight[c] rounded once to dtype; 0 for columns of no catchment and for columns whose
        status has a fault bit.  What LgarEngine.tangent / autograd.parameter_vjp take as w_runoff / w_perc."""
        lib = self._open()
        code = _capi.dtype_code(dtype, _DTYPES % (dtype,))
        if not isinstance(grad, torch.Tensor) or grad.dim() != 2 or grad.shape[1] != self.B:
            raise LgarError("grad must be a [R, %d] tensor" % self.B)
        grad = grad.detach().to(self.device, torch.float64).contiguous()
        R = int(grad.shape[0])
        status = self._status(status)
        out = torch.empty(R, self.N, dtype=dtype, device=self.device)
        w = self.weights(dtype)
        _capi.launch(lib, "catchment_spread", self.device, grad.data_ptr(), R, self.B, self.ids.data_ptr(), self.N, ptr(w),
                     ptr(status), out.data_ptr(), code)
        return out


class _CatchmentSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, series, cmap, status):
        ctx.cmap, ctx.status, ctx.dtype = cmap, status, series.dtype
        return cmap.sums(series.detach().contiguous(), status=status)

    @staticmethod
    def backward(ctx, grad):
        return ctx.cmap.spread(grad, ctx.dtype, status=ctx.status), None, None


def catchment_sum(series, cmap, status=None):
    """Differentiable cmap.sums(series, status): [T, N] -> fp64 [T, B]; the backward pass is cmap.spread.  Composes with
    autograd.lgar_series (parameters -> runoff [T, N] -> catchment runoff [T, B] -> loss) and with the graph-connected blocks
    model.dpLGAR returns."""
    return _CatchmentSum.apply(series, cmap, status)


class CatchmentRouting:
    """One unit hydrograph per catchment over a [T, B] matrix of catchment sums (lgar_catchment_route, include/lgar.h; DESIGN.md
    section 12 has the definition: the reference's GIUH queue, lgar/giuh.py:8-20, without its skip test).

    ordinates: [K] (one hydrograph shared by all catchments) or [B, K] (one per catchment; kept transposed, [K, B], on the
    device), finite, 1 <= K <= 64 (LGAR_ROUTE_KMAX).  n_catchments: B; required for nothing -- shared ordinates take B from the
    first matrix routed -- but a [B', K] that does not match it is refused.  The operator works at the row resolution of the
    series it is given: with num_subcycles > 1 the in-kernel GIUH shifts once per sub-step and is a different operator.
    There is no CPU fallback: the object can be BUILT for device="cpu" (its host logic needs no GPU), route(), adjoint() and
    ordinate_grad() need the library and a GPU."""

    def __init__(self, ordinates, n_catchments=None, device="cuda:0"):
        try:
            g = ordinates if isinstance(ordinates, torch.Tensor) else torch.from_numpy(np.asarray(ordinates, dtype=np.float64))
            g = g.detach().to("cpu", torch.float64)
        except (TypeError, ValueError, RuntimeError) as err:
            raise LgarError("ordinates must be [K] or [B, K] numbers (%s)" % err)
        if g.dim() not in (1, 2):
            raise LgarError("ordinates must be [K] (shared) or [B, K] (one hydrograph per catchment); got shape %s" % (tuple(g.shape),))
        K = int(g.shape[-1])
        if not 1 <= K <= _capi.ROUTE_KMAX:
            raise LgarError("a hydrograph has 1 .. %d ordinates (got %d)" % (_capi.ROUTE_KMAX, K))
        if not bool(torch.isfinite(g).all()):
            raise LgarError("ordinates must be finite")
        self.per_catchment = g.dim() == 2
        B = None if n_catchments is None else int(n_catchments)
        if B is not None and not 0 <= B < 2 ** 31:
            raise LgarError("n_catchments must be in 0 .. 2^31 - 1 (got %d)" % B)
        if self.per_catchment:
            if B is not None and int(g.shape[0]) != B:
                raise LgarError("ordinates are [%d, %d]: one hydrograph for each of %d catchments, not %d" % (g.shape[0], K, g.shape[0], B))
            B = int(g.shape[0])
            g = g.t()
        self.K, self.B = K, B
        self.ordinates_host = g.contiguous()  # [K] or [K, B]
        self.device = torch.device(device)
        self.ordinates = self.ordinates_host.to(self.device)
        self._queues = {}  # key -> [K, B] carried queue (absent: zeros)

    # ------------------------------------------------------------------------------------------
    def _open(self):
        """The library the routing runs on (what the test suite's device-code simulator replaces)."""
        return _capi.open_library(self.device, "catchment routing runs on a ROCm GPU: there is no CPU fallback (routing device %s)")

    def _matrix(self, x, what):
        if (not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float64 or x.device != self.ordinates.device
                or (self.B is not None and x.shape[1] != self.B)):
            raise LgarError("%s must be a fp64 [T, %s] tensor on %s" % (what, "B" if self.B is None else self.B, self.device))
        if x.shape[0] >= 2 ** 31 or x.shape[1] >= 2 ** 31:
            raise LgarError("at most 2^31 - 1 rows and catchments")
        return x.detach().contiguous()

    def _route(self, x, queue_in, want_queue, reverse):
        lib = self._open()
        T, B = int(x.shape[0]), int(x.shape[1])
        y = torch.empty(T, B, dtype=torch.float64, device=self.device)
        queue_out = torch.empty(self.K, B, dtype=torch.float64, device=self.device) if want_queue else None
        _capi.launch(lib, "catchment_route", self.device, x.data_ptr(), T, B, self.ordinates.data_ptr(), self.K,
                     int(self.per_catchment), ptr(queue_in), ptr(queue_out), y.data_ptr(), int(reverse))
        return y, queue_out

    def _queue_arg(self, queue, B):
        if queue is None:
            return None
        if (not isinstance(queue, torch.Tensor) or tuple(queue.shape) != (self.K, B) or queue.dtype != torch.float64
                or queue.device != self.ordinates.device):
            raise LgarError("queue must be a fp64 [%d, %d] tensor on %s" % (self.K, B, self.device))
        return queue.detach().contiguous()

    def route(self, x, carry=True, key=None, queue=None):
        """x: fp64 [T, B] on the routing's device -> fp64 [T, B], routed.  carry=True: the [K, B] queue stays on the device
        between calls, as an engine keeps its state: chunked calls equal one call bit for bit (one queue per `key`: an engine
        that routes several series through one routing keeps them apart by name); `queue` (a [K, B] tensor) replaces the carried
        queue first: a run resumed from a stored one.  carry=False: starts from `queue` (or None = zeros) and keeps nothing."""
        x = self._matrix(x, "x")
        if carry:
            q = self._queues.get(key) if queue is None else self._queue_arg(queue, int(x.shape[1]))
            if q is not None and q.shape[1] != x.shape[1]:
                raise LgarError("the carried queue is [%d, %d]: x must keep its %d catchments (reset() starts anew)" % (self.K, q.shape[1], q.shape[1]))
            y, self._queues[key] = self._route(x, q, True, False)
            return y
        return self._route(x, self._queue_arg(queue, int(x.shape[1])), False, False)[0]

    def reset(self):
        """Empty every carried queue."""
        self._queues = {}

    def queue_of(self, key=None):
        """The carried [K, B] queue of `key` (the layout and meaning of the reference's giuh_runoff_queue), or None before the
        first carried call."""
        return self._queues.get(key)

    queue = property(queue_of)

    def adjoint(self, gy):
        """The adjoint of route() with respect to x (a zero queue): gy fp64 [T, B] -> gx [T, B],
        gx[t] = the fold of g[k] * gy[t + k] from k = min(K - 1, T - 1 - t) down to 0 -- the same kernel under t -> T - 1 - t."""
        return self._route(self._matrix(gy, "gy"), None, False, True)[0]

    def ordinate_grad(self, x, gy):
        """The gradient of sum(gy * route(x)) with respect to the ordinates, in their own shape: [B, K] per catchment,
        gg[b, k] = sum_{t >= k} gy[t, b] * x[t - k, b] in increasing t (a fixed order); for shared ordinates that [B, K] result
        is summed over b with torch, and THAT sum is not order-pinned (its last bits may differ between runs).  The carried
        queue is a constant."""
        lib = self._open()
        x, gy = self._matrix(x, "x"), self._matrix(gy, "gy")
        if x.shape != gy.shape:
            raise LgarError("x and gy must have one shape (got %s and %s)" % (tuple(x.shape), tuple(gy.shape)))
        T, B = int(x.shape[0]), int(x.shape[1])
        out = torch.empty(self.K, B, dtype=torch.float64, device=self.device)
        _capi.launch(lib, "catchment_route_grad", self.device, x.data_ptr(), gy.data_ptr(), T, B, self.K, out.data_ptr())
        return out.t().contiguous() if self.per_catchment else out.sum(dim=1)


class _CatchmentRoute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ordinates, routing, queue):
        ctx.routing, ctx.g_dtype = routing, None if ordinates is None else ordinates.dtype
        ctx.save_for_backward(x)
        return routing.route(x, carry=False, queue=queue)

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        gy = gy.contiguous()
        gx = ctx.routing.adjoint(gy) if ctx.needs_input_grad[0] else None
        gg = ctx.routing.ordinate_grad(x, gy).to(ctx.g_dtype) if ctx.needs_input_grad[1] else None
        return gx, gg, None, None


def catchment_route(x, routing_or_ordinates, queue=None):
    """Differentiable routing: fp64 [T, B] -> [T, B].  routing_or_ordinates: a CatchmentRouting (its ordinates are constants),
    or an ordinates tensor [K] / [B, K], which gets a gradient when it requires one (CatchmentRouting.ordinate_grad).  The
    backward pass with respect to x is CatchmentRouting.adjoint.  No stateful queue is used or kept: the routing starts from
    `queue` ([K, B], a constant) or from zeros.  Composes with catchment_sum and autograd.lgar_series (parameters -> runoff
    [T, N] -> catchment runoff [T, B] -> routed runoff -> loss)."""
    if isinstance(routing_or_ordinates, CatchmentRouting):
        return _CatchmentRoute.apply(x, None, routing_or_ordinates, queue)
    if not isinstance(routing_or_ordinates, torch.Tensor):
        raise LgarError("catchment_route takes a CatchmentRouting or an ordinates tensor ([K] or [B, K])")
    routing = CatchmentRouting(routing_or_ordinates, n_catchments=int(x.shape[1]) if x.dim() == 2 else None, device=x.device)
    return _CatchmentRoute.apply(x, routing_or_ordinates, routing, queue)
