"""Catchment sums: the [T, B] matrix of per-catchment sums of a stored [T, N] series, and its adjoint.

A NextGen-style job is thousands of catchments, each a handful to a few thousand columns (soil classes x sub-areas, area
weighted); what is compared with observations is catchment runoff.  CatchmentMap turns one catchment id per column into the CSR
map of lgar_catchment_sums (include/lgar.h; DESIGN.md section 10 has the definition), once, and runs the two kernels of
csrc/lgar_catchment.hip over device tensors.  There is no CPU fallback: a map can be BUILT for device="cpu" (its host logic
needs no GPU), sums() and spread() need the library and a GPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import LgarError
from .forcing import ForcingMap


def _dtype_code(dtype):
    if dtype == torch.float64:
        return _capi.F64
    if dtype == torch.float32:
        return _capi.F32
    raise LgarError("catchment sums take float32 or float64 (got %s)" % (dtype,))


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
    def _lib(self):
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise LgarError("catchment sums run on a ROCm GPU: there is no CPU fallback (map device %s)" % (self.device,))
        return _capi.load()

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
        lib = self._lib()
        if (not isinstance(series, torch.Tensor) or series.dim() != 2 or series.shape[1] != self.N
                or series.device != self.ids.device or not series.is_contiguous()):
            raise LgarError("series must be a contiguous [R, %d] tensor on %s" % (self.N, self.device))
        code = _dtype_code(series.dtype)
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
        ptr = lambda t: None if t is None else t.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            rc = lib.lgar_catchment_sums(series.data_ptr(), R, self.N, self.offsets.data_ptr(), self.B, ptr(self.order),
                                         0 if self.order is None else int(self.order.numel()), ptr(w), ptr(status),
                                         out.data_ptr(), ptr(wsum), code, stream)
        _capi.check(rc, "lgar_catchment_sums")
        return (out, wsum) if weight_sums else out

    def spread(self, grad, dtype, status=None):
        """The adjoint of sums(): grad [R, B] (converted to fp64) -> [R, N] tensor of `dtype`,
        out[r, c] = grad[r, ids[c]] * weight[c] rounded once to dtype; 0 for columns of no catchment and for columns whose
        status has a fault bit.  What LgarEngine.tangent / autograd.parameter_vjp take as w_runoff / w_perc."""
        lib = self._lib()
        code = _dtype_code(dtype)
        if not isinstance(grad, torch.Tensor) or grad.dim() != 2 or grad.shape[1] != self.B:
            raise LgarError("grad must be a [R, %d] tensor" % self.B)
        grad = grad.detach().to(self.device, torch.float64).contiguous()
        R = int(grad.shape[0])
        status = self._status(status)
        out = torch.empty(R, self.N, dtype=dtype, device=self.device)
        w = self.weights(dtype)
        ptr = lambda t: None if t is None else t.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            rc = lib.lgar_catchment_spread(grad.data_ptr(), R, self.B, self.ids.data_ptr(), self.N, ptr(w), ptr(status),
                                           out.data_ptr(), code, stream)
        _capi.check(rc, "lgar_catchment_spread")
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
