"""Forcing map: N soil columns read a [T, B] forcing through a per-column index.

The forcing layouts of LgarDims (forcing_columns / forcing_group) are periodic or equal-sized-group broadcasts.  A catchment job
has B catchments of unequal size, each with its own precipitation / PET series; ForcingMap is the per-column index
LgarForcing.column_map takes (include/lgar.h; DESIGN.md section 11 has the definition), checked on the host and uploaded once,
so that [T, B] forcing goes into LgarEngine.forward / tangent / autograd.lgar_series with no [T, N] forcing tensor anywhere.
Building one needs no GPU.

ForcingDirections: the derivatives of the forcing along a handful of parameters per forcing cell, what autograd.lgar_series takes
to carry a loss on the columns' output back to parameters that sit AHEAD of the columns (a precipitation or PET multiplier, the
snow parameters): the tangent kernels integrate them as extra lanes beside the soil-parameter directions.
scaled_forcing is the simplest producer.
"""
import numpy as np
import torch

from ._capi import LgarError


class ForcingMap:
    """index: 1-D integers [M], entry i = the forcing column (0 .. n_forcing - 1) that soil columns i * G .. i * G + G - 1 read
    (G = the call's forcing_group; 1: one entry per soil column); n_forcing: B, the number of forcing columns (default: the
    largest entry + 1).  `index` is the int32 [M] tensor on `device` the kernels read; M and B say what it holds."""

    def __init__(self, index, n_forcing=None, device="cuda:0"):
        idx = index.detach().cpu().numpy() if isinstance(index, torch.Tensor) else np.asarray(index)
        if idx.ndim != 1:
            raise LgarError("index must be one forcing column per soil column, [M] (got shape %s)" % (tuple(idx.shape),))
        if idx.dtype.kind not in "iu":
            raise LgarError("index must be integers (got %s): an entry is a column of the forcing" % idx.dtype)
        M = int(idx.shape[0])
        if M < 1 or M >= 2 ** 31:
            raise LgarError("index must have 1 .. 2^31 - 1 entries (got %d)" % M)
        if idx.dtype.kind == "u" and int(idx.max()) >= 2 ** 31:
            raise LgarError("forcing columns must be below 2^31")
        idx64 = idx.astype(np.int64)
        lo, top = int(idx64.min()), int(idx64.max()) + 1
        B = top if n_forcing is None else int(n_forcing)
        if B < 1 or B >= 2 ** 31:
            raise LgarError("n_forcing must be in 1 .. 2^31 - 1 (got %d)" % B)
        if lo < 0 or top > B:
            raise LgarError("index entries must be 0 .. %d; got %d .. %d" % (B - 1, lo, top - 1))
        self.M, self.B = M, B
        self.device = torch.device(device)
        self.index = torch.from_numpy(idx64.astype(np.int32)).to(self.device).contiguous()
        self._index_host = idx64.astype(np.int32)
        self._cell_map = None

    def cell_map(self, make):
        """The catchments.CatchmentMap whose catchments are this map's forcing cells (entry i belongs to cell index[i]), built on
        first use by make(ids, n_catchments=, device=) and kept: what sums per-column values to per-cell ones in a fixed order."""
        if self._cell_map is None:
            self._cell_map = make(self._index_host, n_catchments=self.B, device=self.device)
        return self._cell_map


class ForcingDirections:
    """params: a sequence of K tensors, each [B] (one value per forcing cell) or a scalar (one for all cells), the parameters the
    forcing was computed from; d_precip / d_pet: [K, T, B] tensors (or None = the parameter does not move that series),
    d_precip[k, t, b] = d precip[t, b] / d params[k][b] (a scalar parameter: / d params[k]).  The contract is CELL-LOCAL: forcing
    column b depends on params[k][b] only, so one lane per (column, k) carries the whole derivative.  B is the number of forcing
    columns of the run: the cells of its forcing_map, or its N columns when the forcing is [T, N].  The arrays are constants:
    autograd.lgar_series follows no graph through them."""

    def __init__(self, params, d_precip=None, d_pet=None):
        self.params = tuple(params)
        K = len(self.params)
        for k, p in enumerate(self.params):
            if not isinstance(p, torch.Tensor) or p.dim() > 1:
                raise LgarError("params[%d] must be a tensor, [B] or a scalar" % k)
        shape = None
        for nm, d in (("d_precip", d_precip), ("d_pet", d_pet)):
            if d is None:
                continue
            if not isinstance(d, torch.Tensor) or d.dim() != 3 or d.shape[0] != K or (shape is not None and tuple(d.shape) != shape):
                raise LgarError("%s must be a [K, T, B] tensor with K = %d parameters, and d_precip and d_pet alike; got %s"
                                % (nm, K, tuple(d.shape) if isinstance(d, torch.Tensor) else type(d).__name__))
            shape = tuple(d.shape)
        if K and shape is None:
            raise LgarError("forcing directions need d_precip or d_pet")
        for k, p in enumerate(self.params):
            if p.dim() == 1 and shape is not None and p.shape[0] != shape[2]:
                raise LgarError("params[%d] has %d entries, the forcing has %d cells" % (k, p.shape[0], shape[2]))
        self.K, self.shape = K, shape
        self.d_precip = None if d_precip is None else d_precip.detach()
        self.d_pet = None if d_pet is None else d_pet.detach()


def scaled_forcing(precip, pet, scale_p, scale_e):
    """(precip * scale_p, pet * scale_e, fd): [T, B] forcing under a precipitation and a PET multiplier per cell (tensors [B], or
    scalars), and the ForcingDirections that let autograd.lgar_series(..., forcing_directions=fd) return d loss / d scale_p and
    d loss / d scale_e.  The two products are plain tensors (detached): the gradient travels through fd."""
    precip, pet = torch.as_tensor(precip).detach(), torch.as_tensor(pet).detach()
    scale_p, scale_e = torch.as_tensor(scale_p), torch.as_tensor(scale_e)
    if precip.dim() != 2 or precip.shape != pet.shape:
        raise LgarError("precip and pet must be [T, B] alike; got %s / %s" % (tuple(precip.shape), tuple(pet.shape)))
    zero = torch.zeros_like(precip)
    fd = ForcingDirections((scale_p, scale_e), d_precip=torch.stack([precip, zero]), d_pet=torch.stack([zero, pet]))
    return precip * scale_p.detach().to(precip.device), pet * scale_e.detach().to(pet.device), fd
