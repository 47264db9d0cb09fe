"""Forcing map: N soil columns read a [T, B] forcing through a per-column index.

The forcing layouts of LgarDims (forcing_columns / forcing_group) are periodic or equal-sized-group broadcasts.  A catchment job
has B catchments of unequal size, each with its own precipitation / PET series; ForcingMap is the per-column index
LgarForcing.column_map takes (include/lgar.h; DESIGN.md section 11 has the definition), checked on the host and uploaded once,
so that [T, B] forcing goes into LgarEngine.forward / tangent / autograd.lgar_series with no [T, N] forcing tensor anywhere.
Building one needs no GPU.
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
