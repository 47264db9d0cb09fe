"""Catchment scores: per-catchment moments of a [T, B] simulation against [To, B] observations with gaps, their adjoint, and
the metrics a catchment job trains on and reports (MSE, NSE, KGE, bias, correlation), one value per catchment.

What such a job compares with observations is routed catchment runoff (catchments.catchment_route).  Gauge records have
missing rows, different ones in every catchment, and may be coarser than the model's step (5-minute steps, hourly gauges).
CatchmentScore holds the observations on the device and runs the kernels of csrc/lgar_score.hip (lgar_catchment_moments /
lgar_catchment_moments_grad, include/lgar.h; DESIGN.md section 13 has the definition): seven moments per catchment, summed in a
pinned order -- the same bits whatever B, the other catchments, the launch or the run.  Every metric is then a few torch
operations on [B] vectors and differentiates through catchment_moments.  There is no CPU fallback: a score can be BUILT for
device="cpu" (its host logic needs no GPU), moments() and moments_grad() need the library and a GPU.

    autograd.lgar_series -> catchments.catchment_sum -> catchments.catchment_route -> catchment_moments -> loss
"""
import numpy as np
import torch

from . import _capi, _stage
from ._capi import LgarError

NMOM = _capi.SCORE_NMOM
N, MO, MS, SOO, SSS, SOS, SEE = range(NMOM)  # the rows of the moments
_COEF_ROWS = (MS, SSS, SOS, SEE)  # the moments that depend on the simulation: what the gradient kernel takes coefficients for
LOSS_METRICS = ("nse", "kge", "r", "mse")


class CatchmentScore:
    """observations: [To, B] numbers, one column per catchment; NaN and +-inf are gaps.  Uploaded once, as fp64.
    window: model rows per observation row (their mean is what is compared; the gradient is spread back over them).
    warmup: model rows skipped before the first observation row -- the reference's y_hat_[warmup:] -- a multiple of window; the
    observations START after the warm-up (rows of a gauge record that fall into it are cut by the caller).
    A simulation is fp64 [T, B] with T = warmup + To * window on the score's device."""

    def __init__(self, observations, window=1, warmup=0, device="cuda:0"):
        try:
            o = observations if isinstance(observations, torch.Tensor) else torch.from_numpy(np.asarray(observations, dtype=np.float64))
            o = o.detach().to("cpu", torch.float64).contiguous()
        except (TypeError, ValueError, RuntimeError) as err:
            raise LgarError("observations must be [To, B] numbers (%s)" % err)
        if o.dim() != 2:
            raise LgarError("observations must be [To, B], one column per catchment (got shape %s)" % (tuple(o.shape),))
        for name, v, low in (("window", window, 1), ("warmup", warmup, 0)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
                raise LgarError("%s must be an integer >= %d (got %r)" % (name, low, v))
        window, warmup = int(window), int(warmup)
        if warmup % window:
            raise LgarError("warmup counts model rows and must be a multiple of window = %d (got %d)" % (window, warmup))
        self.To, self.B, self.window, self.warmup = int(o.shape[0]), int(o.shape[1]), window, warmup
        self.T = warmup + self.To * window
        if self.T >= 2 ** 31 or self.B >= 2 ** 31:
            raise LgarError("at most 2^31 - 1 model rows and catchments (got %d and %d)" % (self.T, self.B))
        self.observations_host = o
        self.device = torch.device(device)
        self.observations = o.to(self.device)
        self._workspace = None

    # ------------------------------------------------------------------------------------------
    def _open(self):
        """The library the scores run on (what the test suite's host build of the kernels replaces)."""
        return _capi.open_library(self.device, "catchment scores run on a ROCm GPU: there is no CPU fallback (score device %s)")

    def _sim(self, sim):
        if (not isinstance(sim, torch.Tensor) or tuple(sim.shape) != (self.T, self.B) or sim.dtype != torch.float64
                or sim.device != self.observations.device):
            raise LgarError("sim must be a fp64 [%d, %d] tensor on %s: warmup %d + %d observation rows x window %d, %d catchments"
                            % (self.T, self.B, self.device, self.warmup, self.To, self.window, self.B))
        return sim.detach().contiguous()

    def _rows(self, x, rows, what):
        return _stage.matrix(x, what, self.B, self.observations.device, rows, shown=self.device)

    def _scratch(self, lib):
        """The device scratch of a call, kept on the object (the library allocates nothing)."""
        if self._workspace is None:
            nbytes = int(lib.lgar_catchment_moments_workspace(self.To, self.B))
            if nbytes < 0:
                raise LgarError("lgar_catchment_moments_workspace refused %d rows x %d catchments" % (self.To, self.B))
            self._workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        return self._workspace

    def moments(self, sim):
        """sim: fp64 [warmup + To * window, B] -> fp64 [7, B]: n, mo, ms, soo, sss, sos, see of every catchment over its valid
        rows (include/lgar.h), in the pinned order of the definition."""
        lib = self._open()
        sim = self._sim(sim)
        out = torch.empty(NMOM, self.B, dtype=torch.float64, device=self.device)
        ws = self._scratch(lib)
        _capi.launch(lib, "catchment_moments", self.device, sim[self.warmup:].data_ptr(), self.observations.data_ptr(), self.To,
                     self.B, self.window, out.data_ptr(), ws.data_ptr() if ws.numel() else None)
        return out

    def moments_grad(self, sim, moments, coef):
        """The adjoint: moments = self.moments(sim), coef fp64 [4, B] = d F / d (ms, sss, sos, see) -> d F / d sim, [T, B]: zero on
        the warm-up rows and on every row under a gap."""
        lib = self._open()
        sim, moments, coef = self._sim(sim), self._rows(moments, NMOM, "moments"), self._rows(coef, 4, "coef")
        out = torch.empty(self.T, self.B, dtype=torch.float64, device=self.device)
        out[:self.warmup].zero_()
        _capi.launch(lib, "catchment_moments_grad", self.device, sim[self.warmup:].data_ptr(), self.observations.data_ptr(), self.To,
                     self.B, self.window, moments.data_ptr(), coef.data_ptr(), out[self.warmup:].data_ptr())
        return out

    # ------------------------------------------------------------------------------------------
    def _moments_of(self, moments_or_sim):
        """A [7, B] tensor is taken for moments, anything else for a simulation (a score whose simulations have exactly seven
        rows must be given moments)."""
        x = moments_or_sim
        if isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[0] == NMOM:
            return x
        return catchment_moments(x, self)

    def metrics(self, moments_or_sim):
        """dict of [B] tensors, plain torch on the moments (so each differentiates through catchment_moments): n, mse = see / n,
        rmse, nse = 1 - see / soo, r = sos / sqrt(sss soo), alpha = sqrt(sss / soo), beta = ms / mo,
        kge = 1 - sqrt((r - 1)^2 + (alpha - 1)^2 + (beta - 1)^2), bias = ms - mo.  A catchment without a usable record (n = 0,
        soo = 0) gets the NaN or infinity the formula gives."""
        m = self._moments_of(moments_or_sim)
        n, mo, ms, soo, sss, sos, see = m.unbind(0)
        mse = see / n
        r = sos / torch.sqrt(sss * soo)
        alpha = torch.sqrt(sss / soo)
        beta = ms / mo
        kge = 1.0 - torch.sqrt((r - 1.0) ** 2 + (alpha - 1.0) ** 2 + (beta - 1.0) ** 2)
        return dict(n=n, mse=mse, rmse=torch.sqrt(mse), nse=1.0 - see / soo, r=r, alpha=alpha, beta=beta, kge=kge, bias=ms - mo)

    def loss(self, sim, metric="nse", min_count=2):
        """The mean of 1 - metric ("nse", "kge", "r"; of mse itself for "mse") over the catchments with n >= min_count and
        soo > 0.  A catchment without a usable record contributes neither value nor gradient: its metrics are never formed.
        Raises when no catchment qualifies."""
        if metric not in LOSS_METRICS:
            raise LgarError("loss takes one of %s (got %r)" % (", ".join(LOSS_METRICS), metric))
        m = self._moments_of(sim)
        with torch.no_grad():
            keep = torch.nonzero((m[N] >= min_count) & (m[SOO] > 0)).flatten()
        if keep.numel() == 0:
            raise LgarError("no catchment has %d valid rows and observations that vary: nothing to score" % min_count)
        v = self.metrics(m.index_select(1, keep))[metric]
        return (v if metric == "mse" else 1.0 - v).mean()


class _CatchmentMoments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sim, score):
        ctx.score = score
        m = score.moments(sim)
        ctx.save_for_backward(sim, m)
        return m

    @staticmethod
    def backward(ctx, gm):
        sim, m = ctx.saved_tensors
        coef = torch.stack([gm[i] for i in _COEF_ROWS]).to(torch.float64)  # (one launch; an index tensor would be a host-to-device copy)
        return ctx.score.moments_grad(sim, m, coef), None


def catchment_moments(sim, score):
    """Differentiable score.moments(sim): fp64 [T, B] -> [7, B].  The backward pass takes rows 2, 4, 5 and 6 of the incoming
    gradient (ms, sss, sos, see; n, mo and soo do not depend on sim) as the coefficients of lgar_catchment_moments_grad.
    Composes with catchments.catchment_route, catchments.catchment_sum and autograd.lgar_series."""
    if not isinstance(score, CatchmentScore):
        raise LgarError("catchment_moments takes a CatchmentScore")
    return _CatchmentMoments.apply(sim, score)
