#!/usr/bin/env python
"""Write tests/golden/leaf_tangent/leaf_tangent_ref.npz: the 100-digit derivative of the leaf statements (tests/leaf_ref/tangent.py:
mpmath dual numbers through leaf_ref.stmt_*) and, at the same points, the reference's own double-precision gradient --
torch.autograd.grad through the reference's physics/utils.py closures, calc_geff and calc_aet, imported as make_golden.py imports
them -- for tests/test_leaf_tangent_host.py and tests/test_gpu_leaf_tangent.py.  Needs mpmath and the reference; the tests that read
the file need neither.

Per function F of leaf_ref.tangent.FUNCTIONS: F.soil (int16 row of `soils`), F.x, F.y, F.z (float64 operands; z: the AET's dt_h),
F.f32ok (uint8: the point is an fp32 number, the fp32 run takes it too), F.value (float64: the statement), F.grad (float64 [N, 7]:
its partials in leaf_ref.tangent.SEEDS order), F.cond (float32 [N, 7]: each partial's terms added up by absolute value, leaf_ref.tangent.D), F.powt (float32: the largest
|y log2 x| among the point's pows), for the two trapezoids F.drift (float32 [N, 7]: leaf_ref.tangent.drift), F.ref_grad (float64 [N, 7]: the reference's autograd; NaN where the reference raises; geff's is geff_literal's: one reference).
nudge_gap [S, 8]: per soil, the largest relative gap between the trapezoid with and without calc_k_from_se's nudge at its nodes,
in the value and in each of the 7 partials.

Self-checks (any failure aborts): at most 2 % of a function's points are inf / NaN in the statement; the dual propagation agrees
with mpmath.diff at 150 digits on a subsample; the nudge gap is under the 1e-6 parity bar.

Usage:  python tests/golden/make_leaf_tangent_golden.py
"""
import multiprocessing
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(HERE, "_refstub"))
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import numpy as np

import leaf_ref as R
from leaf_ref import grid
from leaf_ref import tangent as TG

NINT = grid.NINT
PARITY_BAR = 1e-6


def _statement(job):
    fn, S, si, x, y, z = job
    val, grad, cond, powt, drift = [], [], [], [], []
    for i in range(len(x)):
        if fn in TG.LEAVES:
            v, g, _, a, t = TG.leaf(fn, S[int(si[i])], x[i], y[i], z[i], NINT)
            if fn in ("geff", "geff_literal"):
                drift.append(TG.drift(fn, S[int(si[i])], x[i], y[i], NINT))
        else:
            v, dx, dy = TG.prim(fn, x[i], y[i])
            v, g = float(v), [0.0] * 5 + [float(dx), float(dy)]
            a = [abs(u) for u in g]
            t = abs(y[i] * np.log2(x[i])) if fn in ("pw", "pwx") and x[i] > 0 else 0.0
        val.append(v); grad.append(g); cond.append(a); powt.append(t)
    return (np.array(val, dtype=np.float64), np.array(grad, dtype=np.float64).reshape(-1, TG.NS),
            np.array(cond, dtype=np.float64).reshape(-1, TG.NS), np.array(powt, dtype=np.float64),
            np.array(drift, dtype=np.float64).reshape(-1, TG.NS))


def _reference(job):
    """torch autograd through the reference at the job's points: [N, 7], NaN where the reference raises."""
    import logging
    import torch
    logging.disable(logging.CRITICAL)
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float64)  # (as make_golden.py: the reference makes its constants with torch.tensor(1.0))
    from dpLGAR.models.physics import utils as U
    import dpLGAR.models.physics.lgar.aet as aet_module
    from dpLGAR.models.physics.lgar.aet import calc_aet
    from dpLGAR.models.physics.lgar.green_ampt import calc_geff

    class _Torch:
        """torch as calc_aet sees it: this torch's clamp takes its two bounds as numbers or as tensors, not one of each as
        calc_aet passes them (min=0.0, max=pet) -- the number is made a tensor, nothing else changes."""

        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def clamp(x, min=None, max=None):
            if isinstance(max, torch.Tensor) and not isinstance(min, torch.Tensor):
                min = torch.as_tensor(min, dtype=x.dtype)
            return torch.clamp(x, min=min, max=max)

    aet_module.torch = _Torch()
    fn, S, si, x, y, z = job
    if fn == "geff":  # (the reference has one trapezoid: geff_literal's entry holds its gradient for both)
        return np.zeros((0, TG.NS))
    index = dict(theta_r=0, theta_e=1, m=2, bc_lambda=3, bc_psib_cm=4, h_min_cm=5)
    out = np.full((len(x), TG.NS), np.nan)
    t = lambda v: torch.tensor(float(v), dtype=torch.float64, requires_grad=True)
    for i in range(len(x)):
        alpha, n, ksat, te, tr = (t(v) for v in S[int(si[i])])
        X, Y = t(x[i]), t(y[i])
        inputs = [alpha, n, ksat, te, tr, X, Y]
        try:
            m = U.calc_m(n)
            if fn == "theta_from_h":
                r = U.calc_theta_from_h(X, alpha, m, n, te, tr)
            elif fn == "se_from_h":
                r = U.calc_se_from_h(X, alpha, m, n)
            elif fn == "k_from_se":
                r = U.calc_k_from_se(X, ksat, m)
            elif fn == "h_from_se":
                r = U.calc_h_from_se(X, alpha, m, n)
            elif fn == "se_from_theta":
                r = U.calc_se_from_theta(X, te, tr)
            elif fn == "aet":
                gp = types.SimpleNamespace(relative_moisture_at_which_PET_equals_AET=0.75,
                                           wilting_point_psi_cm=torch.tensor(R.WP_PSI, dtype=torch.float64))
                r = calc_aet(gp, torch.tensor(float(z[i]), dtype=torch.float64), Y, X, te, tr, m, alpha, n)
            elif fn in ("geff", "geff_literal", "geff_closed"):
                lam, psib = U.calc_bc_lambda(m), U.calc_bc_psib(alpha, m)
                gp = types.SimpleNamespace(soil_index=index, use_closed_form_G=(fn == "geff_closed"), nint=NINT, device="cpu")
                r = calc_geff(gp, [tr, te, m, lam, psib, U.calc_h_min_cm(lam, psib)], X, Y, alpha, n, ksat)
            elif fn in ("pw", "pwx"):
                r = torch.pow(X, Y)
            elif fn in ("dv", "quotient"):
                r = X / Y
            elif fn == "dv_dual_real":
                r = X / Y.detach()
            elif fn == "dv_real_dual":
                r = X.detach() / Y
            elif fn == "sq":
                r = torch.sqrt(X)
            elif fn in ("lg2", "lg2p"):
                r = torch.log2(X)
            elif fn in ("ex2", "ex2p"):
                r = torch.exp2(X)
            elif fn == "mn":
                r = torch.minimum(X, Y)
            elif fn == "ab":
                r = torch.abs(X)
            else:
                raise KeyError(fn)
        except ValueError:  # safe_pow / error_check: a negative base, a NaN
            continue
        if not r.requires_grad:  # (calc_se_from_h under the cut returns a constant)
            out[i] = 0.0
            continue
        g = torch.autograd.grad(r, inputs, allow_unused=True)
        out[i] = [0.0 if v is None else float(v) for v in g]
    return out


def _diff_check(job):
    fn, soil, x, y, z = job
    return fn, TG.check_against_diff(fn, soil, x, y, z, NINT)


def main():
    S, pts = grid.tangent_inputs()
    jobs, where = [], []
    for fn, (si, x, y, z, ok) in pts.items():
        step = 4 if fn in ("geff", "geff_literal") else 128
        for lo in range(0, len(x), step):
            jobs.append((fn, S, si[lo:lo + step], x[lo:lo + step], y[lo:lo + step], z[lo:lo + step]))
            where.append(fn)
    # the dual propagation against mpmath.diff at 150 digits: every 37th point of every leaf that lies away from its branches
    # (no theta_e end -- Se = 1 sits on the nudge's branch --, no operand within 1e-3 of the cut)
    checks = []
    for fn in TG.LEAVES:
        si, x, y, z, ok = pts[fn]
        te = S[si, 3]
        away = (np.abs(x - 0.1) > 1e-3) & (x != 1.0) & (x != te) & (y != te)
        if fn in ("k_from_se", "h_from_se"):
            away &= x < 0.999
        if fn in ("geff", "geff_literal"):
            away &= x < te
        if fn == "aet":
            away &= (x > 0) & (z <= 1.0)
        idx = np.nonzero(away)[0][::37 if fn not in ("geff", "geff_literal") else 97]
        checks += [(fn, S[int(si[i])], x[i], y[i], z[i]) for i in idx]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        ref_async = pool.map_async(_reference, jobs, chunksize=1)
        parts = pool.map(_statement, jobs, chunksize=1)
        refs = ref_async.get()
        diffs = pool.map(_diff_check, checks, chunksize=1)
    worst = {}
    for fn, w in diffs:
        worst[fn] = max(worst.get(fn, 0.0), w)
    for fn in TG.LEAVES:
        print("dual numbers against mpmath.diff at 150 digits, %-14s %3d points: worst relative difference %.1e"
              % (fn, sum(1 for c in checks if c[0] == fn), worst.get(fn, 0.0)))
        assert fn in worst and worst[fn] <= 1e-15, fn
    out = dict(soils=S, soil_names=np.array(grid.SOIL_NAMES))
    for fn, (si, x, y, z, ok) in pts.items():
        val = np.concatenate([p[0] for p, w in zip(parts, where) if w == fn])
        grad = np.concatenate([p[1] for p, w in zip(parts, where) if w == fn])
        # (what the tolerance needs of them: single precision, rounded up)
        cond = np.nextafter(np.concatenate([p[2] for p, w in zip(parts, where) if w == fn]).astype(np.float32), np.float32(np.inf))
        powt = np.concatenate([p[3] for p, w in zip(parts, where) if w == fn]).astype(np.float32)
        if fn in ("geff", "geff_literal"):
            drift = np.nextafter(np.concatenate([p[4] for p, w in zip(parts, where) if w == fn]).astype(np.float32), np.float32(np.inf))
            assert np.isfinite(drift).all()
        ref = np.concatenate([r for r, w in zip(refs, where) if w == ("geff_literal" if fn == "geff" else fn)])
        bad = ~(np.isfinite(val) & np.isfinite(grad).all(axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(ref - grad) / np.abs(grad)
        print("%-14s %5d points, %3d inf/NaN in the statement, %3d where the reference raises; median |reference - statement| / |statement| %.1e"
              % (fn, len(x), int(bad.sum()), int(np.isnan(ref).any(axis=1).sum()), float(np.nanmedian(rel[np.isfinite(rel) & (rel > 0)])) if np.isfinite(rel).any() else 0.0))
        assert bad.sum() <= 0.02 * len(x), (fn, int(bad.sum()), len(x))
        # a trapezoid the reference itself cannot evaluate (its running sum of heads overshoots into a negative pow base: very dry
        # soil with n = 1.09, h_i ~ 1e20 cm) has no measured bar: left out
        keep = ~(np.isnan(ref).any(axis=1) & np.isfinite(val)) if fn in ("geff", "geff_literal") else np.ones(len(x), dtype=bool)
        if not keep.all():
            print("%-14s %d points left out: the reference raises" % (fn, int((~keep).sum())))
        if fn in ("geff", "geff_literal"):
            out["%s.drift" % fn] = drift[keep]
        si, x, y, z, ok, val, grad, ref, cond, powt = (a[keep] for a in (si, x, y, z, ok, val, grad, ref, cond, powt))
        for k, a in (("soil", si), ("x", x), ("y", y), ("z", z), ("f32ok", ok), ("value", val), ("grad", grad), ("ref_grad", ref),
                     ("cond", cond), ("powt", powt)):
            if (fn, k) != ("geff", "ref_grad"):
                out["%s.%s" % (fn, k)] = a
    # the nudge the fused node leaves out: relative gap of the two trapezoids per soil, value and partials
    si = out["geff.soil"]
    a = np.concatenate([out["geff.value"][:, None], out["geff.grad"]], axis=1)
    b = np.concatenate([out["geff_literal.value"][:, None], out["geff_literal.grad"]], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(b != 0, np.abs(a - b) / np.abs(b), np.where(a != 0, np.inf, 0.0))
    rel = np.where(np.isfinite(a) & np.isfinite(b), rel, 0.0)
    gap = np.array([rel[si == k].max(axis=0) for k in range(len(S))])
    out["nudge_gap"] = gap
    for k in np.argsort(-gap.max(axis=1))[:4]:
        print("nudge gap, %-18s value %.1e, partials %s" % (grid.SOIL_NAMES[k], gap[k, 0], " ".join("%.1e" % v for v in gap[k, 1:])))
    assert gap.max() < PARITY_BAR, gap.max()
    path = os.path.join(HERE, "leaf_tangent", "leaf_tangent_ref.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (os.path.relpath(path, HERE), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
