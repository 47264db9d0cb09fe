#!/usr/bin/env python3
"""Generate the forcing-gradient fixtures (tests/golden/forcing_grad/gradx_<case>.npz) by running the LGAR-py reference itself.

As make_golden.py: runs ONLY where the reference is present, imports it here and nowhere else, and commits nothing but the
numbers it saves -- in a folder of their own, as the leaf and score fixtures: every .npz at the top of tests/golden is taken for a
trajectory or gradient fixture of make_golden.py (conftest.golden_names).  Five of make_golden.py's gradient cases are run again, by its own recipe (build_cfg, make_model, the agent's
call sequence), with the forcing tensor x ([T, 2]: precipitation, PET) as a leaf that requires grad; the loss is the one of the
grad_* fixtures, mean(runoff^2), and x.grad is what the tangent kernels' forcing direction is pinned to
(tests/test_forcing_tangent_host.py, tests/test_gpu_forcing_tangent.py).

calc_aet calls torch.clamp(x, min=0.0, max=pet) with a number and a tensor, which this torch refuses: the `clamp` shim of
make_leaf_tangent_golden.py (the number is made a tensor, nothing else changes) is put in its place.

Every fixture must reach precipitation (max |x.grad[:, 0]| > 0), and grad_two_layer_phil_150, which has PET and ponding, must
reach PET too (column 1); the script asserts both.  The reference's own central differences along a precipitation multiplier
are printed for comparison and not saved: they differ from its autograd by the line-search offsets, which autograd holds
constant.

Usage:  python tests/golden/make_forcing_grad_golden.py [case ...]
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import numpy as np
import torch

import make_golden as MG

NAMES = ("grad_synth0_12h", "grad_synth1_phil", "grad_manyfronts_60", "grad_two_layer_phil_150", "grad_six_layer_synth1")
NEEDS_PET = ("grad_two_layer_phil_150",)
OUT = os.path.join(HERE, "forcing_grad")


def _shim_clamp():
    import dpLGAR.models.physics.lgar.aet as aet_module

    class _Torch:
        """torch as calc_aet sees it (make_leaf_tangent_golden.py): clamp's number bound is made a tensor."""

        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def clamp(x, min=None, max=None):
            if isinstance(max, torch.Tensor) and not isinstance(min, torch.Tensor):
                min = torch.as_tensor(min, dtype=x.dtype)
            return torch.clamp(x, min=min, max=max)

    aet_module.torch = _Torch()


def _inputs(forcing, soil, pdm, subcycle_s, forcing_res_s, endtime_h, forcing_scale=1.0, initial_psi=2000.0, closed_form=False,
            frozen_factor=1, pulse=None, scale_pet=True, **_):
    """cfg and the forcing x of a case, as make_golden.run_case forms them"""
    from dpLGAR.data.Data import Data
    tmpdir = tempfile.mkdtemp(prefix="lgar_golden_")
    fcsv = MG._fixed_forcing_csv(os.path.join(MG.REF, "data", forcing), tmpdir)
    sdat = MG._write_soil_dat(soil, tmpdir)
    cfg = MG.build_cfg(fcsv, sdat, soil, pdm, subcycle_s, forcing_res_s, endtime_h, initial_psi, closed_form, frozen_factor)
    data = Data(cfg)
    x = data.x * forcing_scale
    if not scale_pet:
        x = data.x.clone()
        x[:, 0] = x[:, 0] * forcing_scale
    if pulse is not None:
        x = torch.tensor(MG.pulse_forcing(x.shape[0], **pulse))
    return cfg, x.detach().clone()


def _loss(cfg, soil, x):
    from dpLGAR.models.physics.MassBalance import MassBalance
    model = MG.make_model(cfg, soil)
    mb = MassBalance(cfg, model)
    runoffs = []
    for i in range(x.shape[0]):
        runoff, _ = model(x[i])
        runoffs.append(runoff)
        mb.change_mass(model)  # (the agent's call sequence: it also clears the model's per-step sums)
    y = torch.stack(runoffs)
    return torch.mean(y * y), y


def run(name):
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(0)
    _shim_clamp()
    os.makedirs(OUT, exist_ok=True)
    kw = MG.CASES[name][1]
    cfg, x = _inputs(**kw)
    x.requires_grad_()
    with torch.enable_grad():
        loss, y = _loss(cfg, kw["soil"], x)
        loss.backward()
    gx = x.grad.detach().numpy().copy()
    old = np.load(os.path.join(HERE, name + ".npz"))
    assert np.array_equal(old["forcing"], x.detach().numpy()) and float(old["loss"]) == float(loss.detach()), name  # the same run
    assert np.abs(gx[:, 0]).max() > 0.0, name + ": the reference's graph does not reach precipitation"
    if name in NEEDS_PET:
        assert np.abs(gx[:, 1]).max() > 0.0, name + ": the reference's graph does not reach PET"
    np.savez_compressed(os.path.join(OUT, "gradx_" + name + ".npz"), forcing=x.detach().numpy(), grad_x=gx, loss=float(loss),
                        runoff=y.detach().numpy().reshape(-1))
    # reported, never saved: the reference's own central difference along a precipitation multiplier
    auto = float((gx[:, 0] * x.detach().numpy()[:, 0]).sum())
    h, fd = 1e-6, []
    with torch.no_grad():
        for s in (1.0 + h, 1.0 - h):
            xs = x.detach().clone()
            xs[:, 0] *= s
            fd.append(float(_loss(cfg, kw["soil"], xs)[0]))
    return "%s: T=%d loss=%.6g max|dL/dprecip|=%.4g max|dL/dpet|=%.4g  d/dscale_p autograd %.6g central difference %.6g" % (
        name, x.shape[0], float(loss), np.abs(gx[:, 0]).max(), np.abs(gx[:, 1]).max(), auto, (fd[0] - fd[1]) / (2 * h))


if __name__ == "__main__":
    for nm in sys.argv[1:] or NAMES:
        print(run(nm), flush=True)
