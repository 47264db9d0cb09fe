"""TEST INFRASTRUCTURE ONLY: the job tests/test_forcing_map_host.py and tests/test_gpu_forcing_map.py share -- three-layer
perturbed Phillipsburg columns under B = 5 forcing columns (48 rows of synth_1 from the start of its long storm, scaled per
forcing column: its FIRST 48 rows shed no runoff in any column, whatever the scale, so no comparison of runoff could tell the
forcing columns apart and every tangent would be zero) read through a shuffled, non-monotone index -- and the comparison both
use: a mapped run against the SAME engine settings run with the gathered forcing precip[:, index], bit for bit.  Columns are
independent and the gathered run is what the rest of the suite pins to the reference, so there is no tolerance here."""
import numpy as np
import torch

from lgar_py_amd import ACC_NAMES
from lgar_py_amd import workloads as W

PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
SCALES = np.array([0.5, 0.8, 1.0, 1.2, 1.5])  # rain per forcing column
B = len(SCALES)
T = 48
ROW0 = 56  # synth_1: three dry rows, then the long storm (rows 59 .. 128)
LONE = 3  # the forcing column a single soil column reads
KW = dict(dt_h=300.0 / 3600.0, ponded_depth_max=0.0)  # synth_1: five-minute rows, no ponding
STATE = ("depth", "theta", "psi", "k", "dzdt", "flags", "n_fronts", "scalars", "totals", "status")


def soil(N, seed):
    P = W.perturbed_columns(N, seed=seed)
    return tuple(P[k] for k in PARAMS)


def forcing(rows=T, pet=0.0):
    """(precip, pet) [rows, B] fp64 numpy: synth_1's rows from ROW0 on scaled per forcing column (its PET is zero; pet > 0 adds
    pet * (B - b) cm/h to forcing column b, so that the two arrays do not scale alike)."""
    f = W.synth1_forcing()[ROW0:ROW0 + rows]
    return f[:, 0:1] * SCALES[None, :], f[:, 1:2] * SCALES[None, :] + pet * (B - np.arange(B))[None, :]


def index(M, seed=0):
    """[M] forcing columns: every one of the B is used, by 1 (LONE) to ~0.4 M soil columns, in shuffled order."""
    rng = np.random.default_rng(seed)
    others = [b for b in range(B) if b != LONE]
    idx = np.concatenate([[LONE], others, rng.choice(others, M - B, p=[0.4, 0.3, 0.2, 0.1])])
    idx = idx[rng.permutation(M)].astype(np.int64)
    sizes = np.bincount(idx, minlength=B)
    assert sizes[LONE] == 1 and len(set(sizes.tolist())) >= 3 and (np.diff(idx) < 0).any() and (np.diff(idx) > 0).any()
    return idx


def gathered(pr, pe, idx, group=1):
    """The [rows, N] forcing the map stands for."""
    cols = np.repeat(np.asarray(idx), group)
    return np.ascontiguousarray(pr[:, cols]), np.ascontiguousarray(pe[:, cols])


def state(eng):
    return {f: getattr(eng, f).cpu().clone() for f in STATE}


def run(eng, pr, pe, **kw):
    """forward() over all ten series, then the state: one dict of CPU tensors."""
    out = eng.forward(torch.as_tensor(pr), torch.as_tensor(pe), series=tuple(ACC_NAMES), check=False, **kw)
    res = {k: v.cpu() for k, v in out.items()}
    res.update(state(eng))
    return res


def same(got, want, fields=None):
    """Bit for bit (NaN rows included: the bytes are compared)."""
    for f in want if fields is None else fields:
        a, b = got[f].contiguous().numpy(), want[f].contiguous().numpy()
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f


def forcing_matters(res, idx, group=1):
    """The gathered run tells the forcing columns apart: every valid member of the wettest forcing column sheds runoff, and
    more of it than any valid member of the driest one (a kernel that ignored the map could not pass the comparison that
    follows)."""
    cols = np.repeat(np.asarray(idx), group)
    ok = (res["status"].numpy() & 0x7F) == 0
    total = res["runoff"].double().sum(0).numpy()
    wet, dry = total[(cols == B - 1) & ok], total[(cols == 0) & ok]
    assert len(wet) and len(dry) and wet.min() > dry.max() >= 0.0 and wet.min() > 0.1, (wet.min(), dry.max())
    assert ok.mean() >= 0.9, ok.mean()
