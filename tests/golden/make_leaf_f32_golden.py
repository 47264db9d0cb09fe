#!/usr/bin/env python
"""Write tests/golden/leaf_f32/leaf_f32_ref.npz: the fp32 leaf functions' 40-digit statement and the coefficients of their error bound
(tests/leaf_ref: the formulas, the bound model; tests/leaf_ref/grid.py: the points), for tests/test_leaf_f32_host.py and
tests/test_gpu_leaf_f32.py.  Needs mpmath; the tests that read the file need none.

Per function F of leaf_ref.FUNCTIONS: F.soil (int16 row of `soils`), F.x, F.y, F.z (fp32 operands; z: the AET's dt_h), F.ref (float64:
the statement, or the inf / NaN the fp32 sequence ends in), F.coef (float64 [N, 6]: leaf_ref.COEF_NAMES).  A few minutes on eight cores.

Usage:  python tests/golden/make_leaf_f32_golden.py
"""
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import numpy as np

import leaf_ref as R
from leaf_ref import grid


def _chunk(job):
    fn, S, si, x, y, z = job
    return grid.evaluate(fn, S, si, x, y, z)


def main():
    S, pts = grid.inputs()
    jobs, where = [], []
    for fn, (si, x, y, z) in pts.items():
        step = 8 if fn.startswith("geff") and fn != "geff_closed" else 256
        for lo in range(0, len(x), step):
            jobs.append((fn, S, si[lo:lo + step], x[lo:lo + step], y[lo:lo + step], z[lo:lo + step]))
            where.append(fn)
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        parts = pool.map(_chunk, jobs, chunksize=1)
    out = dict(soils=S, soil_names=np.array(grid.SOIL_NAMES))
    for fn, (si, x, y, z) in pts.items():
        ref, coef, near, gap = (np.concatenate([p[j] for p, w in zip(parts, where) if w == fn]) for j in range(4))
        keep = ~(near < grid.NEAR_CUT)
        finite = np.isfinite(ref)
        b = R.FACTOR * R.bound(coef, R.UNITS_HOST[R.OPS_OF[fn][0][1]])
        # the statement and the exact walk of the kernel's sequence are two ways of writing one function: what they differ by
        # (a nudge one of them does not apply) must be nothing next to the bound
        worst_gap = float(np.max(np.where(finite & keep & (b > 0), gap / np.where(b > 0, b, 1.0), 0.0)))
        print("%-16s %5d points, %3d left out (a node at the cut), %3d inf/NaN, %4d unbounded, statement - sequence <= %.1e of the bound"
              % (fn, int(keep.sum()), int((~keep).sum()), int((~finite & keep).sum()), int((np.isinf(b) & finite & keep).sum()), worst_gap))
        assert worst_gap <= 1e-3, fn
        for k, a in (("soil", si), ("x", x), ("y", y), ("z", z), ("ref", ref), ("coef", coef)):
            out["%s.%s" % (fn, k)] = a[keep]
    # (a subdirectory: conftest.golden_names() takes every file of the top level for a trajectory fixture)
    path = os.path.join(HERE, "leaf_f32", "leaf_f32_ref.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (os.path.relpath(path, HERE), os.path.getsize(path)))


if __name__ == "__main__":
    main()
