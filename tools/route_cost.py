"""What catchment routing costs: lgar_catchment_route (forward and reverse) and lgar_catchment_route_grad over fp64 [T, B]
matrices of catchment sums.
(dev tool)  usage: python tools/route_cost.py [quick]

Cases: T = 144 rows with B = 64, 4096 and 65 536 catchments and K = 5 and 64 ordinates, shared and per-catchment; and one
streaming case, T = 8760 (a year of hourly rows) x B = 65 536 with K = 64 per-catchment ordinates (4.6 GB a matrix: beyond the
256 MB last-level cache).  `quick` leaves the streaming case out.  Per case and operation: device-event time of one call
(median of 7 after 2 warm-up calls) and GB/s on the algorithmic bytes -- x, y and g once each (the gradient: x, gy and its
[K, B] result once each).

The yardstick, alternating with the kernel in the same process on the same tensors: the plain torch statement of the same
convolution -- K shifted addcmul_ into a zeroed output (forward: y[k:] += g[k] * x[:T - k]; reverse: y[:T - k] += g[k] * x[k:]);
for the gradient K products summed over the rows ((gy[k:] * x[:T - k]).sum(0)).  The condition of DESIGN.md section 12: at no
shape is the kernel's median above the torch statement's median by more than that statement's own max - min.
One JSON line per result; LGAR_LIB selects a measurement variant (build.build_variant("route_tiled", ["-DLGAR_ROUTE_TILED"]))."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lgar_py_amd.catchments import CatchmentRouting

quick = len(sys.argv) > 1 and sys.argv[1] == "quick"
REPS, WARM = 7, 2


def timed_pair(kernel, torch_fn):
    """kernel and yardstick alternating: (sorted kernel us, sorted yardstick us)"""
    us = ([], [])
    for i in range(WARM + REPS):
        for which, fn in enumerate((kernel, torch_fn)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= WARM:
                us[which].append(1e3 * a.elapsed_time(b))
    return sorted(us[0]), sorted(us[1])


def report(op, T, B, K, per, nbytes, ker, ref):
    med, rmed = ker[len(ker) // 2], ref[len(ref) // 2]
    print(json.dumps({"mode": "route_cost", "op": op, "T": T, "B": B, "K": K, "per_catchment": per, "us_median": med, "us_min": ker[0],
                      "us_max": ker[-1], "torch_us_median": rmed, "torch_us_min": ref[0], "torch_us_max": ref[-1], "reps": REPS,
                      "algorithmic_bytes": nbytes, "GBps": nbytes / (med * 1e-6) / 1e9, "torch_GBps": nbytes / (rmed * 1e-6) / 1e9,
                      "kernel_over_torch": med / rmed, "holds": bool(med <= rmed + (ref[-1] - ref[0])),
                      "library": os.environ.get("LGAR_LIB", "default")}), flush=True)


cases = [(144, B, K, per) for B in (64, 4096, 65536) for K in (5, 64) for per in (False, True)]
if not quick:
    cases.append((8760, 65536, 64, True))
gen = torch.Generator(device="cuda").manual_seed(0)
for T, B, K, per in cases:
    x = torch.rand(T, B, dtype=torch.float64, device="cuda", generator=gen)
    gy = torch.rand(T, B, dtype=torch.float64, device="cuda", generator=gen)
    g = torch.rand((B, K) if per else (K,), dtype=torch.float64, device="cuda", generator=gen)
    r = CatchmentRouting(g, n_catchments=B)
    G = r.ordinates  # [K, B] or [K]
    y = torch.empty_like(x)
    gbytes = 8 * (K * B if per else K)

    def torch_forward():
        y.zero_()
        for k in range(min(K, T)):
            y[k:].addcmul_(G[k], x[:T - k])

    def torch_reverse():
        y.zero_()
        for k in range(min(K, T)):
            y[:T - k].addcmul_(G[k], gy[k:])

    def torch_grad():
        return torch.stack([(gy[k:] * x[:T - k]).sum(dim=0) for k in range(K)])

    report("forward", T, B, K, per, 16 * T * B + gbytes, *timed_pair(lambda: r.route(x, carry=False), torch_forward))
    report("reverse", T, B, K, per, 16 * T * B + gbytes, *timed_pair(lambda: r.adjoint(gy), torch_reverse))
    if per:  # (the kernel is the same for shared ordinates: their gradient is this one summed over b)
        report("ordinate_grad", T, B, K, per, 16 * T * B + 8 * K * B, *timed_pair(lambda: r.ordinate_grad(x, gy), torch_grad))
    del x, gy, y, r
    torch.cuda.empty_cache()
