"""What catchment scores cost: lgar_catchment_moments (one CatchmentScore.moments call: four launches) and
lgar_catchment_moments_grad (one backward call through scores.catchment_moments) over fp64 [T, B] simulations against [To, B]
observations with 10 % gaps.
(dev tool)  usage: python tools/score_cost.py [quick] [out.jsonl]

Cases: T in {144, 8760} model rows x B in {1, 64, 4096, 65 536} catchments x window in {1, 12} (To = T / window), and one
streaming case, To = 8760 observation rows at window = 12 (a year of 5-minute rows against hourly gauges) x B = 4096 (3.4 GB
of sim: beyond the 256 MB last-level cache).  `quick` leaves out the streaming case and T = 8760 at B = 65 536.  Per case and
operation: device-event time of one call (median of 7 after 2 warm-up calls) and GB/s on the algorithmic bytes -- sim and obs
twice each for the moments (two passes), once each plus one write of grad_sim for the gradient.

The yardstick, alternating with the kernel in the same process on the same tensors: the plain torch statement of the same
quantities -- isfinite mask, where, the window's mean, two masked passes ([7, B]); for the gradient, autograd of that statement
(backward of sum(moments * v) with the graph retained, against catchment_moments' backward of the same).  The condition of
DESIGN.md section 12, applied in section 13: at no shape is the kernel's median above the torch statement's median by more than
that statement's own max - min.  One JSON line per result, also appended to out.jsonl when given."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lgar_py_amd.scores import CatchmentScore, catchment_moments

args = sys.argv[1:]
quick = "quick" in args
out_path = next((a for a in args if a != "quick"), None)
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


def report(op, T, B, window, nbytes, ker, ref):
    med, rmed = ker[len(ker) // 2], ref[len(ref) // 2]
    line = json.dumps({"mode": "score_cost", "op": op, "T": T, "To": T // window, "B": B, "window": window, "us_median": med, "us_min": ker[0],
                       "us_max": ker[-1], "torch_us_median": rmed, "torch_us_min": ref[0], "torch_us_max": ref[-1], "reps": REPS,
                       "algorithmic_bytes": nbytes, "GBps": nbytes / (med * 1e-6) / 1e9, "torch_GBps": nbytes / (rmed * 1e-6) / 1e9,
                       "kernel_over_torch": med / rmed, "holds": bool(med <= rmed + (ref[-1] - ref[0])),
                       "library": os.environ.get("LGAR_LIB", "default")})
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as fh:
            fh.write(line + "\n")


def plain_moments(sim, obs, window):
    """The masked plain torch statement -> [7, B]"""
    To, B = obs.shape
    valid = torch.isfinite(obs)
    o = torch.where(valid, obs, torch.zeros_like(obs))
    s = sim.reshape(To, window, B).mean(dim=1)
    zero = torch.zeros_like(s)
    n = valid.sum(dim=0).to(torch.float64)
    mo, ms = o.sum(dim=0) / n, torch.where(valid, s, zero).sum(dim=0) / n
    d_o, d_s, e = torch.where(valid, o - mo, zero), torch.where(valid, s - ms, zero), torch.where(valid, s - o, zero)
    return torch.stack([n, mo, ms, (d_o * d_o).sum(dim=0), (d_s * d_s).sum(dim=0), (d_o * d_s).sum(dim=0), (e * e).sum(dim=0)])


cases = [(T, B, w) for T in (144, 8760) for B in (1, 64, 4096, 65536) for w in (1, 12) if not (quick and T * B > 2 ** 28)]
if not quick:
    cases.append((8760 * 12, 4096, 12))
gen = torch.Generator(device="cuda").manual_seed(0)
for T, B, window in cases:
    To = T // window
    sim = torch.rand(T, B, dtype=torch.float64, device="cuda", generator=gen)
    obs = torch.rand(To, B, dtype=torch.float64, device="cuda", generator=gen)
    obs[torch.rand(To, B, device="cuda", generator=gen) < 0.1] = float("nan")
    v = torch.rand(7, B, dtype=torch.float64, device="cuda", generator=gen)
    score = CatchmentScore(obs, window=window)
    nsim, nobs = 8 * T * B, 8 * To * B
    report("moments", T, B, window, 2 * (nsim + nobs), *timed_pair(lambda: score.moments(sim), lambda: plain_moments(sim, obs, window)))
    # the backward passes alone, on graphs built once
    leaf_k, leaf_t = sim.clone().requires_grad_(True), sim.clone().requires_grad_(True)
    fk, ft = (catchment_moments(leaf_k, score) * v).sum(), (plain_moments(leaf_t, obs, window) * v).sum()

    def back(f, leaf):
        leaf.grad = None
        f.backward(retain_graph=True)

    report("moments_grad", T, B, window, 2 * nsim + nobs, *timed_pair(lambda: back(fk, leaf_k), lambda: back(ft, leaf_t)))
    del sim, obs, v, score, leaf_k, leaf_t, fk, ft
    torch.cuda.empty_cache()
