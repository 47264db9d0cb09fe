"""Differentiable LGAR: torch autograd through the HIP kernels.

The reference differentiates forward() by recording every scalar torch op
(/root/reference/dpLGAR/agents/DifferentiableLGAR.py:119,163).  Here the vector-Jacobian product is assembled from
forward-mode tangents computed on the GPU (csrc/lgar_tangent_nl.hip): columns are independent, so one tangent launch
with a one-hot direction over (alpha | n | Ksat, layer) yields d runoff_t / d p for every column's own parameter,
contracted on the fly with the incoming gradient.  3 x L launches per backward, nothing stored per step.
Line-search offsets are constants w.r.t. the parameters, exactly as in the reference (Layer.py:277-288, 683-696).

Both entry points are ordinary torch.autograd.Function nodes whose inputs are the parameters, so the outputs carry a
grad_fn that reaches them (models/dpLGAR.py:299) and torch.autograd.grad / loss.backward() both work.
"""
import weakref

import torch

from ._capi import ST_FAULT_MASK
from .catchments import CatchmentMap
from .engine import LgarEngine, LgarError, LgarStatusError
from .forcing import ForcingDirections

KINDS = ("alpha", "n", "ksat")
# the directions of a backward pass ride side by side as extra columns of a tangent launch (column-major: column
# c * D + b integrates column c's parameters perturbed in direction b, so that a column's directions sit in adjacent lanes);
# forcing and weights are NOT replicated -- the kernels broadcast them (LgarDims.forcing_columns / forcing_group).  Above this
# many (column, direction) pairs the directions go in groups; in fp64 fast modes the lanes of a column share the Geff trapezoid.
BATCH_DIRECTIONS_MAX_COLUMNS = 1 << 23
SHARE_MIN_LANES = 65536  # columns x directions: one wave on every SIMD of the chip


def _forcing_lanes(fd, part, T, Nf, dtype, device):
    """The forcing tangents of one group of directions: {} when `part` holds no ("forcing", k), else d_precip / d_pet
    [T, Nf, len(part)] with fd's series k in the lane of ("forcing", k) and zeros in the lanes of the parameter directions."""
    lanes = [(b, key[1]) for b, key in enumerate(part) if key[0] == "forcing"]
    out = {}
    for nm, src in (("d_precip", fd.d_precip), ("d_pet", fd.d_pet)) if lanes else ():
        if src is not None:
            d = torch.zeros(T, Nf, len(part), dtype=dtype, device=device)
            for b, k in lanes:
                d[:, :, b] = src[k].to(device, dtype)
            out[nm] = d
    return out


def _windowed_tangent(e, direction, precip, pet, w_runoff, w_perc, start, moisture, group, kw, fkw):
    """One group of directions over the whole run in windows of `every` rows, the state carried (LgarEngine.tangent_window: the
    bits of one call), with snapshot s's cotangent contracted into the carried gradient after window s
    (LgarEngine.soil_moisture_tangent); trailing T % every rows form a last window without one.  moisture = (every, device
    edges or None, number of bins, what, cot [T // every, bins, N] fp64).  Returns (grad[M], status[M])."""
    every, e_dev, n_bins, what, cot = moisture
    T = int(precip.shape[0])
    rows = lambda t, lo, hi: None if t is None else t[lo:hi]
    grad = torch.zeros(e.N, dtype=e.dtype, device=e.device)
    status = torch.zeros(e.N, dtype=torch.int32, device=e.device)
    state = start
    for lo in range(0, T, every):
        hi = min(lo + every, T)
        full = hi - lo == every
        grad, _, st, end = e.tangent_window(direction, precip[lo:hi], pet[lo:hi], w_runoff=rows(w_runoff, lo, hi), w_perc=rows(w_perc, lo, hi),
                                            start=state, keep_state=full, **kw, **{nm: d[lo:hi] for nm, d in fkw.items()})
        status |= st
        if full:
            e._moisture_tangent_launch(end, e_dev, n_bins, what, None, cot[lo // every], group)
            state = end
    return grad, status


def parameter_vjp(eng, precip, pet, w_runoff, w_perc, wanted, check=True, forcing_map=None, start=None, forcing_directions=None,
                  moisture=None):
    """Vector-Jacobian product for every (kind, layer) in `wanted` (list of (kind, l)).
    Returns ({(kind, l): grad[N]}, tangent_status[N]).  Columns are independent, so the directions are laid side by side as
    len(wanted) * N columns of a single launch (fills the chip even for ensembles of 10^5 columns; very large jobs go in
    groups of directions).  A column whose tangent integration faults (status != 0: NaN, iteration cap, front overflow
    ...) has no valid gradient: with check=True that raises LgarStatusError (a ValueError, like the reference's physics
    faults), with check=False its gradient entries are zeroed and the status tensor says which columns those are.
    forcing_map: a forcing.ForcingMap with one entry per column -- precip / pet are [T, B], the weights stay [T, N].
    start: None = the run starts from a fresh state; an engine.EngineState (LgarEngine.snapshot()) = the rows are a window that
    starts from that FIXED state (LgarEngine.tangent_window: the derivative of forward() from the state, nothing flows into the
    run that produced it).  Where the directions ride side by side the state is laid out with them (repeat_interleave: (5 F +
    NSCAL) * Dg * N values, small beside the [T, N] arrays).
    forcing_directions: a forcing.ForcingDirections over the run's forcing columns; `wanted` may then hold ("forcing", k) as
    well: lane k of a column integrates the forcing tangent d_precip[k] / d_pet[k] of the column's forcing cell
    (lgar_forward_tangent_forced) and the result is the column's own share of d loss / d params[k] of its cell.  Groups without
    such a lane are launched as they always were.
    moisture: None, or (every, edges, what, cot) with cot [T // every, bins, N] the cotangent of the soil-moisture snapshots
    LgarEngine.run_with_soil_moisture(every, edges, what) takes: every group of directions then goes through tangent_window in
    windows of `every` rows, the state carried from `start`, and after window s the contraction of snapshot s's cotangent with the
    tangent of the bins is added to the carried gradient (LgarEngine.soil_moisture_tangent).  The result is the vector-Jacobian
    product of the two series AND the snapshots.  None is the code path as it always was."""
    L, N, D = eng.L, eng.N, len(wanted)
    if moisture is not None:
        every, edges, what, cot = moisture
        every = int(every)
        if every < 1:
            raise LgarError("every must be >= 1")
        e_dev, n_bins = eng._moisture_bins(edges, what, need_state=False)
        want = (int(precip.shape[0]) // every, n_bins, N)
        if (not isinstance(cot, torch.Tensor) or tuple(cot.shape) != want or cot.dtype != torch.float64 or cot.device != eng.status.device):
            raise LgarError("the soil-moisture cotangent must be a fp64 %s tensor on %s" % (list(want), eng.device))
        moisture = (every, e_dev, n_bins, what, cot.contiguous())
    fd = forcing_directions
    T, Nf = (int(precip.shape[0]), int(precip.shape[1])) if fd is not None else (0, 0)
    out = {}
    status = torch.zeros(N, dtype=torch.int32, device=eng.device)
    if D == 0:
        return out, status
    group = max(1, min(D, BATCH_DIRECTIONS_MAX_COLUMNS // max(N, 1)))
    d = eng.dims
    # fp64 fast modes: the directions of a column sit in adjacent lanes that SHARE the Geff trapezoid (LgarDims.tangent_share =
    # group width; the tangent of the trapezoid needs only five direction-independent sums, so all 3 x L directions of a column
    # fit one group: 9 lanes for three layers, seven groups per wavefront)
    # (only when the launch fills the chip: a small job is bound by the latency of ONE wave)
    share = (eng.dtype == torch.float64 and d.search_mode != 0 and not d.use_closed_form_G and 2 <= group <= 32
             and N * group >= SHARE_MIN_LANES)
    for g0 in range(0, D, group):
        part = wanted[g0:g0 + group]
        Dg = len(part)
        if Dg == 1:
            kind, l = part[0]
            if kind == "forcing":
                direction, fkw = {}, _forcing_lanes(fd, part, T, Nf, eng.dtype, eng.device)
            else:
                dmat = torch.zeros(L, N, dtype=eng.dtype, device=eng.device)
                dmat[l] = 1.0
                direction, fkw = {kind: dmat}, {}
            if moisture is not None:
                out[(kind, l)], st = _windowed_tangent(eng, direction, precip, pet, w_runoff, w_perc, start, moisture, 1,
                                                       dict(forcing_map=forcing_map), fkw)
            elif start is None:
                out[(kind, l)], _, st = eng.tangent(direction, precip, pet, w_runoff=w_runoff, w_perc=w_perc, forcing_map=forcing_map, **fkw)
            else:
                out[(kind, l)], _, st, _ = eng.tangent_window(direction, precip, pet, w_runoff=w_runoff, w_perc=w_perc,
                                                              forcing_map=forcing_map, start=start, keep_state=False, **fkw)
            status |= st
            continue
        # column n's Dg directions sit in ADJACENT lanes (column n * Dg + b): they follow the same branches, so a wavefront
        # diverges over 64 / Dg columns instead of 64; the kernel reads forcing / weight column c // Dg (forcing_group)
        rep = lambda t: t.repeat_interleave(Dg, dim=1)
        big = eng.like(rep(eng.alpha), rep(eng.n), rep(eng.ksat), rep(eng.theta_e), rep(eng.theta_r), rep(eng.thickness),
                       with_state=False)
        dirs = {k: torch.zeros(L, Dg * N, dtype=eng.dtype, device=eng.device) for k in KINDS}
        for b, (kind, l) in enumerate(part):
            if kind != "forcing":
                dirs[kind][l, b::Dg] = 1.0
        # forcing / weights broadcast by the kernel (forcing_group); the SAME map, not replicated: entry c // Dg of the launch is
        # the original column, and the incoming [T, N] gradient is the [T, Dg * N // Dg] weight array as it is
        layout = dict(forcing_group=Dg, share=Dg if share else 0, forcing_map=forcing_map)
        fkw = _forcing_lanes(fd, part, T, Nf, eng.dtype, eng.device)
        kw = dict(w_runoff=w_runoff, w_perc=w_perc, **layout, **fkw)
        if moisture is not None:
            g, st = _windowed_tangent(big, dirs, precip, pet, w_runoff, w_perc, None if start is None else start.expand(Dg), moisture,
                                      Dg, layout, fkw)
        elif start is None:
            g, _, st = big.tangent(dirs, precip, pet, **kw)
        else:
            g, _, st, _ = big.tangent_window(dirs, precip, pet, start=start.expand(Dg), keep_state=False, **kw)
        for b, key in enumerate(part):
            out[key] = g[b::Dg].contiguous()
            status |= st[b::Dg]
    status &= ST_FAULT_MASK
    bad = status != 0
    if bool(bad.any()):
        if check:
            first = int(torch.nonzero(bad)[0].item())
            raise LgarStatusError("%d of %d columns faulted in the tangent (gradient) integration; first column %d, status %d"
                                  % (int(bad.sum().item()), N, first, int(status[first].item())))
        for key in out:
            out[key] = torch.where(bad, torch.zeros_like(out[key]), out[key])
    return out, status


def _open_run(ctx, alpha, n, ksat, theta_e, theta_r, thickness, precip, pet, engine_kw):
    """What the forward passes of the series nodes do alike before the run: the engine over the detached parameters, the forcing as
    the backward pass will pair it with the incoming gradient, the given state restored, and on ctx what backward needs.  Returns
    (engine, precip, pet, forcing_map, check, state_out, status_out)."""
    engine_kw = dict(engine_kw)
    fd = engine_kw.pop("forcing_directions", None)
    check = engine_kw.pop("check", True)
    status_out = engine_kw.pop("status_out", None)
    fmap = engine_kw.pop("forcing_map", None)
    start = engine_kw.pop("initial_state", None)
    state_out = engine_kw.pop("state_out", None)
    eng = LgarEngine(alpha.detach(), n.detach(), ksat.detach(), theta_e, theta_r, thickness, **engine_kw)
    precip, pet = torch.as_tensor(precip), torch.as_tensor(pet)
    if fd is not None and fmap is None and (precip.dim() != 2 or precip.shape[1] != eng.N):
        raise LgarError("forcing_directions need [T, N] forcing or a forcing_map, not the broadcast [T, Nf] layout: a forcing "
                        "cell there is read by columns that are not one group, and its parameters' lanes have no place")
    if fmap is not None:
        pass  # [T, B] forcing through the map, forward and backward: nothing is expanded (the weights do not go through it)
    elif precip.dim() == 2 and precip.shape[1] != eng.N:
        # broadcast forcing [T, Nf]: the backward pass pairs the forcing with the incoming [T, N] gradient column by
        # column (the tangent kernels take one layout for both), so the series is expanded here, once
        if eng.N % max(int(precip.shape[1]), 1) != 0 or precip.shape != pet.shape:
            raise LgarError("forcing must be [T, N] or [T, Nf] with Nf dividing N = %d; got %s / %s"
                            % (eng.N, tuple(precip.shape), tuple(pet.shape)))
        rep = eng.N // int(precip.shape[1])
        precip, pet = precip.repeat(1, rep).contiguous(), pet.repeat(1, rep).contiguous()  # column c reads c % Nf
    if fd is not None:
        if fd.K and fd.shape != (fd.K, int(precip.shape[0]), int(precip.shape[1])):
            raise LgarError("forcing_directions hold %s, the forcing is [T, B] = %s: d_precip / d_pet must be [K, T, B]"
                            % (fd.shape, tuple(precip.shape)))
    if start is not None:
        eng.restore(start)  # (in place of the fresh state the constructor left)
    ctx.engine = eng
    ctx.forcing = (precip, pet)
    ctx.forcing_map = fmap
    ctx.start = start
    ctx.forcing_directions = fd
    ctx.in_dtypes = (alpha.dtype, n.dtype, ksat.dtype)
    ctx.check = check
    ctx.status_out = status_out
    return eng, precip, pet, fmap, check, state_out, status_out


class LgarSeriesFunction(torch.autograd.Function):
    """(alpha, n, ksat)[L, N] -> (runoff, percolation)[T, N] from a fresh state, or from a given one held fixed; differentiable
    in alpha/n/ksat and, through forcing_directions, in the parameters the forcing was computed from (the inputs behind engine_kw)."""

    @staticmethod
    def forward(ctx, alpha, n, ksat, theta_e, theta_r, thickness, precip, pet, engine_kw, *forcing_params):
        eng, precip, pet, fmap, check, state_out, status_out = _open_run(ctx, alpha, n, ksat, theta_e, theta_r, thickness, precip, pet, engine_kw)
        out = eng.forward(precip, pet, series=("runoff", "percolation"), check=check, forcing_map=fmap)
        if state_out is not None:
            state_out.append(eng.snapshot())
        if status_out is not None:
            status_out.append(eng.status)
        return out["runoff"], out["percolation"]

    @staticmethod
    def backward(ctx, g_runoff, g_perc):
        grads, forcing_grads = _series_backward(ctx, g_runoff, g_perc, 9)
        return (*grads, None, None, None, None, None, None, *forcing_grads)


def _series_backward(ctx, g_runoff, g_perc, first_forcing_input, moisture=None):
    """What the backward passes of the series nodes do alike: the incoming gradients masked where the forward run faulted, one
    parameter_vjp over the wanted (kind, layer) and forcing lanes, its status reported, the gradients gathered.  Returns
    ([d alpha, d n, d ksat] each [L, N] or None, the gradients of forcing_directions.params).  first_forcing_input: where the
    forcing parameters stand among the node's inputs.  moisture: parameter_vjp's (None: launch for launch what it was)."""
    eng = ctx.engine
    precip, pet = ctx.forcing
    wanted = [(kind, l) for ki, kind in enumerate(KINDS) if ctx.needs_input_grad[ki] for l in range(eng.L)]
    # columns that already faulted in the forward run are the caller's to mask (status_out); they carry no gradient
    fwd_bad = (eng.status & ST_FAULT_MASK) != 0
    keep = (~fwd_bad).to(g_runoff.dtype)[None, :] if g_runoff is not None else None
    gr = None if g_runoff is None else g_runoff * keep
    gp = None if g_perc is None else g_perc * ((~fwd_bad).to(g_perc.dtype)[None, :])
    fd = ctx.forcing_directions
    # the forcing's parameters ride as K more lanes per column in the same groups: one batch of launches
    wanted += [("forcing", k) for k in range(fd.K if fd is not None else 0) if ctx.needs_input_grad[first_forcing_input + k]]
    more = {} if moisture is None else dict(moisture=moisture)
    vj, st = parameter_vjp(eng, precip, pet, gr, gp, wanted, check=False, forcing_map=ctx.forcing_map, start=ctx.start,
                           forcing_directions=fd, **more)
    st = torch.where(fwd_bad, torch.zeros_like(st), st)
    if ctx.status_out is not None:
        ctx.status_out.append(st)  # [forward status, tangent status]
    if ctx.check and bool((st != 0).any()):
        raise LgarStatusError("%d columns faulted in the tangent (gradient) integration" % int((st != 0).sum().item()))
    grads = []
    for ki, kind in enumerate(KINDS):
        if not ctx.needs_input_grad[ki]:
            grads.append(None)
            continue
        g = torch.stack([vj[(kind, l)] for l in range(eng.L)])
        g = torch.where(fwd_bad[None, :], torch.zeros_like(g), g)
        grads.append(g.to(ctx.in_dtypes[ki]))
    return grads, _forcing_parameter_grads(ctx, fd, vj, fwd_bad, first_forcing_input)


def _forcing_parameter_grads(ctx, fd, vj, fwd_bad, first_forcing_input=9):
    """d loss / d params[k] of a ForcingDirections from the columns' shares vj[("forcing", k)] [N]: with a forcing_map the columns
    of a cell are summed in the fixed order of CatchmentMap.sums (its bits, whatever the launch), with [T, N] forcing a column is
    its own cell; a scalar parameter gets the sum over the cells."""
    if fd is None:
        return ()
    eng = ctx.engine
    ks = [k for k in range(fd.K) if ctx.needs_input_grad[first_forcing_input + k]]
    cells = {}
    if ks:
        shares = torch.stack([torch.where(fwd_bad, torch.zeros_like(vj[("forcing", k)]), vj[("forcing", k)]) for k in ks])
        shares = shares.to(torch.float64).contiguous()
        if ctx.forcing_map is not None:
            shares = ctx.forcing_map.cell_map(CatchmentMap).sums(shares)  # (the map of the cells is made once per ForcingMap)
        cells = dict(zip(ks, shares))
    out = []
    for k, p in enumerate(fd.params):
        g = cells.get(k)
        out.append(None if g is None else (g.sum() if p.dim() == 0 else g).to(p.device, p.dtype))
    return tuple(out)


def lgar_series(alpha, n, ksat, theta_e, theta_r, thickness, precip, pet, **engine_kw):
    """Differentiable run: parameters [L, N] (torch tensors, may require grad), forcing [T, N] -> runoff, percolation [T, N].
    engine_kw: LgarEngine keywords, plus check=False to keep going when columns fault: pass status_out=[] to receive the
    forward status tensor (appended by the forward pass) and the tangent status tensor (appended by the backward pass);
    faulted columns get zero gradient.  forcing_map=<forcing.ForcingMap>: the forcing is [T, B] and column c reads forcing column
    forcing_map.index[c], in the forward run and in the backward pass alike: no [T, N] forcing exists anywhere.
    initial_state=<engine.EngineState> (LgarEngine.snapshot() of a spun-up engine over the same columns): the run starts from that
    state instead of a fresh one, and the state is a CONSTANT: the gradient is the derivative, with respect to the parameters, of
    the run from the fixed state over these rows.  Nothing flows into the spin-up that produced the state, although that spin-up
    depended on the same parameters -- the usual "warm-up excluded from the gradient".  The backward pass integrates the tangent
    over these rows only.  state_out=[]: the forward pass appends the end state (an EngineState), which the next window takes as
    its initial_state.  initial_state=None is a run from a fresh state.
    forcing_directions=<forcing.ForcingDirections> (forcing.scaled_forcing, snow.catchment_snow_directions): the forcing was
    computed from K parameters per forcing cell and fd holds its derivatives along them; fd.params become inputs of the node and
    receive d loss / d params[k] ([B], or the sum over the cells for a scalar), from K more lanes per column in the backward
    pass's launches.  The forcing must be [T, N] or go through a forcing_map (the broadcast [T, Nf] layout raises LgarError); it
    works with initial_state.  The graph of `precip` / `pet` themselves is NOT followed: they are constants to this node, and
    whatever produced them receives a gradient through forcing_directions or not at all.  Without forcing_directions the
    backward pass is what it was, launch for launch."""
    fd = engine_kw.get("forcing_directions")
    if fd is not None and not isinstance(fd, ForcingDirections):
        raise LgarError("forcing_directions must be a forcing.ForcingDirections; got %s" % type(fd).__name__)
    return LgarSeriesFunction.apply(alpha, n, ksat, theta_e, theta_r, thickness, precip, pet, engine_kw, *(fd.params if fd is not None else ()))


class LgarMoistureSeriesFunction(torch.autograd.Function):
    """LgarSeriesFunction with the depth-binned soil moisture after every `every` rows as a third output
    ([T // every, bins, N]); differentiable in what LgarSeriesFunction is differentiable in."""

    @staticmethod
    def forward(ctx, alpha, n, ksat, theta_e, theta_r, thickness, precip, pet, bins, engine_kw, *forcing_params):
        every, edges, what = bins
        eng, precip, pet, fmap, check, state_out, status_out = _open_run(ctx, alpha, n, ksat, theta_e, theta_r, thickness, precip, pet, engine_kw)
        out = eng.run_with_soil_moisture(precip, pet, every, edges, what, series=("runoff", "percolation"), check=check, forcing_map=fmap)
        if state_out is not None:
            state_out.append(eng.snapshot())
        if status_out is not None:
            status_out.append(eng.status)
        ctx.bins = (int(every), edges, what)
        return out["runoff"], out["percolation"], out["soil_moisture"]

    @staticmethod
    def backward(ctx, g_runoff, g_perc, g_moist):
        eng = ctx.engine
        every, edges, what = ctx.bins
        S, D = int(ctx.forcing[0].shape[0]) // every, eng.L if edges is None else len(edges) - 1
        if g_moist is None:
            cot = torch.zeros(S, D, eng.N, dtype=torch.float64, device=eng.device)
        else:
            # fp64, and nothing for the columns that faulted in the forward run (a select: their leftover state may have made a
            # NaN of the snapshot and of its cotangent); a bin below the column is skipped inside the contraction
            fwd_bad = (eng.status & ST_FAULT_MASK) != 0
            cot = g_moist.to(eng.device, torch.float64)
            cot = torch.where(fwd_bad[None, None, :], torch.zeros_like(cot), cot).contiguous()
        grads, forcing_grads = _series_backward(ctx, g_runoff, g_perc, 10, moisture=(every, edges, what, cot))
        return (*grads, None, None, None, None, None, None, None, *forcing_grads)


def lgar_moisture_series(alpha, n, ksat, theta_e, theta_r, thickness, precip, pet, every, edges=None, what="theta", **engine_kw):
    """lgar_series with the soil-moisture profile as a third, differentiable output: returns (runoff [T, N], percolation [T, N],
    moisture [T // every, D, N]), moisture[s] being LgarEngine.soil_moisture(edges, what) of the state after row
    (s + 1) * every - 1 (edges: [D + 1] depths in cm, None = each column's own layers; what: "theta" or "storage").
    engine_kw: what lgar_series takes (forcing_map, initial_state, state_out, check, status_out, forcing_directions, LgarEngine's).

    Forward: LgarEngine.run_with_soil_moisture's windows -- the moisture has its bits, the two series lgar_series' bits.
    Backward: every group of directions parameter_vjp forms goes through LgarEngine.tangent_window in windows of `every` rows, the
    tangent state carried; after window s, LgarEngine.soil_moisture_tangent contracts snapshot s's cotangent (taken as fp64, zero
    for columns that faulted in the forward run) with the tangent of the bins into the carried gradient.  A trailing T % every
    rows form a last window without a snapshot.  Gradients reach alpha, n, ksat and forcing_directions.params as in lgar_series;
    theta_e, theta_r, the thickness and the initial state are constants.  A bin wholly below the column reads NaN with
    what="theta": its cotangent contributes nothing, whatever it holds (mask such entries out of a loss, or a NaN loss results
    from the values themselves).
    Catchment means compose: lg.catchment_sum(moisture[s], cmap) (CatchmentMap.sums over the [D, N] rows of one snapshot, with
    area weights) gives [D, B] catchment moisture, which CatchmentScore takes against satellite or in-situ observations; its
    gradient comes back through this node."""
    fd = engine_kw.get("forcing_directions")
    if fd is not None and not isinstance(fd, ForcingDirections):
        raise LgarError("forcing_directions must be a forcing.ForcingDirections; got %s" % type(fd).__name__)
    return LgarMoistureSeriesFunction.apply(alpha, n, ksat, theta_e, theta_r, thickness, precip, pet, (every, edges, what), engine_kw,
                                            *(fd.params if fd is not None else ()))


class _ChunkFunction(torch.autograd.Function):
    """One model.forward() call's (runoff, percolation) block as an autograd node with the parameters as inputs.
    `token` chains the nodes of an epoch in call order, so autograd necessarily reaches chunk 0 last: there the weights
    recorded by all chunks are turned into parameter gradients by ONE batch of tangent launches over the whole series."""

    @staticmethod
    def forward(ctx, tape, ci, token, runoff, perc, *params):
        ctx.tape_ref, ctx.ci, ctx.n_params = weakref.ref(tape), ci, len(params)  # the model owns the tape; the graph does not
        ctx.set_materialize_grads(False)
        return runoff.clone(), perc.clone(), token.new_zeros(())

    @staticmethod
    def backward(ctx, g_runoff, g_perc, g_token):
        tape = ctx.tape_ref()
        if tape is None:
            raise LgarError("backward through a model that no longer exists")
        tape.add_weights(ctx.ci, g_runoff, g_perc)
        if ctx.ci == 0:
            return (None, None, None, None, None, *tape.finalize())
        # a defined (zero) gradient for the token keeps the chain down to chunk 0 alive
        return (None, None, torch.zeros((), dtype=torch.float64), None, None, *((None,) * ctx.n_params))


class StepTape:
    """Autograd for the reference's calling convention (`model(x[i])` once per forcing row -- or a whole [T, N, 2] block --
    with the loss taken at the end of the epoch).  Every returned runoff/percolation block is the output of an autograd
    node whose inputs are the model's parameters; the backward pass records the gradient each block receives and, at the
    node of the epoch's first block, ONE batch of tangent launches over the recorded forcing series turns the recorded
    weights into parameter gradients -- O(T) work per epoch, nothing stored per step but the forcing rows."""

    def __init__(self, model):
        self._model = weakref.ref(model)  # the model owns the tape, not the other way round
        self.reset()

    def reset(self):
        self.x = []          # forcing chunks [Tc, N, 2] since the last set_internal_states()
        self.n_rows = 0      # ... and how many forcing rows they hold
        self.w = {}          # (chunk, 0|1) -> gradient received, [Tc, N]
        self.token = None
        self.versions = None
        self._params = None  # the model's parameters in (alpha, n, ksat) x layer order, looked up once per recorded series

    def _param_lists(self):
        m = self._model()
        if m is None:
            raise LgarError("the model this tape belongs to is gone")
        return m, (("alpha", m.alpha), ("n", m.n), ("ksat", m.ksat))

    def record(self, x_chunk, runoff_chunk, perc_chunk, steps_before=None):
        """x_chunk [Tc, N, 2]; runoff/perc [Tc, N] (engine outputs); steps_before: forcing rows the model had integrated
        since set_internal_states() before this chunk.  Returns the graph-connected blocks."""
        if self._params is None:
            _, plists = self._param_lists()
            self._params = [p for _, pl in plists for p in pl]
        params = self._params
        recorded = self.n_rows
        if steps_before is not None and steps_before != recorded:
            # finalize() re-integrates the tangent from a FRESH state over the recorded rows only: rows the model advanced
            # off the tape (under torch.no_grad(), or while no parameter required grad -- a spin-up, say) would make the
            # backward pass replay another forcing series and another state than the forward run
            raise LgarError("the model advanced %d forcing rows since set_internal_states() that are not on the autograd tape "
                            "(%d recorded): forward() calls under torch.no_grad() cannot be mixed with differentiated ones "
                            "within one series; call set_internal_states() first" % (steps_before - recorded, recorded))
        versions = tuple(p._version for p in params)
        if self.versions is None:
            self.versions = versions
        elif versions != self.versions:
            raise LgarError("parameters changed in the middle of a recorded series (update_soil_parameters / optimizer step "
                            "before backward): call set_internal_states() first, the gradient would belong to another run")
        ci = len(self.x)
        self.x.append(x_chunk.detach())
        self.n_rows += int(x_chunk.shape[0])
        token = self.token if self.token is not None else torch.zeros((), dtype=torch.float64)
        r, p, self.token = _ChunkFunction.apply(self, ci, token, runoff_chunk, perc_chunk, *params)
        return r, p

    def add_weights(self, ci, g_runoff, g_perc):
        for which, g in enumerate((g_runoff, g_perc)):
            if g is None:
                continue
            key = (ci, which)
            self.w[key] = self.w[key] + g.detach() if key in self.w else g.detach().clone()

    def finalize(self):
        """Parameter gradients (in parameter order) from the weights recorded so far; called by chunk 0's backward."""
        m, plists = self._param_lists()
        eng = m.engine
        X = torch.cat(self.x).to(eng.device, eng.dtype)  # [T, N, 2]
        T = X.shape[0]
        if getattr(m, "steps_advanced", T) != T:
            raise LgarError("the tape holds %d forcing rows but the model advanced %d since set_internal_states(): the gradient "
                            "would belong to another run" % (T, m.steps_advanced))
        W = torch.zeros(2, T, eng.N, dtype=eng.dtype, device=eng.device)
        t0 = 0
        for ci, xc in enumerate(self.x):
            for which in (0, 1):
                g = self.w.get((ci, which))
                if g is not None:
                    W[which, t0:t0 + xc.shape[0]] = g.to(eng.device, eng.dtype).reshape(xc.shape[0], eng.N)
            t0 += xc.shape[0]
        self.w = {}
        precip, pet = X[:, :, 0].contiguous(), X[:, :, 1].contiguous()
        ff = float(m.cfg.constants.frozen_factor)
        wanted = [(kind, l) for kind, plist in plists for l, p in enumerate(plist) if p.requires_grad]
        vj, _ = parameter_vjp(eng, precip, pet, W[0], W[1], wanted, check=True)
        grads = []
        for kind, plist in plists:
            for l, p in enumerate(plist):
                if not p.requires_grad:
                    grads.append(None)
                    continue
                g = vj[(kind, l)]
                if kind == "ksat":
                    g = g / ff  # the Parameter already carries frozen_factor (models/dpLGAR.py:57)
                g = g.to(torch.float64).to(p.device)
                g = g.sum() if p.dim() == 0 else g
                grads.append(g.to(p.dtype))
        return tuple(grads)
