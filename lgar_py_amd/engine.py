"""Many-column LGAR engine: owns the struct-of-arrays device state and drives the HIP kernels
through the C-ABI (include/lgar.h).  Host-side mirror of what dpLGAR(nn.Module) keeps per column
(/root/reference/dpLGAR/models/dpLGAR.py:97-147), laid out column-fastest in HBM.

PyTorch is plumbing here (device memory, streams); the computation is in csrc/*.hip.
"""
import ctypes as C

import torch

from . import _capi
from ._capi import ACC_NAMES, GMAX, LMAX, LMIN, NACC, NSCAL, LgarError
from ._capi import ptr as _ptr

BASIN_SCRATCH_BYTES = 8 << 30  # most series memory, over ALL basin names, an engine allocates on its own behind basin sums
PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
# LgarEngine's keyword settings and their defaults (the class docstring says what they mean); an engine keeps the ones it
# was built with in `settings`
SETTINGS = dict(dt_h=1.0, num_subcycles=1, initial_psi=2000.0, ponded_depth_max=0.0, wilting_point_psi=15495.0,
                frozen_factor=1.0, nint=120, giuh_ordinates=(0.06, 0.51, 0.28, 0.12, 0.03), dtype=torch.float64,
                device="cuda:0", iter_cap=0, search_mode=1, bottom_mode=0, use_closed_form_G=False, front_slots=None,
                geff_precision="native", forward_lanes=0, basin_scratch_bytes=BASIN_SCRATCH_BYTES)
_DIMS_SETTINGS = ("dt_h", "num_subcycles", "initial_psi", "ponded_depth_max", "wilting_point_psi", "frozen_factor", "nint",
                  "giuh_ordinates", "iter_cap", "search_mode", "bottom_mode", "use_closed_form_G", "forward_lanes")


_NO_GPU = "no ROCm GPU visible: the LGAR engine has no CPU fallback (device=%s)"
_DTYPES = "dtype must be torch.float32 or torch.float64"


class LgarStatusError(ValueError):
    """Physics fault in one or more columns (the reference raises ValueError / IndexError / AttributeError)."""


_VALUE_FIELDS = ("depth", "theta", "psi", "k", "dzdt", "scalars")  # what carries a tangent as well


class EngineState:
    """The column state of an LgarEngine at one moment (LgarEngine.snapshot()): clones of depth, theta, psi, k, dzdt, flags
    [front_slots, N], n_fronts [N], scalars [NSCAL, N] and status [N].  The run totals are bookkeeping of a run, not state."""
    FIELDS = _VALUE_FIELDS[:5] + ("flags", "n_fronts", "scalars", "status")

    def __init__(self, **tensors):
        for nm in self.FIELDS:
            setattr(self, nm, tensors[nm])

    N = property(lambda self: self.depth.shape[1])
    front_slots = property(lambda self: self.depth.shape[0])
    dtype = property(lambda self: self.depth.dtype)
    device = property(lambda self: self.depth.device)

    def expand(self, times):
        """Every column `times` times over, side by side (column c becomes columns c * times .. c * times + times - 1)."""
        return EngineState(**{nm: getattr(self, nm).repeat_interleave(times, dim=-1) for nm in self.FIELDS})

    def _struct(self):
        return _capi.LgarState(*[getattr(self, nm).data_ptr() for nm in self.FIELDS[:8]], None, None)


class TangentState:
    """What LgarEngine.tangent_window hands from one window to the next: the value state (an EngineState), the tangent of every
    value in it along the window's direction ({depth, theta, psi, k, dzdt: [front_slots, N], scalars: [NSCAL, N]}) and the
    gradient folded so far ([N])."""

    def __init__(self, value, tangent, grad):
        self.value, self.tangent, self.grad = value, tangent, grad

    def _struct(self):
        t = self.tangent
        return _capi.LgarState(*[t[nm].data_ptr() for nm in _VALUE_FIELDS[:5]], None, None, t["scalars"].data_ptr(), None, None)


class LgarEngine:
    """N independent soil columns advanced by the gfx950 kernels.

    Parameters are [L] (shared by all columns) or [L, N] tensors/sequences; forcing is [T, N] (cm/h).  The other arguments
    are keywords (SETTINGS has the defaults):
    search_mode: 1 (default) = bracketed-Newton psi search + closed-form jumps in the depth search (same roots, same
    tolerances); 0 = verification mode: the reference's literal fixed-step line searches (Layer.py:275-317, 681-701),
    its update_psi pass and, in fp64, its trapezoid operation by operation; 2 = like 1 with the front-capacity chain
    (8 -> 16 -> 32 slots, include/lgar.h) forced even for small jobs (tests).
    front_slots: rows of the per-front state arrays = the most fronts a column can hold (<= 32; the reference's lists are
    unbounded, Layer.py:1336-1416).
    geff_precision: "native" (default) = the Geff trapezoid (lgar/green_ampt.py:45-84) in `dtype`; "f32" (fp64 fast modes
    only) = mixed precision: fp64 column state, branches, mass bookkeeping, trapezoid heads and end nodes; the 119 interior
    nodes with the fp32 hardware transcendentals, summed in fp64 (LgarDims.geff_mode = 1; DESIGN.md section 4 states the
    tolerance this reaches against the reference).
    forward_lanes: lanes per column in lgar_forward.  0 (default) = the library gives fp64 trapezoid jobs under one wave per
    SIMD 4..64 cooperating lanes per column (same results bit for bit); 1 = never; 4..64 = exactly that many (a group needs
    four lanes for the trapezoid's end points, so 2 and 3 do not exist).  Honoured by the fp64 fast modes (native or
    mixed-precision trapezoid) with nint <= 128 only; an explicit request that cannot be honoured raises.
    basin_scratch_bytes: most series memory the engine may allocate on its own behind basin sums whose series the caller
    did not ask for (see forward); 0 = never, such sums are taken by the in-kernel atomics instead.
    bottom_mode: 0 (default) = like the reference, a front reaching the domain bottom faults the column; 1 = it leaves
    the column as percolation (LGAR-C intent; parity unpinned, the reference crashes there).
    with_state=False: a tangent-only engine (autograd.parameter_vjp): the tangent kernels keep no state in HBM.

    What is about the library behind the calling surface sits in _open, _call, step_rows_host and cooperating_lanes; the
    test suite's device-code simulator replaces those and runs everything else of this class on the CPU.
    """

    _new_series = staticmethod(torch.empty)  # (rows of a column that faulted before them are never written)

    def __init__(self, alpha, n, ksat, theta_e, theta_r, thickness, *, n_columns=None, with_state=True, **settings):
        unknown = sorted(set(settings) - set(SETTINGS))
        if unknown:
            raise TypeError("LgarEngine got unexpected keyword arguments %s" % ", ".join(unknown))
        s = self.settings = dict(SETTINGS, **settings)
        L = len(alpha)
        if not LMIN <= L <= LMAX:
            raise LgarError("this build supports %d..%d soil layers (got %d)" % (LMIN, LMAX, L))
        self.lib, self.device = self._open(L, s["device"])
        dtype = self.dtype = s["dtype"]
        self._dt = _capi.dtype_code(dtype, _DTYPES)

        def prep(x):
            t = torch.as_tensor(x, dtype=torch.float64)
            if t.dim() == 1:
                if n_columns is None:
                    raise LgarError("n_columns is required when parameters are per-layer vectors")
                t = t[:, None].expand(-1, n_columns)
            return t.to(self.device, dtype).contiguous()

        self.alpha, self.n, self.ksat = prep(alpha), prep(n), prep(ksat)
        self.theta_e, self.theta_r, self.thickness = prep(theta_e), prep(theta_r), prep(thickness)
        N = self.alpha.shape[1]
        for t in (self.n, self.ksat, self.theta_e, self.theta_r, self.thickness):
            if tuple(t.shape) != (L, N):
                raise LgarError("parameter shapes differ: expected %s, got %s" % ((L, N), tuple(t.shape)))
        if len(s["giuh_ordinates"]) > GMAX:
            raise LgarError("at most %d GIUH ordinates" % GMAX)
        # physical sanity of the soil table (the reference would run into NaNs / negative pow bases much later)
        bad = [nm for nm, ok in (("alpha > 0", self.alpha > 0), ("n > 1", self.n > 1), ("ksat > 0", self.ksat > 0),
                                 ("theta_e > theta_r", self.theta_e > self.theta_r), ("theta_r >= 0", self.theta_r >= 0),
                                 ("thickness > 0", self.thickness > 0)) if not bool(ok.all())]
        if bad:
            raise LgarError("invalid soil parameters: need " + ", ".join(bad))
        nint, search_mode = int(s["nint"]), int(s["search_mode"])
        if not (float(s["dt_h"]) > 0 and int(s["num_subcycles"]) >= 1 and nint >= 1 and float(s["initial_psi"]) > 0):
            raise LgarError("need dt_h > 0, num_subcycles >= 1, nint >= 1, initial_psi > 0")
        self.L, self.N = L, N
        geff_precision = s["geff_precision"]
        if geff_precision not in ("native", "f32"):
            raise LgarError("geff_precision must be 'native' or 'f32'")
        if geff_precision == "f32" and (dtype != torch.float64 or search_mode == 0):
            raise LgarError("geff_precision='f32' is the mixed mode of the fp64 fast searches (dtype float64, search_mode 1 or 2)")
        self.geff_precision = geff_precision
        forward_lanes = s["forward_lanes"] = int(s["forward_lanes"])
        if forward_lanes not in (0, 1) and not 4 <= forward_lanes <= 64:
            raise LgarError("forward_lanes must be 0 (library's choice), 1, or 4..64 (got %d)" % forward_lanes)
        if forward_lanes > 1 and (dtype != torch.float64 or search_mode == 0 or s["use_closed_form_G"] or nint > 128):
            raise LgarError("forward_lanes=%d cannot be honoured: cooperating lanes exist for the fp64 fast modes (native or "
                            "mixed-precision trapezoid; no closed-form G, nint <= 128) only" % forward_lanes)
        self.basin_scratch_bytes = int(s["basin_scratch_bytes"])
        FMAX = int(s["front_slots"]) if s["front_slots"] else _capi.FMAX
        if not L + 1 <= FMAX <= _capi.FMAX:
            raise LgarError("front_slots must be in %d..%d" % (L + 1, _capi.FMAX))
        self.front_slots = FMAX
        self.dims = _capi.make_dims(n_columns=N, n_layers=L, front_slots=FMAX, geff_mode=1 if geff_precision == "f32" else 0,
                                    **{k: s[k] for k in _DIMS_SETTINGS})

        self.status = torch.zeros(N, dtype=torch.int32, device=self.device)
        self._params = _capi.LgarParams(*[getattr(self, nm).data_ptr() for nm in PARAMS])
        self._state = None
        if not with_state:
            return
        z = lambda *shape, dt=dtype: torch.zeros(*shape, dtype=dt, device=self.device)
        self.depth, self.theta, self.psi = z(FMAX, N), z(FMAX, N), z(FMAX, N)
        self.k, self.dzdt = z(FMAX, N), z(FMAX, N)
        self.flags = z(FMAX, N, dt=torch.uint8)
        self.n_fronts = z(N, dt=torch.int32)
        self.scalars = z(NSCAL, N)
        self.totals = z(NACC, N)
        self.counters = z(_capi.NCOUNTERS, dt=torch.int64)
        self._basin_scratch = (0, {})  # series buffers behind basin sums whose series the caller did not ask for
        self.tickets = z(_capi.NTICKETS, dt=torch.int32)  # work counters of the persistent-wave schedule
        self._state = _capi.LgarState(*[t.data_ptr() for t in (self.depth, self.theta, self.psi, self.k, self.dzdt,
                                                               self.flags, self.n_fronts, self.scalars, self.totals,
                                                               self.tickets)])
        self.reset()

    def like(self, alpha, n, ksat, theta_e, theta_r, thickness, with_state=True, **changes):
        """An engine of this class with this one's settings (and `changes`) over other parameter arrays ([L, N]).
        with_state=False: the tangent-only sibling, which takes what the tangent kernels have -- the native trapezoid and no
        cooperating forward lanes."""
        # (ponded_depth_max as it stands now: the model updates it in dims)
        kw = dict(self.settings, device=self.device, ponded_depth_max=self.dims.ponded_depth_max, front_slots=self.front_slots)
        if not with_state:
            kw.update(geff_precision="native", forward_lanes=0)
        kw.update(changes)
        return type(self)(alpha, n, ksat, theta_e, theta_r, thickness, with_state=with_state, **kw)

    # the library behind the calling surface -----------------------------------------------------
    def _open(self, n_layers, device):
        """(library, torch.device) this engine runs on."""
        device = torch.device(device)
        return _capi.open_library(device, _NO_GPU), device

    def _call(self, name, *args, counters=None):
        """Entry point lgar_<name> on this engine's device and current stream: `args`, then the dtype code, the stream and, for
        the tangent, its work counters."""
        _capi.launch(self.lib, name, self.device, *args, self._dt, tail=() if counters is None else (counters.data_ptr(),))

    # ------------------------------------------------------------------------------------------
    def _need_state(self):
        if self._state is None:
            raise LgarError("this engine was created with with_state=False (tangent launches only)")

    def reset(self):
        """dpLGAR.set_internal_states() for every column."""
        self._call("state_init", C.byref(self.dims), C.byref(self._params), C.byref(self._state), self.status.data_ptr())

    def snapshot(self):
        """The column state as it stands now, as an EngineState (clones: later calls do not change it)."""
        self._need_state()
        return EngineState(**{nm: getattr(self, nm).clone() for nm in EngineState.FIELDS})

    def _check_state(self, snap, what, N=None):
        """`snap` is an EngineState for this engine's columns (or N of them), front slots, dtype and device."""
        N = self.N if N is None else N
        if not isinstance(snap, EngineState):
            raise LgarError("%s must be an EngineState (LgarEngine.snapshot()); got %s" % (what, type(snap).__name__))
        if snap.N != N:
            raise LgarError("%s holds %d columns, this engine has %d" % (what, snap.N, N))
        if snap.front_slots != self.front_slots:
            raise LgarError("%s has front_slots = %d, this engine %d" % (what, snap.front_slots, self.front_slots))
        if snap.dtype != self.dtype:
            raise LgarError("%s is %s, this engine %s" % (what, snap.dtype, self.dtype))
        if snap.device != self.status.device:
            raise LgarError("%s is on %s, this engine on %s" % (what, snap.device, self.status.device))

    def restore(self, snap):
        """Put an EngineState back (same N, front_slots, dtype and device, else LgarError).  The run totals stay as they are."""
        self._need_state()
        self._check_state(snap, "the snapshot")
        for nm in EngineState.FIELDS:
            getattr(self, nm).copy_(getattr(snap, nm))

    def release_scratch(self):
        """Free the series buffers forward() keeps behind basin sums (they come back on the next such call)."""
        self._basin_scratch = (0, {})

    def _forcing(self, precip, pet, forcing_group, forcing_map=None):
        """The forcing pair on the device in the engine's dtype ([T, Nf]; a 1-D pair is one row), checked, with LgarDims'
        per-call fields (n_steps and the forcing layout) set for it.  forcing_map: a forcing.ForcingMap -- the pair is then
        [T, B] for the map's B forcing columns and the map has one entry per group of forcing_group columns."""
        precip = torch.as_tensor(precip).to(self.device, self.dtype).contiguous()
        pet = torch.as_tensor(pet).to(self.device, self.dtype).contiguous()
        if precip.dim() == 1:
            precip, pet = precip[None, :], pet[None, :]
        g = max(1, int(forcing_group))
        if forcing_map is not None:
            fm = forcing_map
            index = getattr(fm, "index", None)
            if (not isinstance(index, torch.Tensor) or index.device != self.status.device or index.dtype != torch.int32
                    or index.dim() != 1 or not index.is_contiguous() or index.numel() != getattr(fm, "M", None)):
                raise LgarError("forcing_map must be a ForcingMap on %s (same device as the engine)" % (self.device,))
            if self.N % g != 0 or fm.M != self.N // g:
                raise LgarError("forcing_map has %d entries, this engine needs %d: one per group of forcing_group = %d of its "
                                "%d columns" % (fm.M, self.N // g if self.N % g == 0 else -1, g, self.N))
            if precip.shape != pet.shape or precip.dim() != 2 or precip.shape[1] != fm.B:
                raise LgarError("forcing must be [T, %d], one column per forcing column of the forcing_map; got %s / %s"
                                % (fm.B, tuple(precip.shape), tuple(pet.shape)))
        elif (precip.shape != pet.shape or precip.dim() != 2 or precip.shape[1] < 1 or self.N % g != 0
                or (self.N // g) % precip.shape[1] != 0):
            raise LgarError("forcing must be [T, %d] (or [T, Nf] with forcing_group * Nf dividing it: column c reads forcing "
                            "column (c // forcing_group) %% Nf); got %s / %s, forcing_group %d"
                            % (self.N, tuple(precip.shape), tuple(pet.shape), g))
        d = self.dims
        d.n_steps, d.forcing_columns, d.forcing_group = precip.shape[0], precip.shape[1], g
        return precip, pet

    def _step_out(self, series, basin=None, basin_names=(), weights=None, call_sums=None):
        """LgarStepOut over {name: [T, N] buffer} (+ the basin block with its names and weights, the call sums)."""
        so = _capi.LgarStepOut()
        for nm, buf in series.items():
            so.series[ACC_NAMES.index(nm)] = buf.data_ptr()
        so.basin, so.weights, so.call_sums = _ptr(basin), _ptr(weights), _ptr(call_sums)
        for nm in basin_names:
            so.basin_mask |= 1 << ACC_NAMES.index(nm)
        so.counters = self.counters.data_ptr()
        return so

    def _scratch_series(self, nm, T):
        """The [T, N] scratch series behind a sum over `nm` whose series the caller did not ask for (kept for the next call of
        the same T), or None when all such buffers together would pass basin_scratch_bytes."""
        if self._basin_scratch[0] != T:  # buffers of one call shape at a time
            self._basin_scratch = (T, {})
        scratch = self._basin_scratch[1].get(nm)
        one = T * self.N * self.totals.element_size()
        if scratch is None and (len(self._basin_scratch[1]) + 1) * one <= self.basin_scratch_bytes:
            scratch = self._basin_scratch[1][nm] = self._new_series(T, self.N, dtype=self.dtype, device=self.device)
        return scratch

    def forward(self, precip, pet, series=("runoff", "percolation"), out=None, check=True, basin=(), weights=None,
                call_sums=False, forcing_group=1, catchments=None, catchment=(), forcing_map=None, routing=None):
        """Advance every column by T forcing steps.  precip/pet: [T, N] cm/h on self.device, or [T, Nf] with Nf dividing N
        (broadcast: column c reads forcing column c % Nf; Nf = 1 is one basin series for every column); with forcing_group
        G > 1, G consecutive columns share a forcing column: column c reads (c // G) % Nf.
        forcing_map: a forcing.ForcingMap (CatchmentMap.forcing_map() makes one) -- precip/pet are then [T, B] for ANY B and
        column c reads forcing column forcing_map.index[c // G]: catchments of unequal size, each with its own series, and
        no gathered [T, N] forcing (LgarForcing.column_map, include/lgar.h).  The results are bit for bit those of the
        gathered forcing precip[:, index].

        Returns {name: tensor[T, N]} for the requested per-step series (the model accumulators as they
        stand after each forward(), before MassBalance.change_mass zeroes them).  basin: names whose per-step sum over
        this engine's columns (optionally weighted by weights[N]) is reduced on the device; returned under
        "basin:<name>" as fp64 [T] tensors.  MEMORY: a basin sum is taken from the stored series (one deterministic pass, ~10x
        cheaper than in-kernel atomics), so a basin name that is not also in `series` gets a [T, N] scratch series of its own,
        kept for the next call of the same T -- as long as all such buffers together stay within the engine's
        basin_scratch_bytes (default 8 GiB; 0 = never); past that the sum falls back to the in-kernel atomics and nothing is
        allocated.  release_scratch() frees them.  call_sums=True adds "call_sums": [NACC, N], the accumulators summed over this
        call's steps (rows 8, 9: latest ponded_water / ending_volume).
        catchments: a catchments.CatchmentMap over this engine's columns, catchment: names whose per-step sums over EACH
        catchment are wanted: returned under "catchment:<name>" as fp64 [T, B], with "catchment:weight" [B], the sums of the
        weights (the map's own; `weights` above belongs to the basin sums) of the columns that have not faulted.  They are
        taken from the stored series after the launch (lgar_catchment_sums, include/lgar.h: a fixed summation order per
        catchment, the same bits on every run) with the engine's status, so a faulted column drops out of every row.  A name
        that is not in `series` gets a scratch series by the rule above; past the budget this raises (there is no in-kernel
        catchment sum).
        routing: a catchments.CatchmentRouting over the map's B catchments: every name in `catchment` is also returned routed
        through it, "catchment:routed:<name>" (fp64 [T, B]), on the same stream, with the routing's queue of that name carried
        from call to call as the engine carries its state (lgar_catchment_route, include/lgar.h: at the row resolution of the
        stored series; routing.reset() goes with reset()).  routing needs catchments."""
        self._need_state()
        precip, pet = self._forcing(precip, pet, forcing_group, forcing_map)
        T = precip.shape[0]
        res = {}
        for nm in series:
            buf = out[nm] if out is not None and nm in out else self._new_series(T, self.N, dtype=self.dtype, device=self.device)
            if tuple(buf.shape) != (T, self.N) or buf.dtype != self.dtype or not buf.is_contiguous():
                raise LgarError("bad output buffer for series %r" % nm)
            res[nm] = buf
        stored, block, w = dict(res), None, None
        if basin:
            block = torch.zeros(NACC, T, dtype=torch.float64, device=self.device)
            for nm in basin:
                res["basin:" + nm] = block[ACC_NAMES.index(nm)]
                # a basin sum is taken from the stored series in one deterministic pass after the launch (include/lgar.h:
                # LgarStepOut.basin); the in-kernel atomics are ~10x as expensive, so a name whose series the caller does
                # not want still gets a scratch series (kept for the next call of the same shape) unless it would be huge
                if nm not in stored:
                    scratch = self._scratch_series(nm, T)
                    if scratch is not None:
                        stored[nm] = scratch
            if weights is not None:
                w = torch.as_tensor(weights).to(self.device, self.dtype).contiguous()
                if tuple(w.shape) != (self.N,):
                    raise LgarError("weights must be [N]")
        if catchments is not None:
            if getattr(catchments, "N", None) != self.N or catchments.ids.device != self.status.device:
                raise LgarError("catchments must be a CatchmentMap over this engine's %d columns on %s" % (self.N, self.device))
            for nm in catchment:
                if nm not in ACC_NAMES:
                    raise LgarError("unknown catchment sum %r (one of %s)" % (nm, ", ".join(ACC_NAMES)))
                if nm not in stored:
                    stored[nm] = self._scratch_series(nm, T)
                    if stored[nm] is None:
                        raise LgarError("the catchment sum of %r needs a [%d, %d] series and basin_scratch_bytes = %d does not "
                                        "allow it: ask for the series (series=...) or raise the budget"
                                        % (nm, T, self.N, self.basin_scratch_bytes))
        elif catchment:
            raise LgarError("catchment=%r needs catchments=<CatchmentMap>" % (tuple(catchment),))
        if routing is not None:
            if catchments is None:
                raise LgarError("routing needs catchments=<CatchmentMap>: it routes the [T, B] catchment sums")
            if getattr(routing, "B", None) not in (None, catchments.B) or routing.ordinates.device != self.status.device:
                raise LgarError("routing must be a CatchmentRouting over the map's %d catchments on %s" % (catchments.B, self.device))
        if call_sums:
            res["call_sums"] = torch.zeros(NACC, self.N, dtype=self.dtype, device=self.device)
        so = self._step_out(stored, block, basin, w, res.get("call_sums"))
        fo = _capi.LgarForcing(precip.data_ptr(), pet.data_ptr(), None if forcing_map is None else forcing_map.index.data_ptr())
        self._call("forward", C.byref(self.dims), C.byref(self._params), C.byref(self._state), C.byref(fo), C.byref(so),
                   self.status.data_ptr())
        if catchments is not None:
            # from the stored series, after the launch on the same stream, with the status the launch left: a column that
            # faulted drops out of every row (the rows after its fault were never written)
            for nm in catchment:
                res["catchment:" + nm] = catchments.sums(stored[nm], status=self.status)
            no_rows = torch.empty(0, self.N, dtype=self.dtype, device=self.device)
            res["catchment:weight"] = catchments.sums(no_rows, status=self.status, weight_sums=True)[1]
            if routing is not None:
                for nm in catchment:
                    res["catchment:routed:" + nm] = routing.route(res["catchment:" + nm], carry=True, key=nm)
        if check:
            self.check_status()
        return res

    def step_rows_host(self, precip_row, pet_row):
        """The drop-in's calling convention -- ONE forcing row per call, results wanted on the host (the reference keeps its
        accumulators in host tensors and reads them after every forward(), physics/MassBalance.py:31-53) -- with the host-side
        cost of a call cut to the bone: persistent pinned staging buffers, argument structs built once, one upload, the kernel
        launches of lgar_forward, two downloads and ONE stream synchronisation; no allocation, no other torch op.

        precip_row / pet_row: length-N sequences or tensors (cm/h).  Returns (call_sums [NACC, N], runoff [N], percolation [N],
        status [N]) as views of the pinned host buffers, valid until the next call."""
        self._need_state()
        st = getattr(self, "_row_stepper", None)
        if st is None:
            N, dev = self.N, self.device
            st = self._row_stepper = {}
            st["h_in"] = torch.zeros(2, 1, N, dtype=self.dtype).pin_memory()
            st["d_in"] = torch.zeros(2, 1, N, dtype=self.dtype, device=dev)
            st["d_out"] = torch.zeros(NACC + 2, N, dtype=self.dtype, device=dev)  # call_sums rows, then runoff, percolation
            st["h_out"] = torch.zeros(NACC + 2, N, dtype=self.dtype).pin_memory()
            st["h_status"] = torch.zeros(N, dtype=torch.int32).pin_memory()
            so = self._step_out({"runoff": st["d_out"][NACC], "percolation": st["d_out"][NACC + 1]}, call_sums=st["d_out"])
            fo = _capi.LgarForcing(st["d_in"][0].data_ptr(), st["d_in"][1].data_ptr())
            st["structs"] = (so, fo)  # (byref keeps no reference of its own)
            st["args"] = (C.byref(self.dims), C.byref(self._params), C.byref(self._state), C.byref(fo), C.byref(so),
                          self.status.data_ptr())
        h_in = st["h_in"]
        h_in[0, 0] = torch.as_tensor(precip_row, dtype=self.dtype)
        h_in[1, 0] = torch.as_tensor(pet_row, dtype=self.dtype)
        d = self.dims
        d.n_steps, d.forcing_columns, d.forcing_group = 1, self.N, 1
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            st["d_in"].copy_(h_in, non_blocking=True)
            # (the library itself, not _call: entering the device context a second time costs 2 of a call's 115 us)
            _capi.check(self.lib.lgar_forward(*st["args"], self._dt, C.c_void_p(stream.cuda_stream)), "lgar_forward")
            st["h_out"].copy_(st["d_out"], non_blocking=True)
            st["h_status"].copy_(self.status, non_blocking=True)
            stream.synchronize()
        return st["h_out"][:NACC], st["h_out"][NACC], st["h_out"][NACC + 1], st["h_status"]

    def raise_for_status(self, status_host):
        """check_status() on a host copy of the status words (no device round trip)."""
        if bool((status_host != 0).any()):
            self.check_status()

    def _tangent_inputs(self, direction, precip, pet, w_runoff, w_perc, forcing_group, share, forcing_map):
        """What tangent() and tangent_window() take alike, on the device and checked (LgarDims' per-call fields set):
        (precip, pet, w_runoff, w_perc, {kind: direction [L, N] or None})."""
        prep = lambda t: None if t is None else torch.as_tensor(t).to(self.device, self.dtype).contiguous()
        precip, pet = self._forcing(precip, pet, forcing_group, forcing_map)
        w_runoff, w_perc = prep(w_runoff), prep(w_perc)
        share = int(share)
        if share != 0 and (not 2 <= share <= 32 or self.N % share != 0):
            raise LgarError("share must be 0 or 2..32 (with n_columns a multiple of it)")
        if share:
            # the kernel takes the caller's word that each group of `share` columns is one soil column; a violation would
            # give silently wrong gradients, so the wrapper checks (six small reductions)
            for t in (self.alpha, self.n, self.ksat, self.theta_e, self.theta_r, self.thickness):
                gw = t.reshape(t.shape[0], -1, share)
                if not bool((gw == gw[:, :, :1]).all()):
                    raise LgarError("share=%d needs identical soil parameters within each group of %d columns" % (share, share))
            if forcing_group % share != 0 and precip.shape[1] != 1:
                raise LgarError("share=%d needs the columns of a group to read the same forcing column (forcing_group a "
                                "multiple of it, or one forcing column for all)" % share)
        self.dims.tangent_share = int(share)
        for nm, w in (("w_runoff", w_runoff), ("w_perc", w_perc)):
            if forcing_map is not None:
                if w is not None and tuple(w.shape) != (precip.shape[0], forcing_map.M):
                    raise LgarError("%s must be [T, %d], one column per entry of the forcing_map; got %s"
                                    % (nm, forcing_map.M, tuple(w.shape)))
            elif w is not None and w.shape != precip.shape:
                raise LgarError("%s must be [T, N] like the forcing; got %s" % (nm, tuple(w.shape)))
        dirs = {k: prep(direction.get(k)) for k in ("alpha", "n", "ksat")}
        for k, v in dirs.items():
            if v is not None and tuple(v.shape) != (self.L, self.N):
                raise LgarError("direction[%r] must be [L, N]" % k)
        return precip, pet, w_runoff, w_perc, dirs

    def _forcing_direction(self, d_precip, d_pet, precip):
        """The forcing tangents of tangent() / tangent_window() on the device in the engine's dtype and checked against the forcing
        `precip` that _forcing returned: [T, Nf, G] each (G = forcing_group; [T, Nf] will do when G = 1), or None.  Returns the
        LgarForcing block that holds them and the tensors it points into."""
        T, Nf, g = precip.shape[0], precip.shape[1], self.dims.forcing_group
        keep = []
        for nm, d in (("d_precip", d_precip), ("d_pet", d_pet)):
            if d is not None:
                d = torch.as_tensor(d).to(self.device, self.dtype).contiguous()
                if tuple(d.shape) != (T, Nf, g) and not (g == 1 and tuple(d.shape) == (T, Nf)):
                    raise LgarError("%s must be [T, Nf, forcing_group] = [%d, %d, %d]: one tangent per lane of a direction group of "
                                    "each forcing column; got %s" % (nm, T, Nf, g, tuple(d.shape)))
            keep.append(d)
        return _capi.LgarForcing(_ptr(keep[0]), _ptr(keep[1]), None), keep

    def _tangent_call(self, name, inputs, forcing_map, want_series, window=(), grad=None, st=None, d_forcing=None):
        """What tangent() and tangent_window() do alike with _tangent_inputs' results: lgar_<name> with the direction and forcing
        blocks, `window` (the arguments between the weights and grad) and fresh work counters.  d_forcing = (d_precip, d_pet):
        the call goes to lgar_forward_tangent_forced, with the block of the forcing's tangents behind the forcing.  Returns
        (grad, series, st)."""
        precip, pet, w_runoff, w_perc, dirs = inputs
        dstruct = _capi.LgarParams(_ptr(dirs["alpha"]), _ptr(dirs["n"]), _ptr(dirs["ksat"]), None, None, None)
        grad = torch.zeros(self.N, dtype=self.dtype, device=self.device) if grad is None else grad
        ser = self._new_series(precip.shape[0], self.N, dtype=self.dtype, device=self.device) if want_series else None
        st = torch.zeros(self.N, dtype=torch.int32, device=self.device) if st is None else st
        tickets = torch.zeros(_capi.NTICKETS, dtype=torch.int32, device=self.device)  # persistent-wave work counters
        self._last_tickets = tickets  # (for the tests: entries 4, 5 count the columns kernels 0, 1 of the chain handed over)
        fo = _capi.LgarForcing(precip.data_ptr(), pet.data_ptr(), None if forcing_map is None else forcing_map.index.data_ptr())
        forced = ()
        if d_forcing is not None:
            dfo, keep = self._forcing_direction(*d_forcing, precip)
            name, forced = "forward_tangent_forced", (C.byref(dfo),)
        self._call(name, C.byref(self.dims), C.byref(self._params), C.byref(dstruct), C.byref(fo), *forced, _ptr(w_runoff),
                   _ptr(w_perc), *window, grad.data_ptr(), _ptr(ser), st.data_ptr(), counters=tickets)
        return grad, ser, st

    def tangent(self, direction, precip, pet, w_runoff=None, w_perc=None, want_series=False, forcing_group=1, share=0,
                forcing_map=None, d_precip=None, d_pet=None):
        """Forward-mode tangent from a FRESH state (set_internal_states) over the whole forcing series.

        direction: {"alpha" | "n" | "ksat": [L, N] tensor} -- the parameter perturbation (missing = 0).
        precip / pet / w_runoff / w_perc: [T, N], or all [T, Nf] with forcing_group * Nf dividing N (column c uses column
        (c // forcing_group) % Nf of each).
        forcing_map: a forcing.ForcingMap -- precip / pet are [T, B] and column c reads forcing column
        forcing_map.index[c // forcing_group]; the weights are then [T, N // forcing_group] and column c reads weight column
        c // forcing_group (they do not go through the map: the gradient of a catchment sum carries every column's own weight).
        share = W (2..32): each group of W consecutive columns is ONE soil column along W directions; the W lanes share the
        Geff trapezoid (LgarDims.tangent_share).
        Returns (grad[N], tangent_runoff[T, N] or None, status[N]) with
        grad[c] = sum_t w_runoff[t, c] * d runoff_t[c] + w_perc[t, c] * d percolation_t[c].  status != 0 marks columns whose
        tangent integration faulted (their grad entry is not a gradient): callers must check it (autograd.parameter_vjp does).
        d_precip / d_pet: the direction's part in the FORCING, [T, Nf, forcing_group] each (or None = 0; [T, Nf] when
        forcing_group is 1): column c runs on (precip, d_precip[t, cf, c % forcing_group]), cf its forcing column, so every
        lane of a direction group has its own forcing tangent and those that carry a parameter direction hold zeros
        (lgar_forward_tangent_forced).  The derivative is then along `direction` and the forcing direction together."""
        if d_precip is not None or d_pet is not None:
            return self.tangent_window(direction, precip, pet, w_runoff, w_perc, None, False, want_series, forcing_group, share,
                                       forcing_map, d_precip, d_pet)[:3]
        inputs = self._tangent_inputs(direction, precip, pet, w_runoff, w_perc, forcing_group, share, forcing_map)
        return self._tangent_call("forward_tangent", inputs, forcing_map, want_series)

    def tangent_window(self, direction, precip, pet, w_runoff=None, w_perc=None, start=None, keep_state=True, want_series=False,
                       forcing_group=1, share=0, forcing_map=None, d_precip=None, d_pet=None):
        """tangent() over a WINDOW of rows that may start from a carried state (lgar_forward_tangent_window, include/lgar.h).

        start: None = a fresh state: tangent() itself, bit for bit.  An EngineState (snapshot() of a spun-up engine) = a
        stop-gradient start: the result is the exact derivative, with respect to the parameters, of "forward() from this fixed
        state over these rows"; nothing flows into the run that produced the state.  The TangentState a previous call returned
        as `end` = carry: value state, tangent state and the gradient so far go on, and a run cut into windows leaves the bits
        of one call (the direction must be the same one).
        keep_state=False: no end state is stored (the last window of a backward pass).
        Returns (grad[N], tangent_runoff[T, N] or None, status[N], end): `end` is a TangentState or None.  Columns whose start
        state had faulted keep those fault bits in status.  This engine's own state is neither read nor written; an engine
        made with with_state=False will do.  The other arguments are tangent()'s; with share = W the W columns of a group
        must hold the same start values as well.  d_precip / d_pet are this window's rows of the forcing's tangents; when either
        is given the call is lgar_forward_tangent_forced, and a TangentState carries across such windows as across any."""
        inputs = self._tangent_inputs(direction, precip, pet, w_runoff, w_perc, forcing_group, share, forcing_map)
        N = self.N
        value = start.value if isinstance(start, TangentState) else start
        if value is not None:
            self._check_state(value, "start")
            for nm in EngineState.FIELDS[:8] if share else ():
                t = getattr(value, nm)
                gw = t.reshape(t.shape[:-1] + (-1, int(share)))
                if not bool((gw == gw[..., :1]).all()):
                    raise LgarError("share=%d needs identical start values within each group of %d columns" % (share, share))
        carried = start if isinstance(start, TangentState) else None
        if carried is not None and (tuple(carried.grad.shape) != (N,) or carried.grad.dtype != self.dtype
                                    or carried.grad.device != self.status.device):
            raise LgarError("start carries a gradient of %s %s, this engine needs [%d] %s" % (tuple(carried.grad.shape), carried.grad.dtype, N, self.dtype))
        z = lambda *shape, dt=self.dtype: torch.zeros(*shape, dtype=dt, device=self.device)
        end = None
        if keep_state:
            F = self.front_slots
            # (zeros: rows at and beyond a column's n_fronts are never written, and whole states are compared bit for bit)
            end = TangentState(EngineState(depth=z(F, N), theta=z(F, N), psi=z(F, N), k=z(F, N), dzdt=z(F, N), flags=z(F, N, dt=torch.uint8),
                                           n_fronts=z(N, dt=torch.int32), scalars=z(NSCAL, N), status=z(N, dt=torch.int32)),
                               {nm: z(NSCAL if nm == "scalars" else F, N) for nm in _VALUE_FIELDS}, z(N))
        structs = [None if value is None else value._struct(), None if carried is None else carried._struct(),
                   None if end is None else end.value._struct(), None if end is None else end._struct()]
        win = _capi.LgarTangentWindow(*[None if s is None else C.addressof(s) for s in structs], None if carried is None else carried.grad.data_ptr())
        grad, ser, st = self._tangent_call("forward_tangent_window", inputs, forcing_map, want_series, (C.byref(win),),
                                           *(() if end is None else (end.grad, end.value.status)),
                                           d_forcing=None if d_precip is None and d_pet is None else (d_precip, d_pet))
        if value is not None:
            st |= value.status & _capi.ST_FAULT_MASK  # (the kernels write the status, they do not read it)
        return grad, ser, st, end

    def cooperating_lanes(self):
        """Lanes per column lgar_forward uses for this engine's job (1, or 4..64 for fp64 jobs under one wave per SIMD)."""
        return int(self.lib.lgar_cooperating_lanes(C.byref(self.dims), self._dt))

    def geff_wave_calls(self, reset=True):
        """Wave-level Geff evaluations since the last reset (measurement: LgarStepOut.counters[0])."""
        n = int(self.counters[0].item())
        if reset:
            self.counters.zero_()
        return n

    def check_status(self):
        """Raise like the reference does (ValueError) if any column hit a physics fault."""
        st = self.status
        if not bool((st != 0).any()):
            return
        bad = torch.nonzero(st)[:, 0]
        kinds = torch.tensor(list(_capi.STATUS_NAMES), dtype=st.dtype, device=st.device)
        present = ((st[bad, None] & kinds) != 0).any(0).tolist()  # the fault bits set in any column
        names = [nm for nm, there in zip(_capi.STATUS_NAMES.values(), present) if there]
        raise LgarStatusError("%d of %d columns faulted (%s); first column %d, max status %d"
                              % (bad.numel(), self.N, ", ".join(names), int(bad[0].item()), int(st.max().item())))

    # ------------------------------------------------------------------------------------------
    def fronts(self):
        """Front tables as host numpy arrays: depth/theta/psi/k/dzdt [front_slots, N], layer, to_bottom, n_fronts (rows at and
        beyond a column's n_fronts are not meaningful)."""
        fl = self.flags.cpu().numpy()
        return dict(depth=self.depth.cpu().numpy(), theta=self.theta.cpu().numpy(), psi=self.psi.cpu().numpy(),
                    k=self.k.cpu().numpy(), dzdt=self.dzdt.cpu().numpy(), layer=(fl & 0x7F).astype("int8"),
                    to_bottom=(fl >> 7).astype("int8"), n_fronts=self.n_fronts.cpu().numpy())

    # ------------------------------------------------------------------------------------------
    def _moisture_bins(self, edges, what, need_state=True):
        """Host-side checks of soil_moisture's bins (the library never reads device memory on the host, so the C-ABI takes the
        caller's word for the edges): returns (device fp64 edges or None, number of bins).  need_state=False: the bins are for
        a state that is not this engine's own (soil_moisture_tangent)."""
        if need_state:
            self._need_state()
        if what not in _capi.MOIST_WHAT:
            raise LgarError("what must be 'theta' or 'storage' (got %r)" % (what,))
        if edges is None:
            return None, self.L
        try:
            e = torch.as_tensor(edges).detach().to("cpu", torch.float64)
        except (TypeError, ValueError, RuntimeError) as err:
            raise LgarError("edges must be a 1-D sequence of depths in cm (%s)" % err)
        if e.dim() != 1 or e.numel() < 2:
            raise LgarError("edges must be 1-D with at least two entries (got shape %s)" % (tuple(e.shape),))
        if e.numel() - 1 > _capi.MOIST_BINS:
            raise LgarError("at most %d bins (LGAR_MOIST_BINS); got %d" % (_capi.MOIST_BINS, e.numel() - 1))
        if not bool(torch.isfinite(e).all()) or float(e[0]) < 0.0 or not bool((e[1:] > e[:-1]).all()):
            raise LgarError("edges must be finite, >= 0 and strictly increasing")
        return e.to(self.device).contiguous(), e.numel() - 1

    def _moisture_launch(self, e_dev, n_bins, what, out, w, sums):
        self._call("soil_moisture", C.byref(self.dims), C.byref(self._params), C.byref(self._state), _ptr(e_dev), n_bins,
                   _capi.MOIST_WHAT[what], out.data_ptr(), _ptr(w), _ptr(sums))

    def _moisture_weights(self, weights):
        if weights is None:
            return None
        w = torch.as_tensor(weights).to(self.device, self.dtype).contiguous()
        if tuple(w.shape) != (self.N,):
            raise LgarError("weights must be [N]")
        return w

    def soil_moisture(self, edges=None, what="theta", out=None, weights=None, basin=False):
        """Depth-binned water content of every column as the front table stands now (lgar_soil_moisture, include/lgar.h;
        DESIGN.md section 9 has the definition): computed on the device from the stored state, nothing is copied to the host.

        edges: [D + 1] depths in cm (finite, >= 0, strictly increasing, D <= 32) -> [D, N]; None = each column's own soil
        layers -> [L, N].  what: "theta" = mean volumetric water content of the bin over its in-column width (NaN for a bin
        wholly below the column), "storage" = cm of water in the bin.  The arithmetic is fp64 whatever the engine's dtype; the
        result is rounded once to it.  out: optional [D, N] buffer (engine dtype and device, contiguous).
        basin: True -> also returns the fp64 [D] sums over the columns, sum_c weights[c] * result[:, c] (weights [N], default 1),
        in a fixed order (the same bits on every run); an fp64 [D] device tensor -> the sums are ADDED to it (like
        LgarStepOut.basin) and it is returned.  Columns with a non-zero status hold leftover state: their entries are not
        meaningful (never out of bounds)."""
        e_dev, D = self._moisture_bins(edges, what)
        if out is None:
            out = torch.empty(D, self.N, dtype=self.dtype, device=self.device)
        elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != (D, self.N) or out.dtype != self.dtype
              or out.device != self.totals.device or not out.is_contiguous()):
            raise LgarError("out must be a contiguous [%d, %d] %s tensor on %s" % (D, self.N, self.dtype, self.device))
        w = self._moisture_weights(weights)
        sums = None
        if basin is True:
            sums = torch.zeros(D, dtype=torch.float64, device=self.device)
        elif basin is not False and basin is not None:
            sums = basin
            if (not isinstance(sums, torch.Tensor) or tuple(sums.shape) != (D,) or sums.dtype != torch.float64
                    or sums.device != self.totals.device or not sums.is_contiguous()):
                raise LgarError("basin must be True or a contiguous fp64 [%d] tensor on %s" % (D, self.device))
        elif w is not None:
            raise LgarError("weights are used by the basin sums only: pass basin=True")
        self._moisture_launch(e_dev, D, what, out, w, sums)
        return out if sums is None else (out, sums)

    def _moisture_tangent_launch(self, tstate, e_dev, n_bins, what, out, cot, group):
        """lgar_soil_moisture_tangent over a checked TangentState and checked bins: `out`, or `cot` into tstate.grad."""
        vs, ts = tstate.value._struct(), tstate._struct()
        self._call("soil_moisture_tangent", C.byref(self.dims), C.byref(self._params), C.byref(vs), C.byref(ts), _ptr(e_dev), n_bins,
                   _capi.MOIST_WHAT[what], _ptr(out), _ptr(cot), int(group), None if cot is None else tstate.grad.data_ptr())

    def soil_moisture_tangent(self, tstate, edges=None, what="theta", cot=None, group=1):
        """The tangent of soil_moisture() along the direction a TangentState was integrated for (lgar_soil_moisture_tangent,
        include/lgar.h): a pure function of the state `tangent_window` handed back as `end`, computed on
        the device.  The engine is the one whose tangent_window made the state: its N columns are the state's M lanes.

        edges, what: soil_moisture()'s; the tangent of a bin wholly below the column is 0 (its value is NaN).
        cot=None: returns the [D, M] tangent in the engine's dtype (fp64 arithmetic, rounded once).
        cot: a contiguous fp64 [D, M // group] cotangent on the device -- lane c reads column c // group, the forcing_group
        convention of the tangent launches.  The contraction sum_i cot[i] * tangent[i] (unrounded fp64 tangents, i ascending, bins
        below the column skipped whatever their cotangent holds) is ADDED to tstate.grad in place, no [D, M] array is allocated,
        and tstate is returned: the next window of the same direction carries the sum on."""
        e_dev, D = self._moisture_bins(edges, what, need_state=False)
        if not isinstance(tstate, TangentState):
            raise LgarError("tstate must be a TangentState (the `end` of LgarEngine.tangent_window); got %s" % type(tstate).__name__)
        self._check_state(tstate.value, "tstate")
        for nm in ("depth", "theta"):
            t = tstate.tangent.get(nm)
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != (self.front_slots, self.N) or t.dtype != self.dtype
                    or t.device != self.status.device or not t.is_contiguous()):
                raise LgarError("tstate.tangent[%r] must be a contiguous [%d, %d] %s tensor on %s" % (nm, self.front_slots, self.N, self.dtype, self.device))
        group = int(group)
        if group < 1 or self.N % group != 0:
            raise LgarError("group must be >= 1 and divide the %d lanes of the state (got %d)" % (self.N, group))
        if cot is None:
            out = torch.empty(D, self.N, dtype=self.dtype, device=self.device)
            self._moisture_tangent_launch(tstate, e_dev, D, what, out, None, group)
            return out
        if (not isinstance(cot, torch.Tensor) or tuple(cot.shape) != (D, self.N // group) or cot.dtype != torch.float64
                or cot.device != self.status.device or not cot.is_contiguous()):
            raise LgarError("cot must be a contiguous fp64 [%d, %d] tensor on %s" % (D, self.N // group, self.device))
        g = tstate.grad
        if tuple(g.shape) != (self.N,) or g.dtype != self.dtype or g.device != self.status.device or not g.is_contiguous():
            raise LgarError("tstate carries a gradient of %s %s, this engine needs [%d] %s" % (tuple(g.shape), g.dtype, self.N, self.dtype))
        self._moisture_tangent_launch(tstate, e_dev, D, what, None, cot, group)
        return tstate

    def run_with_soil_moisture(self, precip, pet, every, edges=None, what="theta", series=("runoff", "percolation"), basin=(),
                               weights=None, check=True, forcing_group=1, forcing_map=None):
        """forward() over the whole forcing with a soil-moisture snapshot after every `every` rows: the run is cut into windows
        of `every` rows, each advanced by forward() on the row slice (series written straight into [T, N] buffers, basin rows
        concatenated), and soil_moisture(edges, what) is taken after each full window.  Returns what forward() returns plus
        "soil_moisture": [T // every, D, N]; row r is the state after step (r + 1) * every - 1.  Rows beyond the last full
        window are still integrated.  Series, basin sums, the state and the status are those of ONE forward() over the same
        forcing bit for bit.  So are the run totals: forward() adds a call's own sum to them, which over several windows is
        another summation order, so the windows also store the accumulators that feed the totals (scratch series of `every`
        rows for those the caller did not ask for) and lgar_totals_replay adds them up in the one-call order (include/lgar.h;
        exact for every column that stays in one kernel of the front-capacity chain).  forcing_map: as in forward()."""
        every = int(every)
        if every < 1:
            raise LgarError("every must be >= 1")
        e_dev, D = self._moisture_bins(edges, what)
        precip, pet = self._forcing(precip, pet, forcing_group, forcing_map)
        T = precip.shape[0]
        series = tuple(series)
        # (zeros: a row no kernel writes -- a column that had faulted before the window -- must read zero in the replay)
        res = {nm: torch.zeros(T, self.N, dtype=self.dtype, device=self.device) for nm in series}
        # the accumulators forward() sums into the totals (lgar_forward_body.hpp: percolation only with a percolating bottom)
        summed = [nm for j, nm in enumerate(ACC_NAMES[:7]) if not (j == 5 and self.dims.bottom_mode == 0)]
        scratch = {nm: torch.zeros(min(every, T), self.N, dtype=self.dtype, device=self.device) for nm in summed if nm not in res}
        before = self.totals[:8].clone()
        running = torch.zeros(8, self.N, dtype=self.dtype, device=self.device)
        snaps = torch.empty(T // every, D, self.N, dtype=self.dtype, device=self.device)
        rows = {nm: [] for nm in basin}
        for lo in range(0, T, every):
            hi = min(lo + every, T)
            if lo:
                for buf in scratch.values():
                    buf.zero_()
            out = {nm: res[nm][lo:hi] for nm in series}
            out.update({nm: buf[:hi - lo] for nm, buf in scratch.items()})
            o = self.forward(precip[lo:hi], pet[lo:hi], series=series + tuple(scratch), out=out, check=False, basin=basin,
                             weights=weights, forcing_group=forcing_group, forcing_map=forcing_map)
            for nm in basin:
                rows[nm].append(o["basin:" + nm])
            stored = self._step_out({nm: out[nm] for nm in summed})
            self._call("totals_replay", C.byref(self.dims), C.byref(stored), hi - lo, running.data_ptr())
            if hi - lo == every:
                self._moisture_launch(e_dev, D, what, snaps[lo // every], None, None)
        if T:
            running[7] = running[6]  # discharge gains what giuh_runoff gains (models/dpLGAR.py:293-297)
            self.totals[:8] = before + running
        for nm in basin:
            res["basin:" + nm] = torch.cat(rows[nm]) if rows[nm] else torch.zeros(0, dtype=torch.float64, device=self.device)
        res["soil_moisture"] = snaps
        if check:
            self.check_status()
        return res

    def total(self, name):
        return self.totals[ACC_NAMES.index(name)]

    @property
    def ponded_water(self):
        return self.scalars[0]

    @property
    def previous_precip(self):
        return self.scalars[1]

    @property
    def ending_volume(self):
        return self.scalars[2]

    @property
    def giuh_runoff_queue(self):
        return self.scalars[3:3 + self.dims.n_giuh]


def leaf_batch(op, x, y=None, z=0.0, *, alpha, n, ksat, theta_e, theta_r, nint=120, wilting_point_psi=15495.0,
               dtype=torch.float64, device="cuda:0"):
    """Element-wise leaf kernels (known-answer tests): see lgar_leaf_batch in include/lgar.h."""
    dev = torch.device(device)
    lib = _capi.open_library(dev, _NO_GPU)
    ops = {"theta_from_h": 0, "se_from_h": 1, "k_from_se": 2, "h_from_se": 3, "geff": 4, "aet": 5, "geff_literal": 6,
           "log2": 7, "exp2": 8, "pow": 9, "geff_mixed": 10, "div": 11, "pow_pairwise": 12, "log2_pairwise": 13, "exp2_pairwise": 14,
           # float32 only: the fp32 fast mode's arithmetic (a * v_rcp_f32(b), v_sqrt_f32, v_log_f32 / v_exp_f32 pow)
           "div_rcp32": 15, "sqrt": 16, "theta_from_h_rcp32": 17, "se_from_h_rcp32": 18, "k_from_se_rcp32": 19,
           "h_from_se_rcp32": 20, "aet_rcp32": 21, "geff_from_heads": 22, "geff_closed": 23}
    prep = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float64).to(dev, dtype).contiguous()
    x, y, alpha, n, ksat, theta_e, theta_r = map(prep, (x, y, alpha, n, ksat, theta_e, theta_r))
    out = torch.empty_like(x)
    _capi.launch(lib, "leaf_batch", dev, ops[op], x.numel(), _ptr(x), _ptr(y), float(z), _ptr(alpha), _ptr(n), _ptr(ksat),
                 _ptr(theta_e), _ptr(theta_r), int(nint), float(wilting_point_psi), _ptr(out),
                 _capi.dtype_code(dtype, _DTYPES))
    return out


LEAF_TANGENT_OPS = {"theta_from_h": 0, "se_from_h": 1, "k_from_se": 2, "h_from_se": 3, "geff": 4, "aet": 5, "geff_literal": 6,
                    "lg2p": 7, "ex2p": 8, "pw": 9, "dv": 11, "sq": 16, "geff_closed": 23, "se_from_theta": 24, "pwx": 25,
                    "dv_dual_real": 26, "dv_real_dual": 27, "quotient": 28, "lg2": 29, "ex2": 30, "mn": 31, "ab": 32}
LEAF_SEEDS = ("alpha", "n", "ksat", "theta_e", "theta_r", "x", "y")


def leaf_tangent_batch(op, x, y=None, z=0.0, *, alpha, n, ksat, theta_e, theta_r, seeds=None, policy="lean", share=0, nint=120,
                       wilting_point_psi=15495.0, dtype=torch.float64, device="cuda:0"):
    """Element-wise tangent leaf kernels (known-answer tests): (value, tangent) of `op` along `seeds`, a dict of LEAF_SEEDS
    names -> [n] (a name left out is a seed of 0); with share = W, seeds and both results are [n, W].  See
    lgar_leaf_tangent_batch in include/lgar.h."""
    dev = torch.device(device)
    lib = _capi.open_library(dev, _NO_GPU)
    prep = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float64).to(dev, dtype).contiguous()
    x, y, alpha, n, ksat, theta_e, theta_r = map(prep, (x, y, alpha, n, ksat, theta_e, theta_r))
    seeds = dict(seeds or {})
    unknown = set(seeds) - set(LEAF_SEEDS)
    if unknown:
        raise ValueError("unknown seeds %s" % sorted(unknown))
    shape = (x.numel(), int(share)) if share else (x.numel(),)
    sd = [prep(seeds.get(k)) for k in LEAF_SEEDS]
    for s in sd:
        if s is not None and tuple(s.shape) != shape:
            raise ValueError("a seed has shape %s, not %s" % (tuple(s.shape), shape))
    value = torch.empty(shape, dtype=dtype, device=dev)
    tangent = torch.empty(shape, dtype=dtype, device=dev)
    _capi.launch(lib, "leaf_tangent_batch", dev, LEAF_TANGENT_OPS[op], {"lean": 0, "library": 1}[policy], int(share), x.numel(),
                 _ptr(x), _ptr(y), float(z), _ptr(alpha), _ptr(n), _ptr(ksat), _ptr(theta_e), _ptr(theta_r), *[_ptr(s) for s in sd],
                 int(nint), float(wilting_point_psi), _ptr(value), _ptr(tangent), _capi.dtype_code(dtype, _DTYPES))
    return value, tangent
