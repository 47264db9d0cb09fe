"""GPU (-m gpu): the dual-number arithmetic of the tangent kernels on the hardware, reached element-wise through
lgar_leaf_tangent_batch (include/lgar.h), against the exact derivative of the reference's discrete formulas
(tests/golden/leaf_tangent/leaf_tangent_ref.npz; tests/leaf_ref/tangent.py states it, tests/test_leaf_tangent_host.py asks the
same of the host build).  (a) values: lgar_leaf_batch's bit for bit, independent of the seeds; (b) double precision: every partial
and a mixed direction within MARGIN max(E_ref, 4 2^-53 A) (leaf_ref.check.tangent_tolerance); (c) single precision: classes, errors reported; (d) the SHARED
trapezoid (geff_shared_blocks_w, lgar_dual.hpp -- no host build reaches it) launched as the tangent kernels launch it, for ten
group widths W: values bit-identical to the unshared launch, tangents within (b)'s tolerance of the statement and within
1e-12 |D| + that tolerance of the unshared tangent, a group's value independent of what shares its wave, an item outside the
domain NaN in its own group only.

Reads only the committed fixture: no mpmath needed.  The measured figures are in DESIGN.md section 4."""
import numpy as np
import pytest

import leaf_ref as R
from leaf_ref import check
from leaf_ref import tangent as TG

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LEAF_NAMES = {0: "theta_from_h", 1: "se_from_h", 2: "k_from_se", 3: "h_from_se", 4: "geff", 5: "aet", 6: "geff_literal", 7: "log2", 8: "exp2",
              9: "pow", 11: "div", 16: "sqrt"}
LEAF_OP = dict(theta_from_h=0, se_from_h=1, k_from_se=2, h_from_se=3, aet=5, geff=4, geff_literal=6, lg2p=7, ex2p=8, pw=9, dv=11)
# (the fp32 trapezoid has no counterpart: the fp32 tangent kernels run the fused loop, the fp32 forward kernels the packed one)
LEAF_OP_F32 = dict(LEAF_OP, sq=16, geff=None)
WIDTHS = (2, 3, 5, 6, 8, 9, 12, 15, 18, 32)
NINT = check.NINT
SHARE_GROUPING = 1e-12  # what the comment on c0 / c1 in geff_shared_blocks_w claims for the grouping of the alpha direction


def _names():
    from lgar_py_amd.engine import LEAF_TANGENT_OPS
    return {v: k for k, v in LEAF_TANGENT_OPS.items()}


def gpu_tbatch(op, x, y=None, z=0.0, *, seeds=None, policy=check.LEAN, dtype=np.float64, share=0, **kw):
    import lgar_py_amd as lg
    v, t = lg.leaf_tangent_batch(_names()[op], x, y, z, seeds=seeds, policy="library" if policy == check.LIBRARY else "lean", share=share,
                                 dtype=torch.float64 if dtype == np.float64 else torch.float32, **kw)
    return v.cpu().numpy(), t.cpu().numpy()


def gpu_batch(op, x, y=None, z=0.0, *, dtype=np.float64, **kw):
    import lgar_py_amd as lg
    return lg.leaf_batch(LEAF_NAMES[op], x, y, z, dtype=torch.float64 if dtype == np.float64 else torch.float32, **kw).cpu().numpy()


@pytest.fixture(scope="module")
def fixture():
    return TG.load()


@pytest.mark.parametrize("fn", TG.FUNCTIONS)
def test_value_is_the_leaf_entrys_and_independent_of_the_seeds(fixture, fn):
    S, names, fns, _ = fixture
    for dtype, table in ((np.float64, LEAF_OP), (np.float32, LEAF_OP_F32)):
        check.tangent_values(fn, TG.OP_OF[fn], table.get(fn), gpu_tbatch, gpu_batch, S, fns[fn], dtype)


@pytest.mark.parametrize("fn", TG.FUNCTIONS)
def test_double_tangent_within_the_tolerance_of_the_statement(fixture, fn):
    """(b).  Measured, host build and MI355X: every op within 0.71 of the tolerance (geff d/dtheta_2, vg_table_17); 0.06 ... 0.50
    elsewhere.  The terms of leaf_ref.check.tangent_tolerance beyond MARGIN max(E_ref, floor) and what called for each are in
    DESIGN.md section 4 "Tangent leaves"."""
    S, names, fns, _ = fixture
    ref_stmt = fns["geff_literal"] if fn == "geff" else None  # (the reference computes the trapezoid WITH the nudge)
    for policy in ((check.LEAN, check.LIBRARY) if fn in TG.POLICY_LEAVES else (check.LEAN,)):
        check.tangent_against_fixture(fn, TG.OP_OF[fn], gpu_tbatch, S, fns[fn], names, policy, ref_stmt)


@pytest.mark.parametrize("fn", TG.FUNCTIONS)
def test_float_tangent_classes(fixture, fn):
    S, names, fns, _ = fixture
    check.tangent_f32(fn, TG.OP_OF[fn], gpu_tbatch, S, fns[fn], names, library_too=fn in TG.POLICY_LEAVES)


def test_aet_clamp_regimes(fixture):
    """The clamp of the AET below 0, above pet and at the exact tie: reached by the fixture, torch's derivative in the statement
    and in the reference, the kernel's exact in both precisions and both policies."""
    S, names, fns, _ = fixture
    check.aet_clamp_regimes(gpu_tbatch, S, fns["aet"])


def test_departures_from_torch():
    check.tangent_departures(gpu_tbatch)


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the shared trapezoid
# ---------------------------------------------------------------------------------------------------------------------------
def _heads(S, d, idx):
    """(h_i, h_f) of the trapezoids d[idx], as the kernel forms them (leaf op 3 on Se = (theta - theta_r) / (theta_e - theta_r))."""
    kw = check.soil_kw(S, d["soil"][idx])
    se = lambda th: (th - kw["theta_r"]) / (kw["theta_e"] - kw["theta_r"])
    h = lambda th: gpu_batch(3, se(th), nint=NINT, **kw)
    return h(d["x"][idx]), h(d["y"][idx])


def _safe_nodes(h_i, h_f):
    """geff_fused's count of leading nodes that lie a whole interval above the 0.1 cm cut, per item (lgar_geff.hpp)."""
    dh = (h_f - h_i) / NINT
    with np.errstate(divide="ignore", invalid="ignore"):
        jf = (h_i - 0.1) / -dh - 1.0
    return np.where(jf > 0.0, np.where(jf < NINT, np.floor(np.where(np.isfinite(jf), jf, 0.0)), NINT), 0).astype(int)


def _directions(W, n, rng):
    """[n, W, 7]: the unit seeds first (the first W of them for W < 7), then random directions."""
    sd = np.zeros((n, W, check.NSEED))
    for r in range(W):
        if r < check.NSEED:
            sd[:, r, r] = 1.0
        else:
            sd[:, r, :] = rng.uniform(-1.0, 1.0, (n, check.NSEED))
    return sd


def _shared(S, d, idx, W, sd):
    """(value, tangent) [n, W] of the trapezoids d[idx] through the shared launch along the directions sd [n, W, 7]."""
    seeds = {k: sd[:, :, j] for j, k in enumerate(check.SEED_NAMES)}
    return gpu_tbatch(4, d["x"][idx], d["y"][idx], seeds=seeds, share=W, nint=NINT, **check.soil_kw(S, d["soil"][idx]))


def _unshared(S, d, idx, W, sd):
    n = len(idx)
    rep = np.repeat(idx, W)
    seeds = {k: sd[:, :, j].reshape(-1) for j, k in enumerate(check.SEED_NAMES)}
    v, t = gpu_tbatch(4, d["x"][rep], d["y"][rep], seeds=seeds, nint=NINT, **check.soil_kw(S, d["soil"][rep]))
    return v.reshape(n, W), t.reshape(n, W)


@pytest.fixture(scope="module")
def trapezoids(fixture):
    """The fixture's trapezoids by what the wave-uniform safe-node count of a launch of their kind is: `dry` (both heads far above
    the cut: n_safe = nint), `wet` (up to theta_e: the last nodes fall under the cut), with each item's own count."""
    S, names, fns, _ = fixture
    d = fns["geff"]
    fin = np.isfinite(d["value"]) & np.isfinite(d["grad"]).all(axis=1) & (d["value"] > 0)
    h_i, h_f = _heads(S, d, np.arange(len(d["x"])))
    safe = _safe_nodes(h_i, h_f)
    dry = np.nonzero(fin & (safe == NINT))[0]
    wet = np.nonzero(fin & (safe < NINT))[0]
    assert len(dry) >= 200 and len(wet) >= 100
    return d, safe, dry, wet


@pytest.mark.parametrize("W", WIDTHS)
def test_shared_trapezoid(fixture, trapezoids, W):
    S, names, fns, _ = fixture
    d, safe, dry, wet = trapezoids
    tol = check.tangent_tolerance(d, fns["geff_literal"], lean_pow=True, S=S)
    rng = np.random.default_rng(100 + W)
    groups = 64 // W
    # the four cases.  A launch's wave-uniform count is the smallest count of the wave's items: waves are filled with items of ONE
    # count (a count repeated over whole waves), so every wave's count is known here.
    counts = np.unique(safe[wet])
    rem_nonzero = [c for c in counts if c >= W and c % W != 0]
    rem_zero = [c for c in counts if c >= W and c % W == 0]
    declined = [c for c in counts if c < W]
    cases = {"n_safe = nint": dry[:2 * groups + 1]}  # (two full waves and a last, partly filled one)
    if rem_nonzero:
        cases["n_safe < nint, n_safe % W != 0"] = wet[safe[wet] == rem_nonzero[len(rem_nonzero) // 2]]
    if rem_zero:
        cases["n_safe < nint, n_safe % W == 0"] = wet[safe[wet] == rem_zero[0]]
    if declined:
        cases["n_safe < W"] = wet[safe[wet] == declined[-1]]
    assert len(cases) == 4, "W = %d: the fixture's trapezoids reach only the cases %s (safe-node counts %s)" % (W, sorted(cases), counts)
    for what, idx in cases.items():
        # whole waves of one count: the items repeated until the last wave is full (except in the first case)
        if what != "n_safe = nint":
            idx = np.resize(idx, -(-len(idx) // groups) * groups)
            c = int(safe[idx[0]])
            assert (safe[idx] == c).all() and c < NINT and ((c < W) if what == "n_safe < W" else (c >= W and (c % W != 0) == ("!=" in what)))
        sd = _directions(W, len(idx), rng)
        v_s, t_s = _shared(S, d, idx, W, sd)
        v_u, t_u = _unshared(S, d, idx, W, sd)
        # i. values bit for bit
        assert np.array_equal(v_s.view(np.uint64), v_u.view(np.uint64)), (W, what)
        # ii. tangents: the statement within (b)'s tolerance; the unshared launch within 1e-12 |D| more
        want = np.einsum("nwk,nk->nw", sd, d["grad"][idx])
        t = np.einsum("nwk,nk->nw", np.abs(sd), tol[idx])
        err_stmt, err_plain = np.abs(t_s - want), np.abs(t_s - t_u)
        with np.errstate(divide="ignore", invalid="ignore"):
            r1 = np.where(err_stmt == 0, 0.0, err_stmt / t)
            r2 = np.where(err_plain == 0, 0.0, err_plain / (SHARE_GROUPING * np.abs(want) + t))
        k1, k2 = np.unravel_index(np.argmax(r1), r1.shape), np.unravel_index(np.argmax(r2), r2.shape)
        print("W = %2d %-32s %4d items (n_safe %3d): shared - statement <= %.3g of the tolerance (%s lane %d); shared - unshared <= %.3g of 1e-12 |D| + tolerance, %.2e |D| at worst"
              % (W, what, len(idx), int(safe[idx].min()), r1[k1], names[d["soil"][idx[k1[0]]]], k1[1], r2[k2],
                 float(np.max(np.where(want != 0, err_plain / np.abs(np.where(want != 0, want, 1.0)), 0.0)))))
        assert np.isfinite(t_s).all() and r1[k1] <= 1.0 and r2[k2] <= 1.0, (W, what)
        # the shared path was taken where it must be and declined where it must decline: its tangents come from five sums in
        # another order than the plain loop's, so they differ in their last bits (never in all of W x items by chance); a launch
        # that fell back to the plain loop would return the unshared tangents bit for bit -- as the declined case must
        if what == "n_safe < W":
            assert np.array_equal(t_s.view(np.uint64), t_u.view(np.uint64)), (W, what)
        else:
            assert (t_s != t_u).any(), (W, what)


@pytest.mark.parametrize("W", WIDTHS)
def test_shared_group_does_not_depend_on_its_wave(fixture, trapezoids, W):
    """iii. A group alone in its wave, next to groups whose nodes fall under the cut (a smaller wave-uniform n_safe: other blocks,
    another summation order of the tangent) and in a last, partly filled wave: the same value bit for bit, tangents within ii.
    iv. An item outside the domain (theta > theta_e: Se > 1): NaN in value and tangent in every lane of its group, the wave's other
    groups as they are without it."""
    S, names, fns, _ = fixture
    d, safe, dry, wet = trapezoids
    tol = check.tangent_tolerance(d, fns["geff_literal"], lean_pow=True, S=S)
    rng = np.random.default_rng(200 + W)
    groups = 64 // W
    mine = dry[:: max(1, len(dry) // 24)][:24]
    sd = _directions(W, len(mine), rng)
    want = np.einsum("nwk,nk->nw", sd, d["grad"][mine])
    t = np.einsum("nwk,nk->nw", np.abs(sd), tol[mine])
    within = lambda tan: (np.abs(tan - want) <= t).all()
    v_ref, t_ref = _shared(S, d, mine, W, sd)  # among its own kind; the last wave partly filled
    assert within(t_ref)
    bits = lambda a: a.view(np.uint64)
    if groups > 1:
        # alone in the wave: every other group of the wave is past the last item -- one launch per item
        for k in (0, len(mine) - 1):
            v1, t1 = _shared(S, d, mine[k:k + 1], W, sd[k:k + 1])
            assert np.array_equal(bits(v1), bits(v_ref[k:k + 1])) and (np.abs(t1 - want[k]) <= t[k]).all()
        # next to wet groups: each wave = one of mine + (groups - 1) trapezoids up to theta_e
        other = np.resize(wet, len(mine) * (groups - 1)).reshape(len(mine), groups - 1)
        idx = np.concatenate([mine[:, None], other], axis=1).reshape(-1)
        sd_all = _directions(W, len(idx), rng)
        sd_all[::groups] = sd
        v2, t2 = _shared(S, d, idx, W, sd_all)
        assert safe[idx].reshape(len(mine), groups).min(axis=1).max() < NINT  # every wave's count is below nint
        assert np.array_equal(bits(v2[::groups]), bits(v_ref)) and within(t2[::groups])
        v_u, _ = _unshared(S, d, idx, W, sd_all)
        assert np.array_equal(bits(v2), bits(v_u))
    # iv. theta1 beyond theta_e in one group of each wave
    idx = np.resize(mine, max(groups, 2) * 3)
    x = d["x"][idx].copy()
    bad = np.arange(1 if groups > 1 else 0, len(idx), max(groups, 2))
    x[bad] = S[d["soil"][idx[bad]], 3] + 0.05
    sd4 = _directions(W, len(idx), rng)
    seeds = {k: sd4[:, :, j] for j, k in enumerate(check.SEED_NAMES)}
    v4, t4 = gpu_tbatch(4, x, d["y"][idx], seeds=seeds, share=W, nint=NINT, **check.soil_kw(S, d["soil"][idx]))
    good = np.setdiff1d(np.arange(len(idx)), bad)
    assert np.isnan(v4[bad]).all() and np.isnan(t4[bad]).all()
    v5, t5 = _shared(S, d, idx[good], W, sd4[good])
    assert np.array_equal(bits(v4[good]), bits(v5))
    w4 = np.einsum("nwk,nk->nw", sd4[good], d["grad"][idx[good]])
    assert (np.abs(t4[good] - w4) <= np.einsum("nwk,nk->nw", np.abs(sd4[good]), tol[idx[good]])).all()
