"""CPU: the catchment sums (lgar_catchment_sums / lgar_catchment_spread, include/lgar.h).

The per-lane accumulation and the combine order the GPU kernel runs (lgar_py_amd/csrc/lgar_catchment.hpp) are compiled for the
host into a small stand-alone program (tests/post_host).  Its sums must equal the numpy statement of the definition
(post_host.catchment.sums_ref: a plain loop over the 256 partials and the tree) BIT FOR BIT; the same program built with
AddressSanitizer + UBSan must also get through a corrupt map clean.  CatchmentMap's host logic (the stable sort, the
contiguous fast path, -1, every rejection) needs no GPU either."""
import numpy as np
import pytest

import post_host as PH
from post_host import catchment as CH

T = 3
N = sum(CH.SIZES)  # 2121


def _case(dtype, weighted, permuted, flagged, seed=0, T=T, sizes=CH.SIZES):
    """One map holding catchments of every size of CH.SIZES over random data.  flagged: 40 columns get a fault bit and their
    rows NaN / +-inf (a flagged column's rows are whatever the kernel left: they must not reach a sum); 3 more columns carry a
    status word WITHOUT a fault bit (LGAR_ST_RESUME's bit alone) and stay in."""
    rng = np.random.default_rng(seed)
    N = sum(sizes)
    ids = CH.sized_ids(sizes, permute=7 if permuted else None)
    offsets, order = CH.csr_of(ids, len(sizes))
    assert (order is None) == (not permuted)
    series = ((rng.random((T, N)) - 0.3) * 10.0 ** rng.integers(-3, 4, (T, N))).astype(dtype)
    c = dict(series=series, offsets=offsets, order=order, ids=ids, grad=rng.standard_normal((2, len(sizes))))
    if weighted:
        c["weights"] = rng.random(N).astype(dtype)
    if flagged:
        st = np.zeros(N, dtype=np.int32)
        bad = rng.choice(N, 43, replace=False)
        st[bad[:40]] = 2 ** rng.integers(0, 7, 40)
        st[bad[40:]] = 128
        series[:, bad[:20]] = np.nan
        series[0, bad[20:30]] = np.inf
        series[1:, bad[20:30]] = -np.inf
        c["status"] = st
    return c


KEYS = [(dt, w, p, f) for dt in (np.float64, np.float32) for w in (False, True) for p in (False, True) for f in (False, True)]


@pytest.fixture(scope="module")
def results():
    """Every combination in ONE run of the host program; the numpy reference is computed once per case."""
    cases = [_case(*k) for k in KEYS]
    got = PH.run(map(CH.case, cases))
    ref = [CH.sums_ref(c["series"], c["offsets"], c["order"], c.get("weights"), c.get("status")) for c in cases]
    return {k: (c, g, r) for k, c, g, r in zip(KEYS, cases, got, ref)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_host_build_equals_the_numpy_definition_bit_for_bit(results, dtype):
    """Sizes 0, 1, 63, 64, 65, 255, 256, 257 and 1000 in one map, three rows; with and without weights, contiguous and
    permuted, with and without flagged members over NaN / inf rows: sums and weight sums."""
    for k in KEYS:
        if k[0] is not dtype:
            continue
        c, (sums, wsum, _), (rs, rw) = results[k]
        assert sums.shape == (T, len(CH.SIZES)) and CH.same_bits(sums, rs), k[1:]
        assert CH.same_bits(wsum, rw), k[1:]
        assert np.isfinite(sums).all() and (sums[:, 0] == 0.0).all() and not np.signbit(sums[:, 0]).any()  # NaN kept out; empty = +0.0
        if not k[3]:
            # (and the definition means what it says: within the bound of two fp64 summation orders of numpy's own sum)
            w = np.ones(N) if "weights" not in c else c["weights"].astype(np.float64)
            x = w[None, :] * c["series"].astype(np.float64)
            for b, n in enumerate(CH.SIZES):
                m = c["ids"] == b
                assert (np.abs(sums[:, b] - x[:, m].sum(axis=1)) <= 2 * max(n, 1) * 2.0 ** -53 * np.abs(x[:, m]).sum(axis=1)).all()
            if "weights" not in c:
                assert wsum.tolist() == list(CH.SIZES)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_four_rows_per_wave_give_the_same_bits(dtype):
    """In jobs of many catchments a wave carries its catchment through four rows at once (column, status and weight read once
    for the four, one set of partials per row): six rows -- a full group and a ragged one -- against the same numpy loop."""
    cases = [dict(_case(dtype, w, p, True, seed=5, T=6), rows_per_wave=4) for w in (False, True) for p in (False, True)]
    for c, (sums, wsum, _) in zip(cases, PH.run(map(CH.case, cases))):
        rs, rw = CH.sums_ref(c["series"], c["offsets"], c["order"], c.get("weights"), c.get("status"))
        assert sums.shape == (6, len(CH.SIZES)) and CH.same_bits(sums, rs) and CH.same_bits(wsum, rw)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_catchments_beyond_one_block_of_loads(dtype):
    """From 1024 members on a lane of the one-row kernel runs its main loop, whole blocks of 16 loads (four rows a wave: blocks of
    4 loads, from 256 members on): catchments of 2500, 1024, 1025 and 1023 members, one and four rows per wave, five rows (a
    full group and a ragged one), weighted and flagged, contiguous and permuted, against the same numpy loop."""
    cases = [dict(_case(dtype, True, p, True, seed=9, T=5, sizes=CH.BIG_SIZES), rows_per_wave=r) for p in (False, True) for r in (1, 4)]
    cases.append(_case(dtype, False, False, False, seed=10, T=2, sizes=CH.BIG_SIZES))
    for c, (sums, wsum, _) in zip(cases, PH.run(map(CH.case, cases))):
        rs, rw = CH.sums_ref(c["series"], c["offsets"], c["order"], c.get("weights"), c.get("status"))
        assert sums.shape[1] == len(CH.BIG_SIZES) and CH.same_bits(sums, rs) and CH.same_bits(wsum, rw) and np.isfinite(sums).all()
    assert wsum.tolist() == list(CH.BIG_SIZES)  # (the last case: no weights, nothing flagged)


def test_flagged_members_are_skipped_not_multiplied_by_zero(results):
    """Dropping the flagged columns from the map by hand gives the same bits as flagging them only when they were the LAST
    members of their partials; what must hold in general: a flagged member contributes nothing -- the sums equal those of the
    same data with the flagged columns' rows replaced by any finite garbage."""
    c, (sums, wsum, _), _ = results[(np.float64, True, True, True)]
    other = dict(c, series=c["series"].copy())
    bad = (c["status"] & CH.FAULT_MASK) != 0
    other["series"][:, bad] = 12345.0
    (s2, w2, _), = PH.run(map(CH.case, [other]))
    assert CH.same_bits(sums, s2) and CH.same_bits(wsum, w2)
    # a status word without a fault bit does not skip: clearing it changes nothing, setting a fault bit there does
    kept = dict(c, status=np.where(c["status"] == 128, 0, c["status"]))
    dropped = dict(c, status=np.where(c["status"] == 128, 64, c["status"]))
    (s3, *_), (s4, *_) = PH.run(map(CH.case, [kept, dropped]))
    assert CH.same_bits(sums, s3) and not CH.same_bits(sums, s4)


def test_a_catchment_is_a_function_of_its_own_members():
    """The 1000-member catchment alone in a map, embedded 77 columns further on, gives the bits it gives among the others."""
    c = _case(np.float32, True, False, False)
    lo = sum(CH.SIZES[:-1])
    alone = dict(series=np.concatenate([np.full((T, 77), np.nan, np.float32), c["series"][:, lo:]], axis=1),
                 weights=np.concatenate([np.zeros(77, np.float32), c["weights"][lo:]]),
                 offsets=np.array([0, 77, 77 + 1000], dtype=np.int32))
    (full, fw, _), (part, pw, _) = PH.run(map(CH.case, [c, alone]))
    assert CH.same_bits(full[:, -1], part[:, 1]) and fw[-1] == pw[1] and np.isnan(part[:, 0]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_spread_on_the_host(results, dtype):
    for k in KEYS:
        if k[0] is dtype:
            c, (_, _, spread), _ = results[k]
            ids = c["ids"].copy()
            assert CH.same_bits(spread, CH.spread_ref(c["grad"], ids, c.get("weights"), c.get("status"), dtype))
            if k[3]:
                assert (spread[:, (c["status"] & CH.FAULT_MASK) != 0] == 0).all() and (spread[:, c["status"] == 128] != 0).all()
    ids = CH.sized_ids()
    ids[5:9] = -1
    ids[100] = 40  # (beyond B: no catchment either)
    c = dict(_case(dtype, True, False, False), ids=ids)
    (_, _, spread), = PH.run(map(CH.case, [c]))
    assert CH.same_bits(spread, CH.spread_ref(c["grad"], ids, c["weights"], None, dtype))
    assert (spread[:, 5:9] == 0).all() and (spread[:, 100] == 0).all() and (spread[:, 9:100] != 0).all()


def _corrupt(dtype):
    """A map that keeps none of the C-ABI's promises: order entries of -5 and N + 7, offsets that decrease, offsets[B] beyond
    the order array, a negative offset."""
    rng = np.random.default_rng(1)
    n = 300
    order = rng.permutation(n).astype(np.int32)[:280]
    order[[3, 70, 279]] = -5
    order[[4, 200]] = n + 7
    offsets = np.array([0, 90, 40, 130, -6, 280, 5000], dtype=np.int32)
    st = np.zeros(n, dtype=np.int32)
    st[::17] = 1
    return dict(series=rng.standard_normal((2, n)).astype(dtype), offsets=offsets, order=order, weights=rng.random(n).astype(dtype),
                status=st, ids=rng.integers(-3, 9, n).astype(np.int32), grad=rng.standard_normal((2, 6)))


def test_sanitizer_build_on_the_cases_and_a_corrupt_map():
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python; every
    array is allocated at its exact size) over the size-set cases, catchments large enough for the kernels' main loops, and corrupt maps -- with and without an order array:
    memory safety comes before meaning, offsets are clamped and out-of-range members skipped, so it finishes clean with the
    bits of the plain build.  Any finding aborts the program."""
    cases = [_case(np.float64, True, True, True), _case(np.float32, False, False, True), _case(np.float32, True, True, False)]
    cases += [dict(_case(dt, True, p, True, T=5, sizes=CH.BIG_SIZES), rows_per_wave=r)  # (the main loops of both kernels)
              for dt, p, r in ((np.float32, False, 1), (np.float64, True, 1), (np.float32, True, 4))]
    for dtype in (np.float64, np.float32):
        bad = _corrupt(dtype)
        cases += [bad, dict(bad, rows_per_wave=4), dict(_case(dtype, True, True, True, T=6), rows_per_wave=4), dict(bad, order=None, offsets=np.array([0, 90, 40, 130, -6, 280, 5000], dtype=np.int32)),
                  dict(bad, series=bad["series"][:, :0], weights=bad["weights"][:0], status=bad["status"][:0], ids=bad["ids"][:0])]
    got = PH.run(map(CH.case, cases), sanitize=True)
    plain = PH.run(map(CH.case, cases))
    for c, a, b in zip(cases, got, plain):
        for x, y in zip(a, b):
            assert (x is None and y is None) or CH.same_bits(x, y)
        rs, rw = CH.sums_ref(c["series"], c["offsets"], c.get("order"), c.get("weights"), c.get("status"))
        assert CH.same_bits(a[0], rs) and CH.same_bits(a[1], rw)
    s = got[6][0]
    assert (s[:, 1] == 0).all() and (s[:, 3] == 0).all() and np.isfinite(s).all()  # decreasing offsets: empty catchments
    assert (got[10][0] == 0).all()  # no columns at all: every member is out of range


# CatchmentMap's host logic ---------------------------------------------------------------------------------------------------
def _map(*a, **kw):
    from lgar_py_amd.catchments import CatchmentMap
    return CatchmentMap(*a, device="cpu", **kw)


def test_map_sorts_stably_and_detects_contiguous_ids():
    import torch
    ids = np.array([2, 0, -1, 2, 1, 0, -1, 2, 0])
    m = _map(ids)
    assert (m.B, m.N) == (3, 9) and m.sizes.tolist() == [3, 1, 3]
    assert m.offsets_host.tolist() == [0, 3, 4, 7] and m.order_host.tolist() == [1, 5, 8, 4, 0, 3, 7]  # column order kept
    assert m.order.dtype == torch.int32 and m.offsets.dtype == torch.int32 and m.ids.tolist() == ids.tolist()
    for perm_seed in (None, 3):
        big = CH.sized_ids(permute=perm_seed)
        m = _map(torch.tensor(big), weights=np.ones(len(big)))
        offsets, order = CH.csr_of(big, len(CH.SIZES))
        assert np.array_equal(m.offsets_host, offsets) and m.sizes.tolist() == list(CH.SIZES)
        assert (m.order is None and order is None) if perm_seed is None else np.array_equal(m.order_host, order)
    # non-decreasing ids WITH a gap are still contiguous; a -1 anywhere, or one inversion, needs the order array
    assert _map([0, 0, 2, 2, 5]).order is None and _map([0, 0, 2, 2, 5]).sizes.tolist() == [2, 0, 2, 0, 0, 1]
    assert _map([0, 0, -1, 1]).order_host.tolist() == [0, 1, 3] and _map([0, 1, 0]).order_host.tolist() == [0, 2, 1]
    assert _map([-1, -1]).B == 0 and _map([-1, -1], n_catchments=4).offsets_host.tolist() == [0] * 5
    assert _map(np.array([], dtype=np.int64), n_catchments=2).N == 0 and _map(np.array([1, 1], dtype=np.uint8), n_catchments=3).sizes.tolist() == [0, 2, 0]
    m = _map([0, 1], weights=[0.25, 0.1])
    assert m.weights(torch.float32).dtype == torch.float32 and m.weights(torch.float64).tolist() == [0.25, 0.1] and _map([0]).weights(torch.float64) is None


def test_map_rejections():
    import torch
    from lgar_py_amd import LgarError
    for bad in (dict(ids=[0.0, 1.0]), dict(ids=np.array([True, False])), dict(ids=[[0, 1]]), dict(ids=[0, 3], n_catchments=3),
                dict(ids=[0, -2]), dict(ids=[0, 1], weights=[1.0]), dict(ids=[0, 1], weights=[1.0, float("nan")]),
                dict(ids=[0, 1], weights=[float("inf"), 1.0]), dict(ids=[0, 1], weights=[[1.0, 1.0]]), dict(ids=[0], n_catchments=-1),
                dict(ids=torch.tensor([0.5]))):
        with pytest.raises(LgarError):
            _map(**bad)
    # a map on the CPU holds the host logic only: the sums themselves have no CPU fallback
    m = _map([0, 1, 1])
    with pytest.raises(LgarError, match="no CPU fallback"):
        m.sums(torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(LgarError, match="no CPU fallback"):
        m.spread(torch.zeros(2, 2, dtype=torch.float64), torch.float64)
