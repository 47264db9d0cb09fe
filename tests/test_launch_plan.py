"""CPU: what a lgar_forward / lgar_forward_tangent call launches.  lgar_py_amd/csrc/lgar_plan.hpp decides it for the library and
for the device-code simulator alike; a stand-alone host program (tests/launch_plan) prints its plans.  The expected tables were
derived by hand from the launchers as they were before the plans had a header of their own (forward_typed, tangent_typed), for a
chip of 1024 SIMDs; unstated fields are 3 layers, 1 sub-cycle, nint 120, front_slots 0, search_mode 1."""
import pytest

import launch_plan as LP

M = 1048576
FULL, MID_UP, SMALL_LAST, LAST = [8, 16, 32], [16, 32], [8, 32], [32]
# (case, caps, coop, literal, mixed)
FORWARD = [
    (dict(N=M), FULL, 1, False, False),
    (dict(N=65536), LAST, 1, False, False),
    (dict(N=65537), FULL, 1, False, False),
    (dict(N=64, search_mode=2), FULL, 1, False, False),
    (dict(N=M, front_slots=16), SMALL_LAST, 1, False, False),
    (dict(N=M, front_slots=8), LAST, 1, False, False),
    (dict(N=M, subcycles=8), MID_UP, 1, False, False),
    (dict(N=M, layers=6, subcycles=12), LAST, 1, False, False),
    (dict(N=M, search_mode=0), LAST, 1, True, False),
    (dict(fp64=1, N=100), LAST, 64, False, False),
    (dict(fp64=1, N=100, geff_mode=1), LAST, 64, False, True),
    (dict(fp64=1, N=100, search_mode=2), FULL, 1, False, False),
    (dict(fp64=1, N=100, use_closed_form_G=1), LAST, 1, False, False),
    (dict(fp64=1, N=M), FULL, 1, False, False),
    (dict(fp64=1, N=M, geff_mode=1), FULL, 1, False, True),
    (dict(fp64=1, N=M, forward_lanes=8), LAST, 8, False, False),
]
# (case, caps, columns per block, literal)
TANGENT = [
    (dict(N=100000), SMALL_LAST, 64, False),
    (dict(N=65536), LAST, 64, False),
    (dict(N=64, search_mode=2), SMALL_LAST, 64, False),
    (dict(N=64, search_mode=2, subcycles=4), LAST, 64, False),
    (dict(N=49152, tangent_share=24), LAST, 48, False),
    (dict(N=49176, tangent_share=24), SMALL_LAST, 48, False),
    (dict(N=100000, search_mode=0), LAST, 64, True),
]


def _id(case):
    return ",".join("%s=%s" % kv for kv in case.items())


@pytest.fixture(scope="module")
def plans():
    return LP.forward_plans([c[0] for c in FORWARD]), LP.tangent_plans([c[0] for c in TANGENT])


@pytest.mark.parametrize("k", range(len(FORWARD)), ids=[_id(c[0]) for c in FORWARD])
def test_forward_plan(plans, k):
    _, caps, coop, literal, mixed = FORWARD[k]
    got = plans[0][k]
    assert (got["caps"], got["coop"], bool(got["literal"]), bool(got["mixed"])) == (caps, coop, literal, mixed)


@pytest.mark.parametrize("k", range(len(TANGENT)), ids=[_id(c[0]) for c in TANGENT])
def test_tangent_plan(plans, k):
    _, caps, cpb, literal = TANGENT[k]
    got = plans[1][k]
    assert (got["caps"], got["columns_per_block"], bool(got["literal"])) == (caps, cpb, literal)


def test_chain_positions_and_hand_over_counters(plans):
    """Every kernel's place in its chain comes from one helper: the first has chain_first and nothing handed to it, the last has
    chain_last and hands nothing on, kernel i reads the count kernel i-1 wrote, and no two kernels share a counter."""
    seen = set()
    for got in plans[0] + plans[1]:
        steps = got["steps"]
        n = len(steps)
        assert n == len(got["caps"])
        seen.add(n)
        for i, (first, last, pending_in, pending_out, ticket) in enumerate(steps):
            assert (first, last) == (int(i == 0), int(i == n - 1))
            assert (pending_in == -1) == (i == 0) and (pending_out == -1) == (i == n - 1)
            if i > 0:
                assert pending_in == steps[i - 1][3]
        used = [s[4] for s in steps] + [s[3] for s in steps[:-1]]
        assert -1 not in used and len(set(used)) == len(used) and max(used) < 8  # LGAR_NTICKETS
    assert seen == {1, 2, 3}


def test_sanitizer_build_prints_the_same_plans(plans):
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python); any finding
    aborts it."""
    assert LP.forward_plans([c[0] for c in FORWARD], sanitize=True) == plans[0]
    assert LP.tangent_plans([c[0] for c in TANGENT], sanitize=True) == plans[1]
