"""TEST INFRASTRUCTURE ONLY: front-end of the stand-alone host program (tests/launch_plan/launch_plan.cpp) that prints the launch
plans of lgar_py_amd/csrc/lgar_plan.hpp -- the header the library's launchers and the device-code simulator share -- compiled for
the host with -DLGAR_DEVSIM.  Never imported by the product package.
"""
import json
import os

import _hostbuild

_HERE = os.path.dirname(os.path.abspath(__file__))


def program(sanitize=False):
    """The host program, built on first use with the ROCm clang (sanitize: AddressSanitizer + UBSan, any finding aborts)."""
    return _hostbuild.build(os.path.join(_HERE, "launch_plan_san" if sanitize else "launch_plan"),
                            os.path.join(_HERE, "launch_plan.cpp"), _hostbuild.device_headers(),
                            _hostbuild.SANITIZE if sanitize else [], "the launch-plan host program")


def _run(args, sanitize):
    return [json.loads(line) for line in _hostbuild.run_clean([program(sanitize)] + args).splitlines()]


def forward_plans(cases, sanitize=False):
    """cases: dicts of fp64 (bool), N and optionally layers, subcycles, nint, front_slots, search_mode, geff_mode,
    use_closed_form_G, forward_lanes, simds.  One dict per case: literal, mixed, coop, caps, steps."""
    get = lambda c, k, default: int(c.get(k, default))
    return _run(["f,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d" % (
        get(c, "fp64", 0), c["N"], get(c, "layers", 3), get(c, "subcycles", 1), get(c, "nint", 120), get(c, "front_slots", 0),
        get(c, "search_mode", 1), get(c, "geff_mode", 0), get(c, "use_closed_form_G", 0), get(c, "forward_lanes", 0),
        get(c, "simds", 1024)) for c in cases], sanitize)


def tangent_plans(cases, sanitize=False):
    """cases: dicts of N and optionally layers, subcycles, front_slots, search_mode, tangent_share.  One dict per case: literal,
    columns_per_block, caps, steps."""
    get = lambda c, k, default: int(c.get(k, default))
    return _run(["t,%d,%d,%d,%d,%d,%d" % (c["N"], get(c, "layers", 3), get(c, "subcycles", 1), get(c, "front_slots", 0),
                                          get(c, "search_mode", 1), get(c, "tangent_share", 0)) for c in cases], sanitize)
