"""TEST INFRASTRUCTURE ONLY: the device-code simulator (tests/devsim) built with extra -D switches.

The device code carries switches that turn one piece of work OFF (lgar_py_amd/csrc/lgar_measure.hpp lists them); a CPU test
compares a run with a switch against the run without it.  `engine(flags, ...)` is devsim.SimEngine on a simulator library built
with those flags (libdevsim_<tag>_<L>.so next to the plain ones, rebuilt when a source is newer).
"""
import devsim


def variant_lib(n_layers, flags):
    """The simulator for one soil-layer count compiled with the extra compiler flags `flags` (a tuple of -D... strings)."""
    return devsim.lib(n_layers, tuple(flags))


class VariantEngine(devsim.SimEngine):
    """devsim.SimEngine running a variant library (forward path only)."""

    def __init__(self, flags, *params, **kw):
        self._variant_flags = tuple(flags)
        super().__init__(*params, **kw)

    def _open(self, n_layers, device):
        return variant_lib(n_layers, self._variant_flags), super()._open(n_layers, device)[1]


def prebuild(n_layers, flag_sets):
    """Build several variants concurrently."""
    import concurrent.futures as cf
    jobs = [(n, tuple(fl)) for n in n_layers for fl in flag_sets]
    with cf.ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
        list(ex.map(lambda j: variant_lib(*j), jobs))
