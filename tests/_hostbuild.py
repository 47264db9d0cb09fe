"""TEST INFRASTRUCTURE ONLY: the one recipe by which the suite's host builds of the device code (tests/devsim, tests/*_host,
tests/launch_plan) are made with the ROCm clang -- stale by file time, compiled to a temporary name, renamed into place (several
test workers or threads may build the same output at once) -- and the one way their stand-alone programs are run.  For the units
whose program reads call records (tests/_hostprog.hpp: post_host and the six catchment-stage packages) also the one harness:
HostUnit (program, library, one run over many calls), Out, AsHipLibrary (a host library behind the product's calling surface) and
same_bits."""
import ctypes as C
import os
import struct
import subprocess
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lgar_py_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
# AddressSanitizer + UBSan, any finding aborts
SANITIZE = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def device_headers():
    """include/lgar.h and every header of lgar_py_amd/csrc (taken from the directory, not from a hand-kept list)."""
    return [os.path.join(ROOT, "include", "lgar.h")] + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".hpp")]


def build(out, source, deps, flags=(), what="a host build of the device code"):
    """`out`, compiled from `source` as C++17 with `flags` unless it is newer than the source and every file of `deps`."""
    deps = [source] + list(deps)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        if not os.path.exists(CLANG):
            raise RuntimeError("clang++ of the ROCm toolchain not found: cannot build " + what)
        tmp = "%s.%d.%d.tmp" % (out, os.getpid(), threading.get_ident())
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off"] + list(flags) + [source, "-o", tmp])
        os.replace(tmp, out)
    return out


def run_clean(argv):
    """Run a stand-alone host program (a sanitizer build halts at its first finding) and require a clean exit: status 0,
    nothing on stderr.  Returns its stdout."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and not p.stderr.strip(), (p.returncode, p.stderr[-4000:])
    return p.stdout


def same_bits(a, b):
    """Bit-for-bit equality of two float arrays, fp32 or fp64 (NaNs must sit in the same places)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(u)[~na] == b.view(u)[~nb]).all())


class Out:
    """An output array of a call: the program allocates it at exactly this size and writes it back into .value.  start: what
    it holds before the call (an array that is input and output), default: nothing meaningful (all-ones bytes)."""

    def __init__(self, dtype, *shape, start=None):
        self.dtype, self.shape, self.start, self.value = np.dtype(dtype), shape, start, None


def f64(a):
    """a (or None) as a contiguous fp64 array, what a call record takes for an input"""
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def out(want, *shape):
    """A fp64 Out of `shape`, or None (a null pointer) where the case asks for none"""
    return Out(np.float64, *shape) if want else None


def call_records(calls, null_when_empty):
    """(the input file of a host program, its Outs in the order the program writes them) for a list of calls
    (operation number, int32 scalars, fp64 scalars, arrays) -- tests/_hostprog.hpp states the format.  An array is a numpy
    array (an input), None (a null pointer) or an Out; null_when_empty: an array of no elements is a null pointer too."""
    blob, outs = [struct.pack("i", len(calls))], []
    for op, ints, doubles, arrays in calls:
        blob.append(struct.pack("=4i%di%dd" % (len(ints), len(doubles)), op, len(ints), len(doubles), len(arrays), *ints, *doubles))
        for a in arrays:
            if isinstance(a, Out):
                outs.append(a)
            size = 0 if a is None else int(np.prod(a.shape))
            if a is None or (null_when_empty and size == 0):
                blob.append(struct.pack("=2iq", 1, 3, 0))
            elif isinstance(a, Out):
                blob.append(struct.pack("=2iq", a.dtype.itemsize, 1 if a.start is None else 2, size))
                if a.start is not None:
                    blob.append(np.ascontiguousarray(a.start, dtype=a.dtype).reshape(a.shape).tobytes())
            else:
                a = np.ascontiguousarray(a)
                blob += [struct.pack("=2iq", a.dtype.itemsize, 0, a.size), a.tobytes()]
    return b"".join(blob), outs


class HostUnit:
    """One unit's host build: <directory>/<stem>.hpp holds the host-side launchers of its entry points, <prefix>_<name>(the
    arguments of include/lgar.h without the stream); <stem>.cpp is the stand-alone program around them (its dispatch() under
    tests/_hostprog.hpp), lib<prefix>.so the same header as a shared library.  deps: the device headers it includes; what: the
    unit in words.  null_when_empty: see call_records."""

    def __init__(self, directory, stem, prefix, deps, what, null_when_empty=True):
        self.directory, self.stem, self.prefix, self.what, self.null_when_empty = directory, stem, prefix, what, null_when_empty
        self.hpp = os.path.join(directory, stem + ".hpp")
        self.deps = [os.path.join(CSRC, d) for d in deps] + [os.path.join(ROOT, "include", "lgar.h")]
        self._lib, self._lock = None, threading.Lock()

    def program(self, sanitize=False):
        """The host program, built on first use with the ROCm clang (sanitize: AddressSanitizer + UBSan, any finding aborts)."""
        return build(os.path.join(self.directory, self.stem + ("_san" if sanitize else "")), os.path.join(self.directory, self.stem + ".cpp"),
                     [self.hpp, os.path.join(ROOT, "tests", "_hostprog.hpp")] + self.deps, SANITIZE if sanitize else [],
                     "the %s host program" % self.what)

    def library(self, argtypes, restypes=None):
        """lib<prefix>.so, loaded once.  argtypes: {entry point: its ctypes argument types}; restypes: the same for the entry
        points that do not return an int."""
        with self._lock:
            if self._lib is None:
                lib = C.CDLL(build(os.path.join(self.directory, "lib%s.so" % self.prefix), self.hpp, self.deps, ["-fPIC", "-shared"],
                                   "the %s host library" % self.what))
                for name, types in argtypes.items():
                    getattr(lib, "%s_%s" % (self.prefix, name)).argtypes = types
                for name, res in (restypes or {}).items():
                    getattr(lib, "%s_%s" % (self.prefix, name)).restype = res
                self._lib = lib
        return self._lib

    def run_calls(self, calls, sanitize=False):
        """ONE run of the host program over every call of call_records; the arrays the program wrote are the Outs' .value."""
        blob, outs = call_records(list(calls), self.null_when_empty)
        with tempfile.TemporaryDirectory() as tmp:
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(fin, "wb") as fh:
                fh.write(blob)
            run_clean([self.program(sanitize), fin, fout])
            raw = open(fout, "rb").read()
        at = 0
        for o in outs:
            n = int(np.prod(o.shape)) * o.dtype.itemsize
            o.value = np.frombuffer(raw[at:at + n], dtype=o.dtype).reshape(o.shape).copy()
            at += n
        assert at == len(raw)


def values(outs):
    """What the program wrote into a case's Outs, None where the case asked for none."""
    return tuple(None if o is None else o.value for o in outs)


class AsHipLibrary:
    """Host libraries under the HIP library's names: lgar_<name>(arguments, stream) is <prefix>_<name>(arguments).  libraries:
    (claims, prefix, load) each -- the first whose `claims` <name> starts with ("" claims the rest) serves the call, load() gives
    its library.  hook(name, function): a unit's own way of calling one entry point, or None for the plain one."""

    def __init__(self, *libraries, hook=None):
        self.libraries, self.hook = libraries, hook

    def __getattr__(self, name):
        short = name[len("lgar_"):]
        prefix, load = next((p, ld) for claims, p, ld in self.libraries if short.startswith(claims))
        fn = getattr(load(), "%s_%s" % (prefix, short))
        return (self.hook and self.hook(name, fn)) or (lambda *args: fn(*args[:-1]))
