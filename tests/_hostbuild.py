"""TEST INFRASTRUCTURE ONLY: the one recipe by which the suite's host builds of the device code (tests/devsim,
tests/post_host, tests/launch_plan) are made with the ROCm clang -- stale by file time, compiled to a temporary name,
renamed into place (several test workers or threads may build the same output at once) -- and the one way their stand-alone
programs are run."""
import os
import subprocess
import threading

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
