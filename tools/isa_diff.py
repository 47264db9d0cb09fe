"""Which kernels did a change touch?  Compiles lgar_kernels_nl.hip (3 soil layers, the product flags) from the working tree and
from a git revision, disassembles both code objects and compares every kernel instruction by instruction (branch targets and
literal addresses aside).  A kernel reported SAME executes the very instruction stream it did at that revision: its parity
sweeps, counters and timings carry over.  Runs where hipcc is (no GPU needed).
usage: python tools/isa_diff.py [REV=HEAD] [UNIT] [LAYERS=3] [OLD_UNIT ...]
OLD_UNIT ...: the units that held UNIT's kernels at the revision, when they are not UNIT itself (units merged or split since);
their kernels are pooled.  Padding after a kernel's last s_endpgm is no part of its instruction stream and is not compared.
(dev tool)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lgar_py_amd import build as B

LLVM = "/opt/rocm/lib/llvm/bin"
rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
unit = sys.argv[2] if len(sys.argv) > 2 else "lgar_kernels_nl.hip"
old_units = sys.argv[4:] or [unit]
flags = [f for f in B.FLAGS if f != "-shared"] + ["-DLGAR_NL=%d" % (int(sys.argv[3]) if len(sys.argv) > 3 else 3)]


def kernels(src_root, tag, tmp, unit):
    obj = os.path.join(tmp, tag + ".o")
    subprocess.check_call(["hipcc"] + flags + ["-c", os.path.join(src_root, "lgar_py_amd", "csrc", unit), "-o", obj])
    subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + obj + ".fat", obj])
    subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + obj + ".fat", "--output=" + obj + ".co"])
    dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", obj + ".co"], capture_output=True, text=True).stdout
    res, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = m.group(1)
            res[cur] = []
        elif cur and ln.strip():
            res[cur].append(re.sub(r"0x[0-9a-f]+|\d+$", "", ln.split("//")[0].strip()))
    for body in res.values():
        ends = [i for i, ins in enumerate(body) if ins.startswith("s_endpgm")]
        if ends and all(ins == "..." or ins.startswith(("s_nop", "s_code_end")) for ins in body[ends[-1] + 1:]):
            del body[ends[-1] + 1:]
    return res


with tempfile.TemporaryDirectory() as tmp:
    old_root = os.path.join(tmp, "old")
    # the sources as they are at the revision (its headers, not the working tree's: files may have been added or removed since)
    files = subprocess.check_output(["git", "-C", ROOT, "ls-tree", "-r", "--name-only", rev, "lgar_py_amd/csrc", "include"], text=True)
    for rel in files.split():
        if rel.endswith((".h", ".hpp", ".hip")):
            os.makedirs(os.path.dirname(os.path.join(old_root, rel)), exist_ok=True)
            open(os.path.join(old_root, rel), "wb").write(subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (rev, rel)]))
    a, b = {}, kernels(ROOT, "new", tmp, unit)
    for i, u in enumerate(old_units):
        a.update(kernels(old_root, "old%d" % i, tmp, u))
    for k in sorted(set(a) | set(b)):
        name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip().replace("void lgar::", "").split("(")[0]
        print("%-5s %6d -> %6d instructions  %s" % ("SAME" if a.get(k) == b.get(k) else "DIFF", len(a.get(k, [])), len(b.get(k, [])), name))
