#!/usr/bin/env python3
"""Which kernel every public launcher of the kernel units launches, for every combination of its runtime words -- without a GPU
(refactoring check: a change to the host side of a unit must not change what is launched, how, or with what arguments).

    python tools/launch_record.py dump <out.txt> [<tree>]     one line per call of every launcher: the tuple, the kernel's mangled name,
                                                              grid, block, shared memory, stream, a hash of the argument bytes
    python tools/launch_record.py diff <a.txt> <b.txt>        the lines that differ; exit status 1 if any does

dump builds <tree>'s kernel units with its Makefile (default: this repository), compiles tools/launch_record_driver.hip against that
tree's headers, and links both with tools/launch_record_runtime.cpp -- a recording stand-in for the runtime's launch path -- in place
of the HIP runtime.  The result is a stand-alone program: it opens no device and is loaded into no other process.  The launchers'
signatures are the interface, so one driver serves two trees that differ in how they pick the kernel."""
import difflib
import glob
import os
import subprocess
import sys
import tempfile

ROCM = "/opt/rocm"
HERE = os.path.dirname(os.path.abspath(__file__))


def dump(out, tree):
    csrc = os.path.join(tree, "bev_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-j8", "libbevwarp.so"], stdout=subprocess.DEVNULL)
    objects = sorted(glob.glob(os.path.join(csrc, "warp_*.o")))  # (the units with the launchers; the C ABI layer needs the whole runtime)
    with tempfile.TemporaryDirectory() as tmp:
        runtime, driver, exe = (os.path.join(tmp, n) for n in ("runtime.o", "driver.o", "launch_record"))
        subprocess.check_call([ROCM + "/lib/llvm/bin/clang++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", ROCM + "/include", "-c",
                               os.path.join(HERE, "launch_record_runtime.cpp"), "-o", runtime])
        subprocess.check_call([ROCM + "/bin/hipcc", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "--offload-arch=gfx950", "-I", csrc, "-I",
                               os.path.join(tree, "include"), "-c", os.path.join(HERE, "launch_record_driver.hip"), "-o", driver])
        subprocess.check_call([ROCM + "/lib/llvm/bin/clang++", driver, runtime] + objects + ["-o", exe])
        with open(out, "w") as f:
            subprocess.check_call([exe], stdout=f)
    print("%d calls -> %s" % (sum(1 for _ in open(out)), out))


def diff(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    delta = [ln for ln in difflib.unified_diff(la, lb, a, b, n=0, lineterm="") if not ln.startswith("@@")]
    print("%d and %d calls, %d differing lines" % (len(la), len(lb), sum(1 for ln in delta[2:] if ln[0] in "+-")))
    for ln in delta:
        print(ln)
    return 1 if delta else 0


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "dump":
        dump(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) == 4 else os.path.dirname(HERE))
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
