"""The code object of one kernel unit of bev_amd/csrc, for the tests that bound its kernels' resources: the unit is compiled for the
device only with the Makefile's own flags, and every kernel's registers, scratch and LDS are read from llvm-readelf --notes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bev_amd", "csrc")


def makefile_flags(unit, header=None):
    """CXXFLAGS of the Makefile, which must build `unit` and (where given) rebuild it after an edit to `header`."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        text = f.read()
    assert unit in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    assert header is None or header in re.search(r"^KERNEL_HDRS = (.*)$", text, re.M).group(1).split()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1)
    assert "-ffp-contract=off" in flags
    return flags.replace("$(ARCH)", "gfx950").split()


def kernels(unit, tmp_path, header=None):
    """{kernel name: {"vgpr_count", "sgpr_count", "scratch", "lds"}} of every kernel in the unit's gfx950 code object."""
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("hipcc is absent")
    readelf = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf") or "/opt/rocm/llvm/bin/llvm-readelf"
    co = str(tmp_path / (os.path.splitext(unit)[0] + ".co"))
    subprocess.check_call([hipcc] + makefile_flags(unit, header) + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", unit, "-o", co], cwd=CSRC)
    notes = subprocess.check_output([readelf, "--notes", co], text=True)
    out = {}
    for entry in re.split(r"^\s*- \.agpr_count:", notes, flags=re.M)[1:]:  # (a kernel's first field; its arguments' names lie inside the entry)
        field = lambda key: int(re.search(r"^\s*\.%s:\s+(\d+)\s*$" % key, entry, re.M).group(1))  # noqa: E731
        name = re.search(r"^\s*\.symbol:\s+(\S+)\.kd\s*$", entry, re.M).group(1)
        assert re.search(r"^\s*\.name:\s+%s\s*$" % re.escape(name), entry, re.M), name
        out[name] = {"vgpr_count": field("vgpr_count"), "sgpr_count": field("sgpr_count"), "scratch": field("private_segment_fixed_size"),
                     "lds": field("group_segment_fixed_size")}
    assert len(out) == len(re.findall(r"\.private_segment_fixed_size:", notes)) == len(re.findall(r"\.group_segment_fixed_size:", notes))  # none missed
    return out


def assert_lean(found):
    """No scratch, no LDS, and at most 128 VGPRs: the four waves per SIMD that the launches are sized against."""
    for name, k in found.items():
        assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr_count"] <= 128, (name, k)
