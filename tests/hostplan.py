"""What the CPU tests of the C ABI's host side share: the one builder of the stand-alone drivers of tests/ (host_plan_driver.cpp --
bev_amd/csrc/host_plan.h from the command line, one family of case lines per group of entry points -- launch_pick_driver.cpp and
cubic_tab_driver.cpp), each built once per test run, the runner of a driver that reads case lines, and the library, built when it is
missing."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

from bev_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-Wall", "-Werror"]


@functools.lru_cache(maxsize=None)
def build_driver(sanitize=True, source="host_plan_driver.cpp", extra_flags=()):
    """The driver's path (source: another driver of tests/ built the same way; extra_flags: a tuple of further g++ flags).  sanitize: g++
    under the address and undefined-behaviour sanitizers; a GPU test builds it plainly.
    (-static-libasan: a process that starts with some library preloaded refuses a shared sanitizer runtime that is not the first one)"""
    tmp = tempfile.mkdtemp(prefix="host_plan_driver_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + (SANITIZE if sanitize else []) + list(extra_flags) +
                          ["-I", os.path.join(ROOT, "bev_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", source), "-o", exe])
    return exe


def run_driver(exe, lines, family=None):
    """One list of integers per case line (family: the family of host_plan_driver.cpp the lines belong to, its first argument).  Any
    sanitizer report ends the driver with a non-zero status and fails the caller."""
    r = subprocess.run([exe] + ([family] if family else []), input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    out = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def check_cases(exe, cases, family=None):
    """cases: (line, the numbers it must print) pairs; a failure names the line."""
    got = run_driver(exe, [c for c, _ in cases], family)
    for (c, want), g in zip(cases, got):
        assert g == want, (c, g, want)


def built_lib():
    """The loaded library; a clean checkout builds it first."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()
