"""The pure-host half of giql_hip_inner -- the host pool (giql_amd/csrc/host_pool.h) and the expansion of a compact
plan by a team of threads (giql_amd/csrc/plan_expand.h) -- checked without a GPU.

tests/native/host_side_check.cpp is a stand-alone program over the two headers: it is built here without any
sanitizer and run under a time limit (a hang of the thread team fails, it does not stall the suite).  The same
program runs under ASan + UBSan and TSan from tools/host_side_sanitize.sh, by hand.
"""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "host_side_check.cpp")

EXPANSION_CASES = [
    "every count zero",
    "one query, one pair",
    "short block off a 64-byte line",
    "block of 1024 pairs after the head",
    "block of 1024 + 15 pairs after the head",
    "one run of 5000 ids across staging refills",
    "long stretches of zero counts",
    "lo not monotone within a block",
    "a range past the sorted ids",
    "counts that miss the promised total",
    "chunks arrive one at a time",
    "the second of four chunks fails",
]
POOL_CASES = [
    "get, put, get of a similar size: the same pointer",
    "two live buffers never alias",
    "best fit: the smallest sufficient idle buffer",
    "a 4-byte request leaves an 8 MiB idle buffer alone",
    "page-locked serves plain, plain never serves page-locked",
    "put of an unknown pointer: one page-locked release",
    "over the idle limit the smallest go first",
    "idle limit 0 keeps nothing",
    "trim to keep_bytes: the largest first, bytes reported",
    "zero bytes served as one; allocation failure returns nullptr",
    "everything back and trimmed to 0: allocations and releases balance",
    "four threads get and put",
]


def _compiler():
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    assert cxx, "g++ (or ROCm's clang++) is part of the image"
    return cxx


def test_host_pool_and_plan_expansion(tmp_path):
    exe = tmp_path / "host_side_check"
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-pthread", "-o", str(exe), SOURCE], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    for name in EXPANSION_CASES:
        assert f"ok   expand: {name}" in lines, name
    for name in POOL_CASES:
        assert f"ok   pool: {name}" in lines, name
    assert lines[-1] == "all cases passed"
