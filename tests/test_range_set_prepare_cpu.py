"""The host half of giql_hip_range_set_any_dev (giql_amd/csrc/range_set_prepare.h) -- the ranges of a set ordered by
(chromosome, bound), the running aggregate that restarts at every chromosome, the one-search lookup -- checked without
a GPU.

tests/native/range_set_check.cpp is a stand-alone program over the header: it is built here without any sanitizer and
run under a time limit.  The same program builds with ``-fsanitize=address,undefined``, by hand.
"""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "range_set_check.cpp")

CASES = [
    "one range",
    "duplicate ranges",
    "nested ranges",
    "a long range sorted well before the row's neighbours",
    "a segment per chromosome",
    "the aggregate does not leak across a chromosome boundary",
    "bounds at both ends of int64",
    "1024 ranges",
    "no ranges, too many and an unknown operator are refused",
]


def _compiler():
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    assert cxx, "g++ (or ROCm's clang++) is part of the image"
    return cxx


def test_range_set_preparation(tmp_path):
    exe = tmp_path / "range_set_check"
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-o", str(exe), SOURCE], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    for name in CASES:
        assert f"ok   range_set: {name}" in lines, name
    assert lines[-1] == "all cases passed"
