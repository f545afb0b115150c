"""The ledger of the workspace bytes a call zeroed up front, and the Carver's zeroed span
(giql_amd/csrc/zero_ledger.h) -- what the ledger covers, what it hands over once and refuses afterwards, how its range
grows -- checked without a GPU.

tests/native/zero_ledger_check.cpp is a stand-alone program over the header: it is built here without any sanitizer and
run under a time limit.  The same program builds with ``-fsanitize=address,undefined``, by hand.
"""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "zero_ledger_check.cpp")

CASES = [
    "an empty ledger covers nothing",
    "a buffer inside the range is taken once and refused the second time",
    "a buffer that straddles either end is refused",
    "a buffer outside is refused",
    "add at the end of the range extends it",
    "add anywhere else leaves the ledger as it was",
    "the taken list, once full, refuses",
    "reset forgets the range and the taken list",
    "a zero-byte buffer",
    "the Carver's zeroed span is 256-aligned at both ends, a dry run gives the same offsets",
]


def _compiler():
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    assert cxx, "g++ (or ROCm's clang++) is part of the image"
    return cxx


def test_zero_ledger(tmp_path):
    exe = tmp_path / "zero_ledger_check"
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-o", str(exe), SOURCE], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    for name in CASES:
        assert f"ok   zero_ledger: {name}" in lines, name
    assert lines[-1] == "all cases passed"
