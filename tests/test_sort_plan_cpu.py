"""What a sort of the onesweep driver will do (giql_amd/csrc/sort_plan.h: the plan of one sort and the decisions every
other reader shares with it), checked without a GPU.

tests/native/sort_plan_check.cpp is a stand-alone program over the header.  It carries a literal transcription of the
arithmetic the host driver held inline before the plan existed and compares every field of ``plan_sort`` and every
decision function with it over a grid of tunings and requests; then it checks the properties that hold in their own
right.  It is built here without any sanitizer and run under a time limit.  The same program builds with
``-fsanitize=address,undefined``, by hand.
"""

import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "sort_plan_check.cpp")
HEADER = os.path.join(ROOT, "giql_amd", "csrc", "sort_plan.h")

CASES = [
    "every decision function equals the transcription of the previous driver",
    "row_skip and coarse_b_ok give their no-guess answers before any call has run",
    "every field of plan_sort equals the transcription of the previous driver",
    "digits are consecutive and end at digit 3",
    "source and destination alternate from buffer 0 and the result ends in buffer n_pass & 1",
    "the status words zeroed are n_pass x stride",
    "the span pass counts every digit the side's global passes scatter on, for every tuning",
    "a three-stage sort ignores skip_digits; a fused stage only with its own payload; presorted runs only a fused stage",
]


def _compiler():
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    assert cxx, "g++ (or ROCm's clang++) is part of the image"
    return cxx


def test_sort_plan(tmp_path):
    exe = tmp_path / "sort_plan_check"
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe), SOURCE], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    for name in CASES:
        assert any(line.startswith(f"ok   sort_plan: {name}") for line in lines), name
    assert lines[-1] == "all cases passed"


def test_the_header_is_free_of_hip_and_of_the_context():
    text = open(HEADER).read()
    for word in ("hip/hip_runtime", "giql_hip_ctx", "__global__", "__device__", "hipLaunch"):
        assert word not in text, word


def test_the_driver_holds_one_definition_of_each_decision():
    """The host file calls the header's functions; it defines none of them again and restates none inline."""
    host = open(os.path.join(ROOT, "giql_amd", "csrc", "giql_hip.hip")).read()
    for name in ("density_bits", "sort_local_bits", "sort_is_local", "local_passes", "row_skip", "coarse_b_ok",
                 "os_pass_words", "os_pass_stride", "span_hist_mode"):
        assert f"inline int {name}(" not in host and f"inline bool {name}(" not in host and \
            f"inline size_t {name}(" not in host, name
    assert not re.search(r"sort_local_bits\([^;]*== 16 \? 2 : 1", host)
    for macro in ("GIQL_OS_LAUNCH", "GIQL_BS_LAUNCH", "GIQL_BSF_LAUNCH"):
        assert macro not in host, macro
