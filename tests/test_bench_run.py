"""bench.py end to end on small workloads -- needs a GPU.

A plain run prints the headline line and nothing that follows the timed region; ``--full`` adds the CPU leg (and,
after an INNER workload, the general-form / end-to-end / copy-probe legs), and its parity checks hold."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("general_form", "t_e2e_ms", "measured_copy_GBps")


def bench_line(*argv):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "bench.py"), *argv]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("workload", ["cfg2_sparse_1Mx1M_1chrom", "cfg3_count_1Mx10M_24chrom"])
def test_plain_and_full_runs(workload):
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", workload]
    plain = bench_line(*args)
    full = bench_line(*args, "--full")
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k]
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["cpu_baseline"] is None and not any(k in plain for k in EXTRAS)
    parity = full["cpu_baseline"]["parity"]
    assert parity and all(v is not False for v in parity.values())
    if workload.startswith("cfg2"):
        assert plain["config"]["pairs_per_step"] == full["config"]["pairs_per_step"] > 0
        assert parity["pairs_equal"] and parity["multiset_checksum_equal"]
        g = full["general_form"]
        assert g["pairs_equal_default_form"] and g["checksum_equal_default_form"]
        assert all(full["t_e2e_parity"].values())
    else:
        assert parity["equal"] and not any(k in full for k in EXTRAS)
