"""bench.py's byte accounting and launch plumbing -- CPU only (no GPU call is made here)."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_sort_bytes_model_by_hand():
    # cfg 4, fixed-length B sorted from its raw columns, three-stage sort for the 100M-row side:
    # B: KEYGEN pass 8 + 8 B/row, second pass 8 + 8, bucket sort 8 + 8; A (key, end, rid), four passes:
    # 8 in + 12 out, then 3 x (12 + 12)
    sc, lo = bench.sort_bytes_model([(10_000_000, 2, False), (100_000_000, 1, True)])
    assert sc == 2 * 16 * 100_000_000 + (20 + 3 * 24) * 10_000_000 == 4_120_000_000
    assert lo == 16 * 100_000_000
    # below 32M rows: four passes, first one reads no row ids; keys only: 8 B/row/pass
    sc, lo = bench.sort_bytes_model([(10_000_000, 0, False), (1_000_000, 2, False)])
    assert sc == 4 * 8 * 10_000_000 + (20 + 3 * 24) * 1_000_000 and lo == 0


def test_phase_bytes_agree_with_the_committed_pmc_run():
    """the bench's algorithmic bytes must follow the code -- within 10 % of what the
    counters saw for the sort, and never above the measured traffic for any phase."""
    t = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    pmc = t["cfg4_10Mx100M_24chrom"]["uniform_b"]
    # (round 3: the settled form of the one-call join writes its pairs from the bucket stage -- no fill phase; the
    # query side is sorted from its raw columns in two passes: 12 + 12 B/row, then 12 + 12)
    alg = bench.inner_phase_bytes(10_000_000, 100_000_000, 404_376_266, "uniform_b", True, bucket_join=True)
    alg["sort_scatter"] = 2 * 16 * 100_000_000 + 2 * 24 * 10_000_000
    assert abs(alg["sort_scatter"] - pmc["sort_scatter"]) / pmc["sort_scatter"] < 0.15
    assert abs(alg["sort_local"] - pmc["sort_local"]) / pmc["sort_local"] < 0.10
    assert alg["span"] <= pmc["span"] * 1.02
    assert "fill" not in pmc and alg["fill"] == 0
    assert "csrc_hash" in t and "commit" in t


def test_pmc_traffic_is_withheld_when_the_kernel_sources_changed(monkeypatch):
    import json as _json

    stamped = _json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    # collected on exactly these sources: the figure is handed out, per launch; on any other sources: withheld
    monkeypatch.setattr(bench, "csrc_hash", lambda: stamped["csrc_hash"])
    per_launch = bench.pmc_traffic("cfg4_10Mx100M_24chrom", "uniform_b", "sort_scatter", 4)
    assert per_launch == round(stamped["cfg4_10Mx100M_24chrom"]["uniform_b"]["sort_scatter"] / 4)
    assert bench.pmc_traffic("cfg4_10Mx100M_24chrom", "no_such_form", "sort_scatter", 4) is None
    monkeypatch.setattr(bench, "csrc_hash", lambda: "0" * 16)
    assert bench.pmc_traffic("cfg4_10Mx100M_24chrom", "uniform_b", "sort_scatter", 4) is None


def test_operator_bytes_follow_survey_8d():
    assert bench.op_bytes("inner", 10, 20, 5) == 12 * 30 + 8 * 5
    assert bench.op_bytes("semi", 10, 20, 5) == 12 * 30 + 4 * 5
    assert bench.op_bytes("count", 10, 20, 0) == 12 * 30 + 8 * 10
    assert bench.op_bytes("nearest", 10, 20, 0) == 12 * 30 + 8 * 10


def test_gpus_n_starts_the_ranks_as_a_child_process(monkeypatch):
    """`python bench.py --gpus N` outside torch.distributed.run must launch the ranks itself (and not
    exec): the command line, and that a rank (WORLD_SIZE set) does not launch again."""
    calls = []

    class Done(Exception):
        pass

    def fake_run(cmd, env=None):
        calls.append((cmd, env))

        class R:
            returncode = 7
        return R()

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    args = bench.parse_args()
    with pytest.raises(SystemExit) as ei:
        bench.self_launch(args)
    assert ei.value.code == 7
    cmd, env = calls[0]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert "127.0.0.1" in cmd and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    monkeypatch.setenv("WORLD_SIZE", "4")
    bench.self_launch(args)          # a rank: returns without launching
    assert len(calls) == 1
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    bench.self_launch(bench.parse_args())   # N = 1: nothing to launch
    assert len(calls) == 1


def test_steps_and_warmup_are_checked(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "0"])
    args = bench.parse_args()
    assert args.steps == 7 and args.warmup == 0 and args.dump_outputs is None
    for argv in (["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--exchange", "none", "--dump-outputs", "d"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        with pytest.raises(SystemExit):
            bench.parse_args()


def test_only_full_runs_the_legs_after_the_timed_region(monkeypatch):
    def parsed(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
        a = bench.parse_args()
        return a.full, a.no_cpu_baseline, a.no_extras, a.verify

    # a plain run: no CPU leg, no extras, no verification of a gathered result unless asked for by name
    assert parsed("--gpus", "1", "--steps", "3", "--warmup", "1") == (False, True, True, False)
    assert parsed("--gpus", "2") == (False, True, True, False)
    assert parsed("--force-exchange") == (False, True, True, False)
    assert parsed("--gpus", "2", "--verify") == (False, True, True, True)
    # --full: every leg, as the switches that leave parts of it out say
    assert parsed("--full") == (True, False, False, False)
    assert parsed("--full", "--no-cpu-baseline") == (True, True, False, False)
    assert parsed("--full", "--no-extras") == (True, False, True, False)
    assert parsed("--full", "--gpus", "2") == (True, False, False, True)
    assert parsed("--full", "--force-exchange") == (True, False, False, True)
    assert parsed("--full", "--gpus", "2", "--no-verify") == (True, False, False, False)


def test_pair_sample_depends_on_the_pairs_not_their_order():
    import numpy as np
    import torch

    rng = np.random.default_rng(11)
    n = 300_000
    a = rng.integers(0, 10_000_000, n).astype(np.int32)
    b = rng.integers(0, 100_000_000, n).astype(np.int32)
    perm = rng.permutation(n)
    sa, sb, shift = bench.pair_sample(torch.from_numpy(a), torch.from_numpy(b), target=1 << 14, chunk=1 << 16)
    pa, pb, shift2 = bench.pair_sample(torch.from_numpy(a[perm]), torch.from_numpy(b[perm]), target=1 << 14, chunk=1 << 15)
    assert shift == shift2 == 5
    assert np.array_equal(sa, pa) and np.array_equal(sb, pb)
    assert 0.5 * (n >> shift) < sa.shape[0] < 1.5 * (n >> shift)
    # the sample is a sub-multiset of the pairs, sorted by (row_a, row_b)
    key = a.astype(np.int64) << 32 | b.astype(np.int64)
    skey = sa << 32 | sb
    assert np.all(np.diff(skey) >= 0) and np.isin(skey, key).all()
    # small outputs are kept whole; the byte budget cuts a sample after sorting
    wa, wb, s0 = bench.pair_sample(torch.from_numpy(a[:1000]), torch.from_numpy(b[:1000]))
    assert s0 == 0 and wa.shape[0] == 1000 and np.array_equal(np.sort(wa), wa)
    ca, _cb, _ = bench.pair_sample(torch.from_numpy(a[:1000]), torch.from_numpy(b[:1000]), budget=16 * 100)
    assert np.array_equal(ca, wa[:100])


def test_dump_outputs_writes_float64_under_the_budget(tmp_path, monkeypatch):
    import numpy as np
    import torch

    ra = torch.tensor([3, 1, 2, 1], dtype=torch.int32)
    rb = torch.tensor([99_999_999, 7, 5, 2], dtype=torch.int32)
    info = bench.dump_outputs(str(tmp_path / "inner"), pairs=(ra, rb))
    got = {k: np.load(tmp_path / "inner" / f"{k}.npy") for k in ("n_pairs", "row_a", "row_b")}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["n_pairs"].tolist() == [4]
    assert got["row_a"].tolist() == [1, 1, 2, 3] and got["row_b"].tolist() == [2, 7, 5, 99_999_999]
    assert info["bytes"] == 8 * 9
    # per-row outputs above the budget: a seeded subset of positions, the same on every run
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 24 * 1000)
    idx = torch.arange(5000, dtype=torch.int32) * 3
    dist = torch.arange(5000, dtype=torch.int64)
    runs = []
    for tag in ("x", "y"):
        info = bench.dump_outputs(str(tmp_path / tag), rows={"row_b": idx, "distance": dist})
        runs.append({k: np.load(tmp_path / tag / f"{k}.npy") for k in ("row_b", "distance", "position")})
        assert info["bytes"] <= 24 * 1000
    pos = runs[0]["position"]
    assert pos.shape[0] == 1000 and np.array_equal(runs[0]["row_b"], pos * 3) and np.array_equal(runs[0]["distance"], pos)
    assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])
