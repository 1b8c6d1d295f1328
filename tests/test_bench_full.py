"""A plain `bench.py` run takes only what its headline line needs; `--full` adds every other measurement after the timed
steps (PMC passes, copy ceiling, gather / mapping build / K-NN, secondary workloads, CPU baselines).  The GPU runs use a
small scene (2^14 points): the secondary workloads and the PMC passes belong to the default workload and stay off in both."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRAS = ("gather", "mapping_build", "neighborhood_features", "cpu_baseline")


def _run(tmp_path, *extra):
    detail = tmp_path / "detail.json"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--log2-points", "14",
                        "--detail-file", str(detail), *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    with open(detail) as f:
        return json.loads(lines[0]), json.load(f)


def test_full_is_an_option():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout


@pytest.mark.gpu
def test_plain_run_takes_only_the_headline(tmp_path):
    line, detail = _run(tmp_path)
    for k in CONTRACT:
        assert line[k] is not None, k
    assert line["steps"] == 2 and line["warmup"] == 1
    assert not [k for k in EXTRAS + ("workloads",) if k in detail]
    assert detail["hbm_copy_GBps"] is None and "copy_ceiling" not in detail["roofline"]
    assert detail["pmc_live"] == {"skipped": "run with --full only"}
    assert "cpu_baseline" not in line and "mapping_build_images_per_s" not in line


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements(tmp_path):
    line, detail = _run(tmp_path, "--full")
    for k in CONTRACT:
        assert line[k] is not None, k
    assert all(k in detail for k in EXTRAS), [k for k in EXTRAS if k not in detail]
    assert "error" not in detail["cpu_baseline"], detail["cpu_baseline"]
    assert detail["hbm_copy_GBps"] > 0 and detail["roofline"]["frac_of_copy_ceiling"] > 0
    assert detail["mapping_build"]["indices_bit_exact_vs_oracle"]
    assert "cpu_baseline" in line and "mapping_build_images_per_s" in line
