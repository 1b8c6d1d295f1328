"""tools/measure.py without a device: the loop that alternates the arms (with an injected window), the summaries, the
record writer, and the structure of the sixteen side benchmarks that are built on it."""
import glob
import importlib
import json
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402

TOOLS = ("cloud_augment", "elastic_distortion", "full_res_vote", "grid_sampling", "image_load", "image_pick",
         "image_tail", "image_window", "mapping_collate", "mapping_merge", "mapping_select", "no3d_tail",
         "pointwise_pca", "radius_sampling", "seg_loss", "view_pool")
# these two keep the timing helpers they had: rebuilt on measure.py, host-clock rows of theirs left the margin of the
# parent's figures with no cause found (profiles/measure_unify_ab.json); they use header() and emit() like the rest
OWN_CLOCKS = ("elastic_distortion", "full_res_vote")


class Script:
    """Arms that log their calls, and a fake window that logs (name, inner) and returns scripted milliseconds."""

    def __init__(self, names, ms=1.0):
        self.log = []
        self.in_window = False
        self.ms = ms
        self.arms = {name: self._arm(name) for name in names}
        self.names = {fn: name for name, fn in self.arms.items()}

    def _arm(self, name):
        return lambda: self.log.append(("call", name))

    def window(self, fn, inner):
        self.in_window = True
        self.log.append(("window", self.names[fn], inner))
        self.in_window = False
        return self.ms[self.names[fn]] if isinstance(self.ms, dict) else self.ms

    def before(self, name, rep):
        assert not self.in_window
        self.log.append(("before", name, rep))

    def windows(self):
        return [e[1:] for e in self.log if e[0] == "window"]


def test_alternate_warms_every_arm_first_and_alternates_in_the_order_given():
    s = Script("AB")
    ms, inner = measure.alternate(s.arms, 3, s.window, warmup=2)
    first = s.log.index(("window", "A", 1))
    assert s.log[:first] == [("call", "A")] * 2 + [("call", "B")] * 2
    assert s.windows() == [("A", 1), ("B", 1)] * 3
    assert ms == {"A": [1.0] * 3, "B": [1.0] * 3} and inner == {"A": 1, "B": 1}


def test_alternate_cap_stops_that_arm_only():
    s = Script("AB", ms={"A": 2.0, "B": 5.0})
    ms, _ = measure.alternate(s.arms, 4, s.window, caps={"B": 1})
    assert s.windows() == [("A", 1), ("B", 1), ("A", 1), ("A", 1), ("A", 1)]
    assert ms == {"A": [2.0] * 4, "B": [5.0]}


def test_alternate_takes_a_window_and_a_warmup_per_arm():
    s, other = Script("AB"), []
    ms, _ = measure.alternate(s.arms, 2, {"A": s.window, "B": lambda fn, inner: other.append(inner) or 7.0},
                              warmup={"A": 1, "B": 0})
    assert s.log.count(("call", "A")) == 1 and ("call", "B") not in s.log
    assert ms == {"A": [1.0, 1.0], "B": [7.0, 7.0]} and other == [1, 1]


@pytest.mark.parametrize("probe", [0.01, 1.0, 1000.0])
def test_alternate_calibrates_inner_from_a_probe_window(probe):
    s = Script("AB", ms={"A": probe, "B": 2 * probe})
    _, inner = measure.alternate(s.arms, 2, s.window, seconds=0.25)
    assert inner == {"A": max(1, int(0.25 * 1e3 / probe)), "B": max(1, int(0.25 * 1e3 / (2 * probe)))}
    assert {0.01: 25000, 1.0: 250, 1000.0: 1}[probe] == inner["A"]
    # one probe window per arm, after its warm-up and before any timed window; the timed windows use the result
    assert s.windows() == [("A", 1), ("B", 1)] + [("A", inner["A"]), ("B", inner["B"])] * 2


def test_alternate_calls_before_once_per_timed_window_outside_it():
    s = Script("AB")
    measure.alternate(s.arms, 3, s.window, warmup=2, before=s.before)
    timed = [e for e in s.log if e[0] == "before" and e[2] is not None]
    assert timed == [("before", n, r) for r in range(3) for n in "AB"]
    for e in timed:                                     # directly in front of its window
        assert s.log[s.log.index(e) + 1] == ("window", e[1], 1)
    # in the warm-up it runs before every call, without a repetition
    assert [e for e in s.log if e[0] == "before" and e[2] is None] == [("before", n, None) for n in "AABB"]


def test_repeated_is_alternate_with_one_arm():
    s = Script("A", ms=3.0)
    assert measure.repeated(s.arms["A"], 4, s.window, warmup=2) == [3.0] * 4
    assert s.log.count(("call", "A")) == 2 and s.windows() == [("A", 1)] * 4


def test_summarise():
    assert measure.summarise([3, 1, 2], 3) == {"median": 2, "min": 1, "max": 3, "spread": 2}
    assert measure.summarise([4, 1, 3, 2], 3) == {"median": 2.5, "min": 1, "max": 4, "spread": 3}
    assert measure.summarise([1.2347, 1.2341], 3) == {"median": 1.234, "min": 1.234, "max": 1.235, "spread": 0.001}
    assert measure.summarise([0.12345], 2) == {"median": 0.12, "min": 0.12, "max": 0.12, "spread": 0}
    with pytest.raises(ValueError):
        measure.summarise([], 3)


def test_ranges_overlap():
    assert not measure.ranges_overlap((1, 2), (3, 4)) and not measure.ranges_overlap((3, 4), (1, 2))
    assert measure.ranges_overlap((1, 2), (2, 3)) and measure.ranges_overlap((2, 3), (1, 2))
    assert measure.ranges_overlap((1, 4), (2, 3)) and measure.ranges_overlap((2, 3), (1, 4))


def test_emit_writes_one_line_into_a_new_directory(tmp_path, capsys):
    result = {"tool": "x", "rows": [{"ms": 1.5, "ok": True}], "none": None}
    out = tmp_path / "new" / "deeper" / "record.json"
    measure.emit(result, str(out))
    text = out.read_text()
    assert text.endswith("\n") and text.count("\n") == 1 and json.loads(text) == result
    assert json.loads(capsys.readouterr().out) == result
    measure.emit(result)                                # no file asked for: stdout alone
    assert json.loads(capsys.readouterr().out) == result


def test_the_benchmarks_leave_clocks_and_counters_to_measure():
    paths = sorted(glob.glob(os.path.join(ROOT, "tools", "*_bench.py")))
    assert {os.path.basename(p)[:-len("_bench.py")] for p in paths} >= set(TOOLS)
    for path in paths:
        text = open(path).read()
        name = os.path.basename(path)
        if name[:-len("_bench.py")] in set(TOOLS) - set(OWN_CLOCKS):    # scripts without a main() keep their own too
            for word in ("torch.cuda.Event(", "perf_counter", "set_sync_debug_mode", "reset_peak_memory_stats",
                         "TorchDispatchMode"):
                assert word not in text, f"{name} has {word} of its own"
        imports = re.findall(r"^\s*(?:from|import)\s+([\w.]+)", text, re.M)
        assert not [m for m in imports if m.endswith("_bench")], f"{name} imports another benchmark"


@pytest.mark.parametrize("tool", TOOLS)
def test_tool_imports_and_prints_its_help_without_a_device(tool, capsys):
    import torch
    module = importlib.import_module(tool + "_bench")
    with pytest.raises(SystemExit) as stop:
        module.main(["--help"])
    assert stop.value.code == 0 and "--reps" in capsys.readouterr().out
    assert not torch.cuda.is_initialized()
