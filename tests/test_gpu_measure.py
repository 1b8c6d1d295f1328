"""tools/measure.py on the device: the three windows, what ``profile_once`` counts, and the head of a record."""
import math
import os
import sys

import pytest
import torch

from conftest import ROOT
from deepviewagg_amd import _lib, ops

sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 1 << 20


@pytest.fixture
def x():
    return torch.zeros(N, device=DEV)


def _good(ms):
    return math.isfinite(ms) and ms > 0


def test_windows_return_positive_ms_per_call(x):
    assert _good(measure.event_window(lambda: x.add_(1), 8))
    assert _good(measure.host_window(lambda: x.add_(1), 8))
    host, device = measure.both_window(lambda: x.add_(1), 8)
    assert _good(host) and _good(device)
    assert float(x[0]) == 24                             # inner calls each, nothing else


def test_profile_once_counts_ops_launches_and_syncs(x):
    got = measure.profile_once(lambda: (x + 1) * 2)
    assert (got["torch_ops"], got["dva_launches"], got["syncs"]) == (2, 0, 0) and got["peak_bytes"] >= 4 * N
    # the readback is the one synchronising operation: this pins what the sync counter lets through
    got = measure.profile_once(lambda: ((x + 1) * 2).sum().item())
    assert got["syncs"] == 1 and got["dva_launches"] == 0


def test_profile_once_counts_a_call_into_the_library():
    V = 1024
    packed = ops.pack_gather_index(torch.randint(0, 2, (V,)).to(DEV), torch.arange(V + 1).to(DEV),
                                   torch.stack([torch.randint(0, 32, (V,)), torch.randint(0, 16, (V,))], 1).to(DEV))
    assert measure.profile_once(lambda: ops.gather_row_index(packed, 2, 16, 32))["dva_launches"] == 1


def test_profile_once_reports_the_peak_above_what_was_resident(x):
    def allocate_and_drop():
        torch.empty(4 << 20, dtype=torch.uint8, device=DEV)
    assert measure.profile_once(allocate_and_drop)["peak_bytes"] >= 4 << 20
    assert measure.peak_bytes(allocate_and_drop) >= 4 << 20


def test_profile_once_leaves_the_timer_it_found(x, monkeypatch):
    sentinel = object()
    monkeypatch.setattr(ops, "TIMER", sentinel)
    measure.profile_once(lambda: x + 1)
    assert ops.TIMER is sentinel

    def fails():
        raise RuntimeError("inside the profiled call")
    with pytest.raises(RuntimeError, match="inside the profiled call"):
        measure.profile_once(fails)
    assert ops.TIMER is sentinel


def test_header_names_the_build():
    head = measure.header("x", reps=3)
    assert set(head) == {"tool", "device", "dva_version", "source_sha256", "reps"}
    assert head["tool"] == "x" and head["reps"] == 3 and head["device"] == torch.cuda.get_device_name(0)
    assert head["dva_version"] == _lib.load().dva_version() and head["source_sha256"] == _lib.source_sha256()
