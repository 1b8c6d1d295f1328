"""Workspace sizes and the scratch helper, without a GPU.

The ``*_workspace_bytes`` queries that answer without a device are pinned to the values the library gave before the
workspace layouts moved onto the shared carver of csrc/dva_common.h (measured on a build of that commit, not computed
from the code under test): a layout that pads, orders or sizes a region differently shows up here.  The queries that
ask rocPRIM for temporary storage need a device and are compared on one.  ``_lib.workspace`` is the one place the
Python side turns a query into a scratch tensor."""
import pytest
import torch

from deepviewagg_amd import _lib

F32, BF16 = _lib.DVA_F32, _lib.DVA_BF16

PINNED = [
    ("dva_radius_query_workspace_bytes", (0, 0), 256),
    ("dva_radius_query_workspace_bytes", (513, 1), 512),
    ("dva_radius_query_workspace_bytes", (1000, 7), 512),
    ("dva_radius_query_workspace_bytes", (1 << 20, 64), 528384),
    ("dva_mapping_merge_workspace_bytes", (4, 8, 8), 448),
    ("dva_mapping_merge_workspace_bytes", (100, 300, 900), 12608),
    ("dva_mapping_merge_workspace_bytes", (5000, 20000, 70000), 864032),
    ("dva_elastic_workspace_bytes", (5, 6, 7), 5120),
    ("dva_elastic_workspace_bytes", (22, 17, 15), 134656),
    ("dva_vote_workspace_bytes", (1,), 256),
    ("dva_vote_workspace_bytes", (1000,), 4096),
    ("dva_vote_workspace_bytes", (1 << 20,), 4194304),
    ("dva_voxel_parent_workspace_bytes", (1,), 256),
    ("dva_voxel_parent_workspace_bytes", (1000,), 8192),
    ("dva_voxel_parent_workspace_bytes", (300000,), 4194304),
    ("dva_image_tail_workspace_bytes", (0,), 256),
    ("dva_image_tail_workspace_bytes", (3,), 256),
    ("dva_image_tail_workspace_bytes", (33,), 512),
    ("dva_minmax3_workspace_bytes", (), 6144),
    ("dva_seg_nll_workspace_bytes", (), 16384),
    ("dva_sparse_conv_workspace_bytes", (27, 16, 16, F32), 442368),
    ("dva_sparse_conv_workspace_bytes", (27, 32, 64, BF16), 221184),
    ("dva_sparse_conv_workspace_bytes", (8, 64, 128, BF16), 131072),
]


@pytest.mark.parametrize("query,args,expected", PINNED, ids=[f"{q[4:-16]}{a}" for q, a, _ in PINNED])
def test_workspace_sizes_are_the_ones_before_the_carver(query, args, expected):
    assert getattr(_lib.load(), query)(*args) == expected
    assert _lib.workspace_bytes(query, *args) == expected


def test_workspace_allocates_what_the_query_answers():
    ws, nbytes = _lib.workspace("dva_elastic_workspace_bytes", "cpu", 5, 6, 7)
    assert nbytes == 5120
    assert ws.dtype == torch.uint8 and ws.shape == (5120,) and ws.device.type == "cpu"
    ws, nbytes = _lib.workspace("dva_minmax3_workspace_bytes", "cpu")
    assert nbytes == 6144 and ws.numel() == 6144


@pytest.mark.parametrize("args,code", [((0, 3, 3), -1), ((1 << 12, 1 << 12, 1 << 6), -2)])
def test_workspace_raises_on_a_refused_query_before_it_allocates(monkeypatch, args, code):
    made = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append((a, k)) or real_empty(*a, **k))
    with pytest.raises(_lib.DvaError) as err:
        _lib.workspace("dva_elastic_workspace_bytes", "cpu", *args)
    assert err.value.code == code
    message = str(err.value)
    assert "dva_elastic_workspace_bytes" in message
    assert "(" + ", ".join(str(a) for a in args) + ")" in message
    assert made == []
    with pytest.raises(_lib.DvaError) as err:
        _lib.workspace_bytes("dva_elastic_workspace_bytes", *args)
    assert err.value.code == code
