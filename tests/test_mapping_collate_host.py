"""Without a GPU: the numpy restatement of the mapping collation (tests/mapping_collate_ref.py) against the kept torch
composition (``CSRBatch.from_csr_list`` + ``insert_empty_groups``) on CPU mappings, the argument checks of the C entry
``dva_mapping_collate``, and ``MMData`` / ``MMBatch`` / ``collate_data`` on CPU data."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import t
from mapping_collate_ref import (GROUP, cases, collate_reference, cpu_mapping, mappings_equal, sample, settings_equal,
                                 three_samples)

from deepviewagg_amd import _lib

CASES = cases()
NAMES = sorted(CASES)


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def test_the_case_list_covers_the_launch_groups():
    assert GROUP == _lib.load().dva_mapping_collate_group_items()
    assert f"b{GROUP + 1}" in CASES and f"b{2 * GROUP + 1}" in CASES
    assert len(CASES[f"b{2 * GROUP + 1}"]["items"]) == 2 * GROUP + 1


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_cpu_composition(name):
    from deepviewagg_amd.core.multimodal.csr import CSRBatch
    from deepviewagg_amd.core.multimodal.image import ImageMapping, ImageMappingBatch
    case = CASES[name]
    ref = collate_reference(case["items"], case["point_bases"], case["num_points"])
    maps = [cpu_mapping(a) for a in case["items"]]
    batch = ImageMappingBatch.from_csr_list(maps, group_bases=case["point_bases"], num_groups=case["num_points"])
    assert type(batch) is ImageMappingBatch and type(batch.values[1]) is CSRBatch
    assert batch.__csr_type__ is ImageMapping
    assert batch.__sizes__.tolist() == [a[0].shape[0] - 1 for a in case["items"]]
    assert batch.values[1].__sizes__.tolist() == [a[1].shape[0] for a in case["items"]]
    assert np.array_equal(batch.pointers.numpy(), ref["pointers"])
    assert np.array_equal(batch.images.numpy(), ref["images"])
    assert np.array_equal(batch.values[1].pointers.numpy(), ref["atom_ptr"])
    assert batch.pixels.dtype == torch.int16 and np.array_equal(batch.pixels.numpy(), ref["pixels"])
    assert batch.has_features == (ref["features"] is not None)
    if batch.has_features:
        got = batch.features.numpy()
        assert got.shape == ref["features"].shape and np.array_equal(bits(got), bits(ref["features"]))
    # what the composition has without bases is what it has always been: from_csr_list alone
    if case["point_bases"] is None:
        plain = ImageMappingBatch._from_csr_list_composition(maps)
        assert torch.equal(plain.pointers, batch.pointers) and torch.equal(plain.images, batch.images)


def test_restatement_by_hand():
    a = (np.array([0, 2, 2, 3]), np.array([1, 0, 1]), np.array([0, 1, 3, 3]),
         np.array([[1, 2], [3, 4], [5, 6]], dtype=np.int16), None)
    b = (np.array([0, 0, 1]), np.array([4]), np.array([0, 2]), np.array([[7, 8], [9, 10]], dtype=np.int16), None)
    a, b = [tuple(x.astype(np.int64) if i < 3 else x for i, x in enumerate(m)) for m in (a, b)]
    ref = collate_reference([a, b], point_bases=[1, 5], num_points=9)
    assert ref["pointers"].tolist() == [0, 0, 2, 2, 3, 3, 3, 4, 4, 4]
    assert ref["images"].tolist() == [1, 0, 1, 6] and ref["image_offsets"].tolist() == [0, 2]
    assert ref["atom_ptr"].tolist() == [0, 1, 3, 3, 5]
    assert ref["pixels"].tolist() == [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10]]


def test_num_groups_below_the_top_is_raised_to_it():
    from deepviewagg_amd.core.multimodal.image import ImageMappingBatch
    maps = [cpu_mapping(a) for a in CASES["gap_between"]["items"]]
    got = ImageMappingBatch.from_csr_list(maps, group_bases=[1, 6, 11], num_groups=4)
    ref = collate_reference(CASES["gap_between"]["items"], [1, 6, 11], 4)
    assert got.num_groups == 16 and np.array_equal(got.pointers.numpy(), ref["pointers"])


# ---------------------------------------------------------------------------------------------------------------
# the C entry
# ---------------------------------------------------------------------------------------------------------------

def descriptors(rows, good=0x1000):
    """Items with made-up non-null addresses: the checks run before any HIP call and never follow them."""
    arr = (_lib.DvaCollateItem * len(rows))()
    for d, (n, v, a, base) in zip(arr, rows):
        d.pointers, d.images, d.atom_ptr, d.pixels, d.features = good, good, good, good, None
        d.n_points, d.n_views, d.n_atoms, d.point_base = n, v, a, base
    return arr


def call(lib, items, n_items, n, v, a, pixel_bytes=2, F=0, outs=(0x1000,) * 4, ws=0x1000, ws_bytes=1 << 20):
    p = lambda x: ctypes.c_void_p(x) if x else None
    return lib.dva_mapping_collate(items, n_items, pixel_bytes, F, n, v, a, p(outs[0]), p(outs[1]), p(outs[2]),
                                   p(outs[3]), None, None, p(ws), ws_bytes, None)


def test_abi_entries_and_argument_checks_without_a_device():
    lib = _lib.load()
    assert lib.dva_version() >= 324
    assert lib.dva_mapping_collate_group_items() == 32
    assert lib.dva_mapping_collate_workspace_bytes(0) == -1 and lib.dva_mapping_collate_workspace_bytes(-3) == -1
    small, big = lib.dva_mapping_collate_workspace_bytes(1), lib.dva_mapping_collate_workspace_bytes(65)
    assert 0 < small < big < (1 << 20)
    assert ctypes.sizeof(_lib.DvaCollateItem) == 5 * 8 + 4 * 8
    two = [(3, 4, 5, 0), (2, 1, 1, 3)]
    ok = descriptors(two)
    assert call(lib, None, 2, 5, 5, 6) == -1                                   # null items
    assert call(lib, ok, 0, 5, 5, 6) == -1 and call(lib, ok, -1, 5, 5, 6) == -1  # n_items < 1
    assert call(lib, ok, 2, 5, 5, 6, outs=(0, 0x1000, 0x1000, 0x1000)) == -1   # null outputs
    assert call(lib, ok, 2, 5, 5, 6, outs=(0x1000, 0, 0x1000, 0x1000)) == -1
    assert call(lib, ok, 2, 5, 5, 6, outs=(0x1000, 0x1000, 0, 0x1000)) == -1
    assert call(lib, ok, 2, 5, 5, 6, outs=(0x1000, 0x1000, 0x1000, 0)) == -1
    assert call(lib, ok, 2, 5, 5, 6, ws=0) == -1                               # null workspace
    assert call(lib, ok, 2, 5, 5, 6, ws_bytes=8) == -1                         # workspace too small
    assert call(lib, ok, 2, -1, 5, 6) == -1                                    # negative sizes
    assert call(lib, descriptors([(3, -4, 5, 0), (2, 1, 1, 3)]), 2, 5, 5, 6) == -1
    assert call(lib, descriptors([(3, 4, 5, 4), (2, 1, 1, 0)]), 2, 9, 5, 6) == -1   # bases descend
    assert call(lib, descriptors([(3, 4, 5, 0), (2, 1, 1, 2)]), 2, 5, 5, 6) == -1   # items overlap
    assert call(lib, ok, 2, 4, 5, 6) == -1                                     # the last item ends behind the total
    assert call(lib, ok, 2, 5, 6, 6) == -1 and call(lib, ok, 2, 5, 5, 7) == -1  # totals that do not add up
    assert call(lib, ok, 2, 5, 4, 6) == -1 and call(lib, ok, 2, 5, 5, 5) == -1
    assert call(lib, ok, 2, 5, 5, 6, F=3) == -1                                # features announced, none given
    for pixel_bytes in (1, 4, 8):
        assert call(lib, ok, 2, 5, 5, 6, pixel_bytes=pixel_bytes) == -2
    top = 2 ** 31 - 1
    assert call(lib, descriptors([(top, 0, 0, 0)]), 1, top, 0, 0) == -2        # totals at or above 2^31 - 1
    assert call(lib, descriptors([(1, top, 0, 0)]), 1, 1, top, 0) == -2
    assert call(lib, descriptors([(1, 0, top, 0)]), 1, 1, 0, top) == -2
    assert call(lib, ok, 2, top, 5, 6) == -2


def test_op_refuses_cpu_tensors():
    from deepviewagg_amd import ops
    a = CASES["b1"]["items"][0]
    with pytest.raises(_lib.DvaError):
        ops.collate_mapping([tuple(None if x is None else t(x) for x in a)])


# ---------------------------------------------------------------------------------------------------------------
# MMData, MMBatch, collate_data
# ---------------------------------------------------------------------------------------------------------------

def test_mm_data_construction_checks():
    from deepviewagg_amd.core.multimodal.data import MODALITY_FORMATS, MODALITY_NAMES, MMData
    from deepviewagg_amd.core.multimodal.image import ImageData
    assert MODALITY_NAMES == ["image"] and MODALITY_FORMATS["image"] is ImageData
    mm = sample(0, 6)
    assert mm.num_points == len(mm) == 6 and mm.num_node_features == 5 and mm.device == torch.device("cpu")
    assert mm.pos is mm.data.pos and mm.mapping_index is mm.data.mapping_index and mm.grid_size == 0.05
    assert set(mm.modalities) == {"image"} and "MMData" in repr(mm)
    images = mm.modalities["image"]
    with pytest.raises(AssertionError):                   # no mapping key
        MMData(SimpleNamespace(pos=mm.pos), image=images)
    with pytest.raises(AssertionError):                   # mapping indices that are not 0 .. n - 1
        MMData(SimpleNamespace(pos=mm.pos, mapping_index=torch.tensor([0, 1, 2, 3, 4, 6])), image=images)
    with pytest.raises(AssertionError):                   # an unknown modality
        MMData(mm.data, lidar=images)
    with pytest.raises(AssertionError):                   # a modality of the wrong type
        MMData(mm.data, image=images[0])
    with pytest.raises(AssertionError):                   # mappings over another number of points
        MMData(SimpleNamespace(pos=mm.pos[:5], mapping_index=torch.arange(5)), image=images)
    with pytest.raises(AssertionError):
        MMData([mm.pos], image=images)
    clone = mm.clone()
    assert clone.data is not mm.data and torch.equal(clone.pos, mm.pos) and clone.pos is not mm.pos
    assert mm.to("cpu").num_points == 6


@pytest.mark.parametrize("container", [SimpleNamespace, dict])
def test_mm_data_getitem_equals_a_manual_pick(container):
    mm = sample(1, 9, container=container)
    idx = torch.tensor([7, 0, 3, 4])
    got = mm[idx]
    assert type(got).__name__ == "MMData" and got.num_points == 4
    assert torch.equal(got.pos, mm.pos[idx]) and torch.equal(got.x, mm.x[idx]) and torch.equal(got.y, mm.y[idx])
    assert torch.equal(got.mapping_index, torch.arange(4))
    assert torch.equal(got.centre, mm.centre) and got.scene == mm.scene
    want = mm.modalities["image"].select_points(idx, mode='pick')
    for a, b in zip(got.modalities["image"], want):
        settings_equal(a, b)
    assert torch.equal(mm.mapping_index, torch.arange(9))          # the source is untouched
    # a bool mask and a slice index the same way
    mask = torch.zeros(9, dtype=torch.bool)
    mask[[0, 3, 4]] = True
    assert torch.equal(mm[mask].pos, mm.pos[mask]) and torch.equal(mm[slice(2, 5)].pos, mm.pos[2:5])


@pytest.mark.parametrize("container", [SimpleNamespace, dict])
def test_from_mm_data_list_equals_the_manual_composition(container):
    from deepviewagg_amd.core.multimodal.data import MMBatch, collate_data
    from deepviewagg_amd.core.multimodal.image import ImageBatch
    items = three_samples(container)
    batch = MMBatch.from_mm_data_list(items)
    assert isinstance(batch, MMBatch) and batch.num_points == 17 and batch.num_batch_items == 3
    assert batch.batch_items_sizes.tolist() == [6, 4, 7] and batch.batch_pointers.tolist() == [0, 6, 10, 17]
    data = collate_data([mm.data for mm in items])
    get = (lambda d, k: d[k]) if container is dict else getattr
    for key in ("pos", "x", "y", "centre"):
        assert torch.equal(getattr(batch, key), get(data, key))
        assert torch.equal(getattr(batch, key), torch.cat([getattr(mm, key) for mm in items]))
    # the point index of every sample is offset by the points in front of it
    assert torch.equal(batch.mapping_index, torch.arange(17))
    assert torch.equal(batch.batch, torch.tensor([0] * 6 + [1] * 4 + [2] * 7)) and batch.batch.dtype == torch.int64
    assert torch.equal(batch.grid_size, torch.tensor([0.05] * 3, dtype=torch.float64)) and batch.scene == ["scene2", "scene3", "scene4"]
    want = ImageBatch.from_data_list([mm.modalities["image"] for mm in items])
    got = batch.modalities["image"]
    assert isinstance(got, ImageBatch) and len(got) == len(want) == 2 and got.num_points == 17
    for a, b in zip(got, want):
        settings_equal(a, b)
    # the second setting is missing from the second sample: its points are empty groups
    second = got[1].mappings
    assert second.num_groups == 17 and torch.all(second.pointers[6:11] == second.pointers[6])
    m0, m2 = items[0].modalities["image"][1].mappings, items[2].modalities["image"][1].mappings
    assert torch.equal(second.pointers[:7], m0.pointers)
    assert torch.equal(second.pointers[10:], m2.pointers + m0.num_views)
    assert second.__sizes__.tolist() == [6, 7]


def test_image_batch_equals_the_parent_composition():
    """ImageBatch.from_data_list with the bases forwarded == stacking first, inserting the empty groups afterwards."""
    from deepviewagg_amd.core.multimodal.image import ImageBatch, ImageMappingBatch
    items = [mm.modalities["image"] for mm in three_samples()]
    got = ImageBatch.from_data_list(items)
    first = ImageMappingBatch._from_csr_list_composition([il[0].mappings for il in items])
    assert torch.equal(got[0].mappings.pointers, first.pointers) and torch.equal(got[0].mappings.images, first.images)
    second = ImageMappingBatch._from_csr_list_composition([items[0][1].mappings, items[2][1].mappings])
    second.insert_empty_groups(torch.cat([torch.arange(0, 6), torch.arange(10, 17)]), num_groups=17)
    mappings_equal(got[1].mappings, second)


@pytest.mark.parametrize("container", [SimpleNamespace, dict])
def test_to_mm_data_list_returns_the_inputs(container):
    from deepviewagg_amd.core.multimodal.data import MMBatch, MMData
    items = three_samples(container)
    batch = MMBatch.from_mm_data_list(items)
    back = batch.to_mm_data_list()
    assert len(back) == 3
    for a, b in zip(items, back):
        assert type(b) is MMData and type(b.data) is type(a.data) and b.num_points == a.num_points
        for key in ("pos", "x", "y", "mapping_index", "centre"):
            assert torch.equal(getattr(a, key), getattr(b, key)), key
        assert b.grid_size == a.grid_size and b.scene == a.scene and not hasattr(b, "batch")
        assert len(a.modalities["image"]) == len(b.modalities["image"])
        for sa, sb in zip(a.modalities["image"], b.modalities["image"]):
            settings_equal(sa, sb)
    clone = batch.clone()
    assert isinstance(clone, MMBatch) and clone.batch_items_sizes.tolist() == [6, 4, 7]
    with pytest.raises(RuntimeError):
        MMBatch(batch.data, **batch.modalities).to_mm_data_list()


def test_dropin_resolves_the_data_module():
    import importlib
    import sys
    from deepviewagg_amd import dropin
    from deepviewagg_amd.core.multimodal import data
    before = {k for k in sys.modules if k.startswith("torch_points3d")}
    try:
        dropin.install(patch_existing=False)
        mod = importlib.import_module("torch_points3d.core.multimodal.data")
        assert mod.MMBatch is data.MMBatch and mod.MMData is data.MMData and mod.MODALITY_NAMES == ["image"]
    finally:
        for k in [k for k in sys.modules if k.startswith("torch_points3d") and k not in before]:
            del sys.modules[k]
