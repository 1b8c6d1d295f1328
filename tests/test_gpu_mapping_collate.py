"""-m gpu: the device collation of mappings (``ops.collate_mapping``, C ABI dva_mapping_collate) behind
``CSRBatch.from_csr_list`` on ImageMappings, ``SameSettingImageBatch`` / ``ImageBatch.from_data_list`` and
``MMBatch.from_mm_data_list``.  Every case is held with ``torch.equal`` on all five tensors and the image offsets to
the numpy restatement (tests/mapping_collate_ref.py) and to the kept torch composition (``COLLATE_ON_DEVICE = False``),
container classes and bookkeeping included; features are compared as bits.  Whole tensors are compared, so an output
element the kernels did not write shows under a poisoned allocator (conftest, DVA_TEST_POISON=1)."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

from conftest import t
from mapping_collate_ref import cases, collate_reference, mappings_equal, settings_equal, three_samples

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = cases()
NAMES = sorted(CASES)
REFS = {}
ENTRY = "dva_mapping_collate"


def reference(name):
    if name not in REFS:
        case = CASES[name]
        REFS[name] = collate_reference(case["items"], case["point_bases"], case["num_points"])
    return REFS[name]


def sliced(a, off):
    """The array on the device; with ``off``, as a slice that starts ``off`` rows into a larger tensor."""
    if a is None:
        return None
    if not off:
        return t(a, DEV)
    junk = np.full((off,) + a.shape[1:], -7, dtype=a.dtype)
    return t(np.concatenate([junk, a]), DEV)[off:]


def device_items(case, pixel_dtype=None, feature_dtype=None):
    offs = case["slice_offsets"] or [0] * len(case["items"])
    out = []
    for arrays, off in zip(case["items"], offs):
        pointers, images, atom_ptr, pixels, feats = (sliced(a, off) for a in arrays)
        if pixel_dtype is not None:
            pixels = pixels.to(pixel_dtype)
        if feature_dtype is not None and feats is not None:
            feats = feats.to(feature_dtype)
        out.append((pointers, images, atom_ptr, pixels, feats))
    return out


def device_mappings(case, **dtypes):
    from deepviewagg_amd.core.multimodal.csr import CSRData
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    out = []
    for pointers, images, atom_ptr, pixels, feats in device_items(case, **dtypes):
        values = [images, CSRData(atom_ptr, pixels, dense=False)] + ([feats] if feats is not None else [])
        out.append(ImageMapping(pointers, *values, dense=False, is_index_value=[True, False, False][:len(values)]))
    return out


@contextlib.contextmanager
def composition_forced():
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    ImageMapping.COLLATE_ON_DEVICE = False
    try:
        yield
    finally:
        ImageMapping.COLLATE_ON_DEVICE = True


@contextlib.contextmanager
def route_calls():
    """Counts the calls of the C entry and of the composition."""
    from deepviewagg_amd import _lib
    from deepviewagg_amd.core.multimodal.csr import CSRBatch
    lib = _lib.load()
    calls = {ENTRY: 0, "composition": 0}
    entry, comp = getattr(lib, ENTRY), CSRBatch._from_csr_list_composition

    def counted_entry(*a):
        calls[ENTRY] += 1
        return entry(*a)

    def counted_comp(csr_list):
        calls["composition"] += 1
        return comp(csr_list)
    setattr(lib, ENTRY, counted_entry)
    CSRBatch._from_csr_list_composition = staticmethod(counted_comp)
    try:
        yield calls
    finally:
        setattr(lib, ENTRY, entry)
        CSRBatch._from_csr_list_composition = staticmethod(comp)


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w)


def bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def same_tensors(a, b):
    """The tensors of two mappings (a round trip is held to the values, not to the container classes)."""
    assert torch.equal(a.pointers, b.pointers) and torch.equal(a.images, b.images)
    assert torch.equal(a.values[1].pointers, b.values[1].pointers) and torch.equal(a.pixels, b.pixels)
    assert a.has_features == b.has_features and (not a.has_features or torch.equal(bits(a.features), bits(b.features)))


def op_equals_reference(out, ref):
    pointers, images, atom_ptr, pixels, features, offsets = out
    for got, key in ((pointers, "pointers"), (images, "images"), (atom_ptr, "atom_ptr"), (offsets, "image_offsets")):
        assert got.dtype == torch.int64 and got.device == torch.device(DEV)
        assert torch.equal(got.cpu(), t(ref[key])), key
    assert pixels.dtype == torch.int16 and torch.equal(pixels.cpu(), t(ref["pixels"]))
    assert (features is None) == (ref["features"] is None)
    if features is not None:
        want = t(ref["features"])
        assert features.dtype == torch.float32 and features.shape == want.shape
        assert torch.equal(bits(features.cpu()), bits(want))


def batches_equal(got, comp):
    from deepviewagg_amd.core.multimodal.csr import CSRBatch
    from deepviewagg_amd.core.multimodal.image import ImageMappingBatch
    assert type(got) is type(comp) is ImageMappingBatch and type(got.values[1]) is type(comp.values[1]) is CSRBatch
    assert got.__csr_type__ is comp.__csr_type__ and got.values[1].__csr_type__ is comp.values[1].__csr_type__
    for a, b in ((got, comp), (got.values[1], comp.values[1])):
        assert a.__sizes__.dtype == b.__sizes__.dtype == torch.int64 and a.__sizes__.device.type == "cpu"
        assert torch.equal(a.__sizes__, b.__sizes__)
        assert a.is_index_value.dtype == torch.bool and a.is_index_value.tolist() == b.is_index_value.tolist()
    assert got.device == comp.device and got.num_values == comp.num_values
    for a, b in ((got.pointers, comp.pointers), (got.images, comp.images),
                 (got.values[1].pointers, comp.values[1].pointers), (got.pixels, comp.pixels)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if got.has_features:
        assert got.features.dtype == comp.features.dtype and got.features.shape == comp.features.shape
        assert torch.equal(bits(got.features), bits(comp.features))
    got.debug()


@pytest.mark.parametrize("name", NAMES)
def test_op_equals_the_restatement(name):
    from deepviewagg_amd import ops
    case = CASES[name]
    items = device_items(case)
    out = ops.collate_mapping(items, point_bases=case["point_bases"], num_points=case["num_points"])
    op_equals_reference(out, reference(name))
    again = ops.collate_mapping(items, point_bases=case["point_bases"], num_points=case["num_points"])
    for a, b in zip(out, again):                           # two calls give the same bits
        assert (a is None and b is None) or torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("name", NAMES)
def test_from_csr_list_equals_the_composition(name):
    from deepviewagg_amd.core.multimodal.image import ImageMappingBatch
    case = CASES[name]
    maps = device_mappings(case)
    kw = dict(group_bases=case["point_bases"], num_groups=case["num_points"])
    with route_calls() as calls:
        got = ImageMappingBatch.from_csr_list(maps, **kw)
        assert calls == {ENTRY: 1, "composition": 0}
        with composition_forced():
            comp = ImageMappingBatch.from_csr_list(maps, **kw)
        assert calls == {ENTRY: 1, "composition": 2}      # the mapping and its nested level
    batches_equal(got, comp)
    ref = reference(name)
    assert torch.equal(got.pointers.cpu(), t(ref["pointers"])) and torch.equal(got.images.cpu(), t(ref["images"]))
    # the batch splits back into its items
    if case["point_bases"] is None:
        for item, back in zip(maps, got.to_csr_list()):
            same_tensors(item, back)


def test_num_groups_below_the_top_is_raised_to_it():
    from deepviewagg_amd.core.multimodal.image import ImageMappingBatch
    maps = device_mappings(CASES["gap_between"])
    got = ImageMappingBatch.from_csr_list(maps, group_bases=[1, 6, 11], num_groups=4)
    with composition_forced():
        comp = ImageMappingBatch.from_csr_list(maps, group_bases=[1, 6, 11], num_groups=4)
    batches_equal(got, comp)
    assert got.num_groups == 16


def device_samples():
    return [mm.to(DEV) for mm in three_samples()]


def image_batches_equal(got, comp):
    from deepviewagg_amd.core.multimodal.image import ImageBatch, SameSettingImageBatch
    assert type(got) is type(comp) is ImageBatch and len(got) == len(comp)
    assert got.num_points == comp.num_points
    for a, b in zip(got, comp):
        assert type(a) is type(b) is SameSettingImageBatch
        assert a.batch_items_sizes.tolist() == b.batch_items_sizes.tolist()
        settings_equal(a, b)
        batches_equal(a.mappings, b.mappings)


def test_image_batch_with_a_missing_setting_equals_the_composition():
    from deepviewagg_amd.core.multimodal.image import ImageBatch
    items = [mm.modalities["image"] for mm in device_samples()]
    with route_calls() as calls:
        got = ImageBatch.from_data_list(items)
        assert calls == {ENTRY: 2, "composition": 0}      # one op per setting
        with composition_forced():
            comp = ImageBatch.from_data_list(items)
        assert calls[ENTRY] == 2 and calls["composition"] == 4
    image_batches_equal(got, comp)
    assert got.num_points == 17 and got[1].mappings.__sizes__.tolist() == [6, 7]
    # the points of the sample without the second setting are empty groups, written in the same pass
    second = got[1].mappings.pointers
    assert bool(torch.all(second[6:11] == second[6]))
    for a, b in zip(items, got.to_data_list()):
        for sa, sb in zip(a, b):
            assert torch.equal(sa.x, sb.x) and torch.equal(sa.pos, sb.pos)
            same_tensors(sa.mappings, sb.mappings)


def test_device_routes_do_not_synchronise():
    from deepviewagg_amd.core.multimodal.data import MMBatch
    from deepviewagg_amd.core.multimodal.image import ImageBatch, ImageMappingBatch
    maps = device_mappings(CASES["feat8"])
    samples = device_samples()
    images = [mm.modalities["image"] for mm in samples]
    runs = {"from_csr_list": lambda: ImageMappingBatch.from_csr_list(maps),
            "ImageBatch.from_data_list": lambda: ImageBatch.from_data_list(images),
            "MMBatch.from_mm_data_list": lambda: MMBatch.from_mm_data_list(samples)}
    for name, run in runs.items():
        run()                                             # library load, allocator warm-up
        with composition_forced():
            n_comp = count_syncs(run)
        n_dev = count_syncs(run)
        print("host synchronisations:", name, "composition", n_comp, "device op", n_dev)
        assert n_comp > 2, f"the sync counter sees {n_comp} synchronisations of the composition: it does not count"
        assert n_dev == 0, name


def test_mm_data_on_the_device_is_built_without_a_synchronisation():
    from deepviewagg_amd.core.multimodal.data import MMData
    mm = device_samples()[0]
    assert count_syncs(lambda: MMData(mm.data, **mm.modalities)) == 0


@pytest.mark.parametrize("kind", ["int32_pixels", "f64_features"])
def test_unsupported_dtypes_raise_in_the_op_and_fall_back_in_the_container(kind):
    from deepviewagg_amd import ops
    from deepviewagg_amd._lib import DvaError
    from deepviewagg_amd.core.multimodal.image import ImageMappingBatch
    dtypes = dict(pixel_dtype=torch.int32) if kind == "int32_pixels" else dict(feature_dtype=torch.float64)
    case = CASES["feat8"]
    with pytest.raises(DvaError) as err:
        ops.collate_mapping(device_items(case, **dtypes))
    assert err.value.code == -2
    maps = device_mappings(case, **dtypes)
    with route_calls() as calls:
        got = ImageMappingBatch.from_csr_list(maps)
        assert calls == {ENTRY: 0, "composition": 2}
    with composition_forced():
        comp = ImageMappingBatch.from_csr_list(maps)
    assert got.pixels.dtype == comp.pixels.dtype and got.features.dtype == comp.features.dtype
    mappings_equal(got, comp)


def test_features_on_some_items_only_and_mixed_widths():
    from deepviewagg_amd import ops
    from deepviewagg_amd._lib import DvaError
    from deepviewagg_amd.core.multimodal.image import ImageMappingBatch
    with_f, without = device_items(CASES["feat8"]), device_items(CASES["nofeat"])
    for items in ([with_f[0], without[0]], [with_f[0], device_items(CASES["feat1"])[0]]):
        with pytest.raises(DvaError) as err:
            ops.collate_mapping(items)
        assert err.value.code == -2
    # the container refuses such a list as the composition does, with the switch on or off
    maps = [device_mappings(CASES["feat8"])[0], device_mappings(CASES["nofeat"])[0]]
    with pytest.raises(AssertionError):
        ImageMappingBatch.from_csr_list(maps)
    with composition_forced(), pytest.raises(AssertionError):
        ImageMappingBatch.from_csr_list(maps)


def test_non_contiguous_inputs():
    from deepviewagg_amd import ops
    case = CASES["feat8"]
    items = []
    for pointers, images, atom_ptr, pixels, feats in device_items(case):
        items.append((torch.stack([pointers, pointers], 1)[:, 0], torch.stack([images, images], 1)[:, 1], atom_ptr,
                      torch.cat([pixels, pixels], 1)[:, :2], torch.cat([feats, feats], 1)[:, 8:]))
        assert not items[-1][3].is_contiguous() and not items[-1][4].is_contiguous()
    op_equals_reference(ops.collate_mapping(items), reference("feat8"))


def test_mm_batch_feeds_multimodal_input():
    """Two samples on the device -> MMBatch.from_mm_data_list -> multimodal_input: the dictionary assembled by hand from
    the concatenated 3D fields and the composition's image batch."""
    from deepviewagg_amd.core.multimodal.data import MMBatch
    from deepviewagg_amd.core.multimodal.image import ImageBatch
    from deepviewagg_amd.modules.multimodal.modules import multimodal_input
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    samples = device_samples()[:2]
    batch = MMBatch.from_mm_data_list(samples)
    assert batch.device == torch.device(DEV) and batch.num_points == 10
    assert torch.equal(batch.mapping_index, torch.arange(10, device=DEV))
    mm = multimodal_input(batch, DEV)
    assert set(mm) == {"x_3d", "x_seen", "modalities"} and mm["x_seen"] is None
    x = torch.cat([s.x for s in samples])
    coords = torch.cat([s.coords for s in samples])
    which = torch.tensor([0] * 6 + [1] * 4, device=DEV)
    want = snn.SparseTensor(x, coords, which, DEV)
    assert torch.equal(mm["x_3d"].F, want.F) and torch.equal(mm["x_3d"].C, want.C) and mm["x_3d"].s == want.s
    with composition_forced():
        images = ImageBatch.from_data_list([s.modalities["image"] for s in samples])
    assert set(mm["modalities"]) == {"image"} and len(mm["modalities"]["image"]) == len(images) == 2
    for a, b in zip(mm["modalities"]["image"], images):
        settings_equal(a, b)
    back = batch.to_mm_data_list()
    for a, b in zip(samples, back):
        assert torch.equal(a.pos, b.pos) and torch.equal(a.mapping_index, b.mapping_index)
        for sa, sb in zip(a.modalities["image"], b.modalities["image"]):
            assert torch.equal(sa.x, sb.x)
            same_tensors(sa.mappings, sb.mappings)
