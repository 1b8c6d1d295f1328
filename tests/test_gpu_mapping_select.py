"""-m gpu: the device mapping selection (``ops.select_mapping``, C ABI dva_mapping_select_count / _fill, and
``ops.mapping_image_stats``) behind ``ImageMapping.select_points(mode='pick')``, ``select_images``, ``select_views``
and ``crop``.  Every case is held with ``torch.equal`` on all five tensors and on ``seen`` to the numpy restatement of
the contracts (tests/mapping_select_ref.py) and to the kept torch compositions (``SELECT_ON_DEVICE = False``), the
container classes, ``is_index_value`` and dtypes included.  Features are compared as bits; under ``crop`` they pass
through the sequential mean, whose non-NaN results are compared as bits and whose NaN must sit at the same places."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, t
from mapping_select_ref import cases, golden_mapping, image_stats_reference, select_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METHODS = ("pick", "images", "views", "crop")
NAMES = ["n1", "empties", "all_dropped", "views63_64_65", "views300", "views_T_plus_1", "atoms_0_1_2_65",
         "unsorted_images", "image_map_perm", "pick_dup_perm", "pick70000", "nofeat", "feat1d", "feat1", "feat8",
         "special_feats"]
ENTRIES = ("dva_mapping_select_count", "dva_mapping_select_fill")
COMPOSITIONS = ("_select_images_composition", "_select_views_composition", "_crop_composition")


def _tile():
    from deepviewagg_amd import _lib
    return _lib.load().dva_mapping_select_tile_views()


CASES, REFS = None, {}


def shared_cases():
    global CASES
    if CASES is None:
        CASES = cases(_tile())
    return CASES


def device_mapping(arrays, pixel_dtype=None, feature_dtype=None):
    from deepviewagg_amd.core.multimodal.csr import CSRData
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    pointers, images, atom_ptr, pixels, feats = arrays
    pixels = t(pixels, DEV) if pixel_dtype is None else t(pixels, DEV).to(pixel_dtype)
    values = [t(images, DEV), CSRData(t(atom_ptr, DEV), pixels, dense=False)]
    if feats is not None:
        values.append(t(feats, DEV) if feature_dtype is None else t(feats, DEV).to(feature_dtype))
    return ImageMapping(t(pointers, DEV), *values, dense=False, is_index_value=[True, False, False][:len(values)])


@contextlib.contextmanager
def composition_forced():
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    ImageMapping.SELECT_ON_DEVICE = False
    try:
        yield
    finally:
        ImageMapping.SELECT_ON_DEVICE = True


def arguments(case, method):
    """(mapping arrays, keyword arguments of the restatement) of one method on one case."""
    if method == "pick":
        return case["mapping"], dict(point_idx=case["point_idx"])
    if method == "images":
        return case["mapping"], dict(image_idx=case["image_idx"])
    if method == "views":
        return case["mapping"], dict(view_mask=case["view_mask"], compact=True)
    return case["crop_mapping"], dict(crop=case["crop"])


def apply(m, method, kw, **extra):
    """(mapping, seen) of one method on a mapping object."""
    if method == "pick":
        return m.select_points(t(kw["point_idx"], DEV), mode='pick'), None
    if method == "images":
        return m.select_images(t(kw["image_idx"], DEV)), None
    if method == "views":
        return m.select_views(t(kw["view_mask"], DEV), **extra)
    w, h, offsets = kw["crop"]
    return m.crop((w, h), t(offsets, DEV)), None


def reference(name, method):
    if (name, method) not in REFS:
        arrays, kw = arguments(shared_cases()[name], method)
        if method == "views" and kw["view_mask"].all():
            kw = {}                                       # the mapping itself, seen None
        REFS[name, method] = select_reference(*arrays, **kw)
    return REFS[name, method]


def bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def features_equal(a, b, mean):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if mean:
        nan = a.isnan()
        assert torch.equal(nan, b.isnan())
        a, b = a.masked_fill(nan, 0), b.masked_fill(nan, 0)
    assert torch.equal(bits(a), bits(b))


def equals_reference(got, seen, ref, mean):
    assert torch.equal(got.pointers.cpu(), t(ref["pointers"])) and torch.equal(got.images.cpu(), t(ref["images"]))
    assert torch.equal(got.values[1].pointers.cpu(), t(ref["atom_ptr"]))
    assert got.pixels.dtype == torch.int16 and torch.equal(got.pixels.cpu(), t(ref["pixels"]))
    assert got.has_features == (ref["features"] is not None)
    if got.has_features:
        features_equal(got.features.cpu(), t(ref["features"]), mean)
    assert (seen is None) == (ref["seen"] is None)
    if seen is not None:
        assert seen.dtype == torch.int64 and seen.device == got.device and torch.equal(seen.cpu(), t(ref["seen"]))


def equals_composition(got, seen, comp, comp_seen, mean):
    assert type(got) is type(comp) and type(got.values[1]) is type(comp.values[1])
    assert got.is_index_value.tolist() == comp.is_index_value.tolist()
    assert got.values[1].is_index_value.tolist() == comp.values[1].is_index_value.tolist()
    assert got.device == comp.device
    for a, b in ((got.pointers, comp.pointers), (got.images, comp.images),
                 (got.values[1].pointers, comp.values[1].pointers), (got.pixels, comp.pixels)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    assert got.has_features == comp.has_features
    if got.has_features:
        features_equal(got.features, comp.features, mean)
    assert (seen is None) == (comp_seen is None)
    if seen is not None:
        assert seen.dtype == comp_seen.dtype and seen.shape == comp_seen.shape and torch.equal(seen, comp_seen)
    got.debug()


def check(name, method):
    arrays, kw = arguments(shared_cases()[name], method)
    m = device_mapping(arrays)
    got, seen = apply(m, method, kw)
    ref = reference(name, method)
    assert "unsupported" not in ref
    mean = method == "crop" and not ref.get("early")
    equals_reference(got, seen, ref, mean)
    with composition_forced():
        comp, comp_seen = apply(m, method, kw)
    equals_composition(got, seen, comp, comp_seen, mean)
    return got, ref


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", NAMES)
def test_selection_matches_restatement_and_composition(name, method):
    got, ref = check(name, method)
    case = shared_cases()[name]
    if name == "all_dropped":
        if method == "crop":
            assert ref["early"] and got.num_views == len(case["mapping"][1])        # the reference's early return
        elif method != "pick":
            assert got.num_views == 0 and got.pointers.tolist() == [0] * 5
    if name == "unsorted_images" and method == "crop":
        arrays = case["crop_mapping"]
        ptr = arrays[0]
        assert any(np.any(np.diff(arrays[1][a:b]) < 0) for a, b in zip(ptr[:-1], ptr[1:])), "the input is sorted"
        images = got.images.cpu().numpy()
        ptr = got.pointers.cpu().numpy()
        assert all(np.all(np.diff(images[a:b]) > 0) for a, b in zip(ptr[:-1], ptr[1:]))
        plain = []                                        # what a filter without the re-sort would give
        for i in range(len(arrays[0]) - 1):
            kept = set(images[ptr[i]:ptr[i + 1]].tolist())
            plain += [int(b) for b in arrays[1][arrays[0][i]:arrays[0][i + 1]] if int(b) in kept]
        assert sorted(plain) == sorted(images.tolist()) and plain != images.tolist()
    if name == "views_T_plus_1" and method == "crop":
        sizes = np.diff(case["crop_mapping"][0])
        assert sizes.max() == _tile() + 1
    if name == "pick70000" and method == "pick":
        assert got.num_groups == 70000


def test_select_views_with_the_image_count_given():
    case = shared_cases()["feat8"]
    m = device_mapping(case["mapping"])
    a, seen_a = m.select_views(t(case["view_mask"], DEV), num_images=case["num_images"])
    b, seen_b = m.select_views(t(case["view_mask"], DEV))
    equals_composition(a, seen_a, b, seen_b, False)
    kept, seen = m.select_views(torch.ones(m.num_views, dtype=torch.bool, device=DEV), num_images=case["num_images"])
    assert seen is None and kept is not m and torch.equal(kept.images, m.images)


def test_crop_that_would_unite_views_takes_the_composition():
    """Two views of one point with the same image: from_dense unites them, the op flags it and the composition runs."""
    pointers = np.array([0, 3, 4], dtype=np.int64)
    images = np.array([1, 0, 1, 0], dtype=np.int64)
    atom_ptr = np.array([0, 1, 3, 4, 5], dtype=np.int64)
    pixels = np.array([[3, 3], [4, 4], [5, 5], [6, 6], [7, 7]], dtype=np.int16)
    feats = np.arange(8, dtype=np.float32).reshape(4, 2)
    arrays = (pointers, images, atom_ptr, pixels, feats)
    crop = (20, 20, np.zeros((2, 2), dtype=np.int64))
    assert select_reference(*arrays, crop=crop) == dict(unsupported=True)
    m = device_mapping(arrays)
    with composition_calls() as comps, entry_calls() as calls:
        got, _ = apply(m, "crop", dict(crop=crop))
        assert calls == {ENTRIES[0]: 1, ENTRIES[1]: 0} and comps["_crop_composition"] == 1
    assert got.pointers.tolist() == [0, 2, 3] and got.images.tolist() == [0, 1, 0]
    assert got.values[1].pointers.tolist() == [0, 2, 4, 5]


@pytest.mark.parametrize("kind", ["int32_pixels", "f64_features"])
def test_unsupported_dtypes_fall_back_to_the_composition(kind):
    case = shared_cases()["feat8"]
    dtypes = dict(pixel_dtype=torch.int32) if kind == "int32_pixels" else dict(feature_dtype=torch.float64)
    for method in METHODS:
        arrays, kw = arguments(case, method)
        m = device_mapping(arrays, **dtypes)
        with entry_calls() as calls:
            got, seen = apply(m, method, kw)
            assert calls[ENTRIES[1]] == 0
        with composition_forced():
            comp, comp_seen = apply(m, method, kw)
        assert got.pixels.dtype == comp.pixels.dtype and got.features.dtype == comp.features.dtype
        assert torch.equal(got.pointers, comp.pointers) and torch.equal(got.images, comp.images)
        assert torch.equal(got.values[1].pointers, comp.values[1].pointers) and torch.equal(got.pixels, comp.pixels)
        assert torch.equal(got.features, comp.features)
        assert (seen is None) == (comp_seen is None) and (seen is None or torch.equal(seen, comp_seen))


@pytest.mark.parametrize("method", METHODS)
def test_batch_input(method):
    from deepviewagg_amd.core.multimodal.image import ImageMapping, ImageMappingBatch
    a, b = shared_cases()["pick_dup_perm"], shared_cases()["atoms_0_1_2_65"]
    batch = ImageMappingBatch.from_csr_list([device_mapping(arguments(a, method)[0]),
                                             device_mapping(arguments(b, method)[0])])
    n, v = batch.num_groups, batch.num_views
    rng = np.random.default_rng(21)
    n_img = int(batch.images.max()) + 1
    kw = dict(point_idx=rng.integers(0, n, size=2 * n), image_idx=rng.permutation(n_img)[:n_img - 2].astype(np.int64),
              view_mask=rng.random(v) < 0.6, crop=(24, 20, rng.integers(0, 25, size=(n_img, 2)).astype(np.int64)))
    if method == "crop":
        assert len(torch.unique(batch.images)) == n_img
    got, seen = apply(batch, method, kw)
    with composition_forced():
        comp, comp_seen = apply(batch, method, kw)
    equals_composition(got, seen, comp, comp_seen, method == "crop")
    arrays = [x.cpu().numpy() for x in (batch.pointers, batch.images, batch.values[1].pointers, batch.pixels,
                                        batch.features)]
    ref_kw = {"pick": dict(point_idx=kw["point_idx"]), "images": dict(image_idx=kw["image_idx"]),
              "views": dict(view_mask=kw["view_mask"], compact=True), "crop": dict(crop=kw["crop"])}[method]
    equals_reference(got, seen, select_reference(*arrays, **ref_kw), method == "crop")
    expected = {"pick": ImageMapping, "images": ImageMappingBatch, "views": ImageMappingBatch, "crop": ImageMapping}
    assert type(got) is expected[method]


def test_op_refuses_what_the_kernels_do_not_take():
    from deepviewagg_amd import _lib, ops
    arrays = shared_cases()["feat8"]["mapping"]
    dev = [t(a, DEV) for a in arrays]
    for bad in ([dev[0], dev[1], dev[2], dev[3].int(), dev[4]], [dev[0], dev[1], dev[2], dev[3], dev[4].double()],
                [dev[0].int(), dev[1], dev[2], dev[3], dev[4]]):
        with pytest.raises(_lib.DvaError) as err:
            ops.select_mapping(*bad)
        assert err.value.code == -2
    with pytest.raises(_lib.DvaError) as err:
        ops.select_mapping(*dev, point_idx=torch.zeros(3, dtype=torch.int32, device=DEV))
    assert err.value.code == -2
    out = ops.select_mapping(*dev, point_idx=torch.tensor([0, len(arrays[0]) - 1], device=DEV))
    assert out[0] is None and out[5]["out_of_range"]
    out = ops.select_mapping(*dev, image_keys=torch.tensor([1, 1, 3], device=DEV),
                             image_map=torch.tensor([0, 1, 2], device=DEV))
    assert out[0] is None and out[5]["duplicate_keys"]
    m = device_mapping(arrays)
    with pytest.raises(AssertionError, match="duplicates"):
        m.select_images(torch.tensor([1, 3, 1], device=DEV))


def test_image_map_table_form_equals_the_key_form():
    from deepviewagg_amd import ops
    case = shared_cases()["image_map_perm"]
    dev = [t(a, DEV) for a in case["mapping"]]
    idx = t(case["image_idx"], DEV)
    table = torch.full((case["num_images"],), -1, dtype=torch.int64, device=DEV)
    table[idx] = torch.arange(idx.shape[0], device=DEV)
    keys, order = torch.sort(idx)
    a = ops.select_mapping(*dev, image_map=table)
    b = ops.select_mapping(*dev, image_keys=keys, image_map=order)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a[:5], b[:5]))
    ref = reference("image_map_perm", "images")
    assert torch.equal(a[1].cpu(), t(ref["images"])) and torch.equal(a[0].cpu(), t(ref["pointers"]))


# ---------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------

def test_image_statistics_equal_restatement_and_bounding_boxes():
    from deepviewagg_amd import ops
    case = shared_cases()["atoms_0_1_2_65"]
    arrays = case["mapping"]
    n_img = case["num_images"] + 3                        # the last images have no atoms
    m = device_mapping(arrays)
    stats = torch.stack(ops.mapping_image_stats(m.images, m.values[1].pointers, m.pixels, n_img))
    ref = image_stats_reference(arrays[1], arrays[2], arrays[3], n_img)
    assert torch.equal(stats.cpu(), t(ref)) and (ref[0] == 0).sum() >= 3
    assert torch.equal(torch.stack(m.image_stats(n_img)), stats)
    boxes = torch.stack(m.bounding_boxes)
    assert torch.equal(stats[1:, :boxes.shape[1]], boxes) and not bool(stats[0, boxes.shape[1]:].any())
    with composition_forced():
        assert m.image_stats(n_img) is None


def setting_of(m, n_img, x=True):
    from deepviewagg_amd.core.multimodal.image import SameSettingImageData
    gen = torch.Generator().manual_seed(4)
    return SameSettingImageData(
        path=np.array([f"img_{i}" for i in range(n_img)]), pos=torch.rand(n_img, 3, generator=gen).to(DEV),
        opk=torch.zeros(n_img, 3, device=DEV), ref_size=(64, 48), proj_upscale=1, mappings=m,
        x=torch.randint(0, 256, (n_img, 3, 48, 64), dtype=torch.uint8, generator=gen).to(DEV) if x else None)


class Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def settings_equal(a, b):
    from deepviewagg_amd.core.multimodal.image import ImageData
    a, b = (list(s) if isinstance(s, ImageData) else [s] for s in (a, b))
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert type(u) is type(v) and u.num_views == v.num_views and tuple(u.crop_size) == tuple(v.crop_size)
        assert list(u.path) == list(v.path)
        for key in ("pos", "crop_offsets", "rollings", "x"):
            p, q = getattr(u, key), getattr(v, key)
            assert (p is None) == (q is None) and (p is None or (p.dtype == q.dtype and torch.equal(p, q))), key
        equals_composition(u.mappings, None, v.mappings, None, False)


@pytest.mark.parametrize("kw", [dict(area_ratio=0.002, n_max=4), dict(area_ratio=0.01, n_max=None, use_bbox=True),
                                dict(area_ratio=0.9, n_max=3, n_min=1)])
def test_pick_images_from_mapping_area_same_as_with_the_composition(kw):
    from deepviewagg_amd.core.data_transform.multimodal.image import PickImagesFromMappingArea
    case = shared_cases()["atoms_0_1_2_65"]
    n_img = case["num_images"] + 2                        # two images without atoms
    n = len(case["mapping"][0]) - 1
    data = Data(pos=torch.zeros(n, 3, device=DEV), mapping_index=torch.arange(n, device=DEV), num_nodes=n)
    _, got = PickImagesFromMappingArea(**kw)(data, setting_of(device_mapping(case["mapping"]), n_img))
    with composition_forced():
        _, comp = PickImagesFromMappingArea(**kw)(data, setting_of(device_mapping(case["mapping"]), n_img))
    settings_equal(got, comp)


# ---------------------------------------------------------------------------------------------------------------
# determinism, launches, synchronisations
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
def test_selection_is_deterministic(method):
    arrays, kw = arguments(shared_cases()["views_T_plus_1"], method)
    m = device_mapping(arrays)
    (a, seen_a), (b, seen_b) = apply(m, method, kw), apply(m, method, kw)
    equals_composition(a, seen_a, b, seen_b, False)


@contextlib.contextmanager
def entry_calls():
    """Counts the launches of the selection entries (the kernels, not the compositions, must be what ran)."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    calls = {k: 0 for k in ENTRIES}
    orig = {k: getattr(lib, k) for k in calls}

    def wrap(name):
        def f(*a):
            calls[name] += 1
            return orig[name](*a)
        return f
    for k in calls:
        setattr(lib, k, wrap(k))
    try:
        yield calls
    finally:
        for k, v in orig.items():
            setattr(lib, k, v)


@contextlib.contextmanager
def composition_calls():
    """Counts the runs of the kept compositions; a pick's is the CSR indexing ``self[idx]``."""
    from deepviewagg_amd.core.multimodal.csr import CSRData
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    calls = {k: 0 for k in COMPOSITIONS + ("__getitem__",)}
    owners = {k: (CSRData if k == "__getitem__" else ImageMapping) for k in calls}
    orig = {k: owners[k].__dict__[k] for k in calls}

    def wrap(name):
        def f(self, *a, **k):
            calls[name] += 1
            return orig[name](self, *a, **k)
        return f
    for k in calls:
        setattr(owners[k], k, wrap(k))
    try:
        yield calls
    finally:
        for k, v in orig.items():
            setattr(owners[k], k, v)


@pytest.mark.parametrize("method", METHODS)
def test_methods_launch_the_device_entries_and_not_the_composition(method):
    arrays, kw = arguments(shared_cases()["feat8"], method)
    m = device_mapping(arrays)
    with composition_calls() as comps, entry_calls() as calls:
        apply(m, method, kw)
        assert calls == {ENTRIES[0]: 1, ENTRIES[1]: 1}
        assert not any(comps.values()), comps
        with composition_forced():
            apply(m, method, kw)
        assert calls == {ENTRIES[0]: 1, ENTRIES[1]: 1}
        assert any(comps.values())


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


@pytest.mark.parametrize("method,extra,bound", [("pick", {}, 1), ("images", {}, 1), ("crop", {}, 1),
                                                ("views", dict(num_images=7), 1), ("views", {}, 2)])
def test_methods_synchronise_at_most_once(method, extra, bound):
    arrays, kw = arguments(shared_cases()["feat8"], method)
    m = device_mapping(arrays)
    apply(m, method, kw, **extra)                         # library load, allocator warm-up
    # the arguments live on the device before the count starts
    if method == "pick":
        arg = t(kw["point_idx"], DEV)
        run = lambda: m.select_points(arg, mode='pick')
    elif method == "images":
        arg = t(kw["image_idx"], DEV)
        run = lambda: m.select_images(arg)
    elif method == "views":
        arg = t(kw["view_mask"], DEV)
        run = lambda: m.select_views(arg, **extra)
    else:
        arg = t(kw["crop"][2], DEV)
        run = lambda: m.crop(kw["crop"][:2], arg)
    with composition_forced():
        run()
        n_comp = count_syncs(run)
    n_dev = count_syncs(run)
    print("host synchronisations:", method, extra, "composition", n_comp, "device op", n_dev)
    assert n_comp > bound, f"the sync counter sees {n_comp} synchronisations of the composition: it does not count"
    assert n_dev <= bound


def test_setting_pick_is_one_op_and_synchronises_at_most_twice():
    case = shared_cases()["pick_dup_perm"]
    idx = t(np.unique(case["point_idx"])[::-1].copy(), DEV)
    images = setting_of(device_mapping(case["mapping"]), case["num_images"] + 1)
    with composition_calls() as comps, entry_calls() as calls:
        got = images.select_points(idx, mode='pick')
        assert calls == {ENTRIES[0]: 1, ENTRIES[1]: 1} and not any(comps.values())
    with composition_forced():
        comp = images.select_points(idx, mode='pick')
        n_comp = count_syncs(lambda: images.select_points(idx, mode='pick'))
    settings_equal(got, comp)
    assert got.num_views < images.num_views               # the image no point sees is gone
    n_dev = count_syncs(lambda: images.select_points(idx, mode='pick'))
    print("host synchronisations: composition", n_comp, "device op", n_dev)
    assert n_comp > 2 and n_dev <= 2


def test_setting_pick_of_unseen_points_keeps_no_image():
    case = shared_cases()["empties"]
    images = setting_of(device_mapping(case["mapping"]), case["num_images"], x=False)
    idx = torch.tensor([0, 1, 3], device=DEV)
    got = images.select_points(idx, mode='pick')
    with composition_forced():
        comp = images.select_points(idx, mode='pick')
    settings_equal(got, comp)
    assert got.num_views == 0 and got.mappings.pointers.tolist() == [0, 0, 0, 0]


def test_setting_pick_equals_the_reference_vectors():
    from test_gpu_transforms_golden import fresh
    g = load_golden("transforms")
    images = fresh(g)
    images.mappings = device_mapping(golden_mapping(g))   # the reference's own order of the pixels inside a view
    got = images.select_points(t(g["sel_keep"], DEV), mode='pick')
    ref = select_reference(*golden_mapping(g), point_idx=g["sel_keep"], compact=True)
    equals_reference(got.mappings, None, dict(ref, seen=None), False)
    assert torch.equal(got.pos.cpu(), t(g["sel_pos"]))


# ---------------------------------------------------------------------------------------------------------------
# whole chains
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("center_roll", [True, False], ids=["s3dis", "kitti360"])
def test_whole_chain_same_as_with_the_compositions(center_roll):
    import random
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    from test_gpu_transforms_golden import fresh
    g = load_golden("transforms")
    keep = torch.randperm(int(g["num_points"]), generator=torch.Generator().manual_seed(7))[:110].to(DEV)

    def run():
        torch.manual_seed(11)
        np.random.seed(11)
        random.seed(11)
        chain = [T.SelectMappingFromPointId()] + ([T.CenterRoll(angular_res=16)] if center_roll else []) + [
            T.PickImagesFromMappingArea(area_ratio=0.003, n_max=5), T.CropImageGroups(padding=2, min_size=16),
            T.PickImagesFromMemoryCredit(credit=int(g["credit"]), k_coverage=2)]
        data = Data(pos=torch.rand(keep.shape[0], 3).to(DEV), mapping_index=keep.clone(), num_nodes=keep.shape[0])
        images = fresh(g)
        for tr in chain:
            data, images = tr(data, images)
        return data, images, (torch.rand(1), np.random.rand(), random.random())

    with entry_calls() as calls:
        data_a, images_a, state_a = run()
        assert calls[ENTRIES[1]] >= 3
        n = dict(calls)
        with composition_forced():
            data_b, images_b, state_b = run()
        assert calls == n
    assert state_a == state_b
    assert torch.equal(data_a.pos, data_b.pos) and torch.equal(data_a.mapping_index, data_b.mapping_index)
    assert len(images_a) >= 1
    settings_equal(images_a, images_b)
