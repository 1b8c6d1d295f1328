"""Without a GPU: the numpy restatement of the mapping selections (tests/mapping_select_ref.py) against the vectors the
reference's own source wrote (tests/golden/transforms.npz) and against the kept torch compositions on CPU tensors, and
the workspace query of the device op.

``crop``'s composition ends in ``ImageMapping.from_dense``, which sorts on the HIP device and has no CPU form: the
restatement of ``crop`` is held to the reference's vectors here and to the composition in test_gpu_mapping_select.py."""
import numpy as np
import pytest
import torch

from conftest import load_golden, t
from mapping_select_ref import cases, golden_mapping, image_stats_reference, select_reference

from deepviewagg_amd import _lib

KEYS = (("pointers", "pointers"), ("images", "images"), ("atom_ptr", "atom_pointers"), ("pixels", "pixels"),
        ("features", "features"))


def canonical(pixels, atom_ptr):
    """The pixels of every view as a sorted set: the reference's from_dense orders them by an unstable sort."""
    view = np.repeat(np.arange(len(atom_ptr) - 1), np.diff(atom_ptr))
    return pixels[np.lexsort((pixels[:, 1], pixels[:, 0], view))]


def equals_golden(ref, g, prefix, sets=False):
    for mine, theirs in KEYS:
        a, b = ref[mine], g[prefix + theirs]
        assert a.shape == b.shape, (prefix, mine, a.shape, b.shape)
        if sets and mine == "pixels":
            a, b = canonical(a, ref["atom_ptr"]), canonical(b, ref["atom_ptr"])
        assert np.array_equal(a, b.astype(a.dtype)), (prefix, mine)


def upscaled_mapping(g):
    """The generator wrote the crop_ and sv_ vectors after upscale_images(2) and upscale_images(3, center=False) of the
    same mapping, which share its nested CSR and so had moved its pixels to 3 (2 p + 1)."""
    pointers, images, atom_ptr, pixels, features = golden_mapping(g)
    moved = (3 * (2 * pixels.astype(np.int64) + 1)).astype(np.int16)
    assert np.array_equal(moved, g["up3nc_pixels"])
    return pointers, images, atom_ptr, moved, features


def test_pick_with_seen_images_equals_the_reference_vectors():
    g = load_golden("transforms")
    ref = select_reference(*golden_mapping(g), point_idx=g["sel_keep"], compact=True)
    equals_golden(ref, g, "sel_")
    assert len(ref["seen"]) == int(g["sel_num_views"])
    assert np.array_equal(g["pos"][ref["seen"]].astype(np.float64), g["sel_pos"])


def test_select_views_equals_the_reference_vectors():
    g = load_golden("transforms")
    ref = select_reference(*upscaled_mapping(g), view_mask=g["view_mask"], compact=True)
    equals_golden(ref, g, "sv_")
    assert np.array_equal(ref["seen"], g["sv_seen_images"])


def test_crop_equals_the_reference_vectors():
    g = load_golden("transforms")
    crop = (int(g["crop_size"][0]), int(g["crop_size"][1]), g["crop_offsets"])
    ref = select_reference(*upscaled_mapping(g), crop=crop)
    equals_golden(ref, g, "crop_", sets=True)
    assert ref["features"].dtype == np.float32 and ref["pixels"].dtype == np.int16


@pytest.mark.parametrize("tag,ratio,n_max,use_bbox", [("area", 0.003, 4, False), ("bbox", 0.05, None, True)])
def test_statistics_and_select_images_equal_the_reference_vectors(tag, ratio, n_max, use_bbox):
    g = load_golden("transforms")
    mapping = golden_mapping(g)
    n_img = g["x"].shape[0]
    stats = image_stats_reference(mapping[1], mapping[2], mapping[3], n_img)
    moved = upscaled_mapping(g)                           # the bbox vector was written after the upscales too
    assert np.array_equal(image_stats_reference(moved[1], moved[2], moved[3], n_img)[1:], g["bbox"])
    areas = (stats[2] - stats[1]) * (stats[4] - stats[3]) if use_bbox else stats[0].astype(np.float32)
    areas = np.where(stats[0] == 0, 0, areas)
    order = np.argsort(areas, kind='stable')[::-1]
    idx = order[areas[order] > int(g["ref_size"][0]) * int(g["ref_size"][1]) * ratio][:n_max]
    assert np.array_equal(g["pos"][idx].astype(np.float64), g[f"pick_{tag}_pos"])
    equals_golden(select_reference(*mapping, image_idx=idx), g, f"pick_{tag}_")


# ---------------------------------------------------------------------------------------------------------------
# the restatement against the compositions on CPU tensors
# ---------------------------------------------------------------------------------------------------------------

CASES = None


def shared_cases():
    global CASES
    if CASES is None:
        CASES = cases(_lib.load().dva_mapping_select_tile_views())
    return CASES


NAMES = ["n1", "empties", "all_dropped", "views63_64_65", "views300", "views_T_plus_1", "atoms_0_1_2_65",
         "unsorted_images", "image_map_perm", "pick_dup_perm", "pick70000", "nofeat", "feat1d", "feat1", "feat8",
         "special_feats"]


def cpu_mapping(arrays):
    from deepviewagg_amd.core.multimodal.csr import CSRData
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    pointers, images, atom_ptr, pixels, feats = arrays
    values = [t(images), CSRData(t(atom_ptr), t(pixels), dense=False)]
    if feats is not None:
        values.append(t(feats))
    return ImageMapping(t(pointers), *values, dense=False, is_index_value=[True, False, False][:len(values)])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def equals_reference(got, ref):
    assert same_bits(got.pointers.numpy(), ref["pointers"]) and same_bits(got.images.numpy(), ref["images"])
    assert same_bits(got.values[1].pointers.numpy(), ref["atom_ptr"]) and same_bits(got.pixels.numpy(), ref["pixels"])
    assert got.has_features == (ref["features"] is not None)
    if got.has_features:
        assert same_bits(got.features.numpy(), ref["features"])


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_compositions_on_cpu(name):
    case = shared_cases()[name]
    m = cpu_mapping(case["mapping"])
    equals_reference(m.select_points(t(case["point_idx"]), mode='pick'),
                     select_reference(*case["mapping"], point_idx=case["point_idx"]))
    equals_reference(m.select_images(t(case["image_idx"])),
                     select_reference(*case["mapping"], image_idx=case["image_idx"]))
    got, seen = m.select_views(t(case["view_mask"]))
    ref = select_reference(*case["mapping"], view_mask=case["view_mask"], compact=True)
    if case["view_mask"].all():
        assert seen is None
        ref = select_reference(*case["mapping"])
    else:
        assert same_bits(seen.numpy(), ref["seen"])
    equals_reference(got, ref)


def test_image_statistics_restatement_equals_bounding_boxes_on_cpu():
    case = shared_cases()["atoms_0_1_2_65"]
    m = cpu_mapping(case["mapping"])
    boxes = torch.stack(m.bounding_boxes).numpy()
    n = boxes.shape[1]
    stats = image_stats_reference(*case["mapping"][1:4], case["num_images"])
    assert np.array_equal(stats[1:, :n], boxes) and not stats[0, n:].any()


# ---------------------------------------------------------------------------------------------------------------
# workspace query
# ---------------------------------------------------------------------------------------------------------------

QUERY = "dva_mapping_select_workspace_bytes"
# regions padded to 16 bytes: 8 flag words, seen and rank int32 [B], views and atoms per point int32 [M], their two
# int64 scans [M + 1], the block sums int64 [ceil(M / 1024) + 1], and with a crop the atoms per view int32 [V]
PINNED = [((1, 0, 0, 0), 32 + 0 + 0 + 16 + 16 + 16 + 16 + 16),
          ((4, 8, 3, 0), 32 + 16 + 16 + 16 + 16 + 48 + 48 + 16),
          ((4, 8, 3, 1), 32 + 16 + 16 + 16 + 16 + 48 + 48 + 16 + 32),
          ((70000, 150000, 300, 1), 32 + 1200 + 1200 + 280000 + 280000 + 560016 + 560016 + 560 + 600000)]


@pytest.mark.parametrize("args,expected", PINNED, ids=[str(a) for a, _ in PINNED])
def test_select_workspace_sizes(args, expected):
    assert getattr(_lib.load(), QUERY)(*args) == expected
    assert _lib.workspace_bytes(QUERY, *args) == expected
    ws, nbytes = _lib.workspace(QUERY, "cpu", *args)
    assert nbytes == expected and ws.dtype == torch.uint8 and ws.shape == (expected,)


@pytest.mark.parametrize("args,code", [((0, 3, 3, 0), -1), ((4, -1, 3, 0), -1), ((1 << 31, 8, 3, 0), -2),
                                       ((4, 1 << 31, 3, 1), -2)])
def test_select_workspace_raises_on_a_refused_query_before_it_allocates(monkeypatch, args, code):
    made = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append((a, k)) or real_empty(*a, **k))
    with pytest.raises(_lib.DvaError) as err:
        _lib.workspace(QUERY, "cpu", *args)
    assert err.value.code == code and QUERY in str(err.value) and made == []


def test_entries_reject_bad_arguments_before_any_device_call():
    lib = _lib.load()
    assert lib.dva_mapping_select_tile_views() >= 64
    nil = [None] * 4
    assert lib.dva_mapping_select_count(*nil, 2, 1, 0, 0, None, 1, None, None, None, 0, 0, 0, 0, 0, None, None, None,
                                        0, None) == -1                       # null pointers
    assert lib.dva_mapping_select_count(*nil, 4, 1, 0, 0, None, 1, None, None, None, 0, 0, 0, 0, 0, None, None, None,
                                        0, None) == -2                       # int32 pixels
    assert lib.dva_mapping_select_count(*nil, 2, 1, 1 << 31, 0, None, 1, None, None, None, 0, 0, 0, 0, 0, None, None,
                                        None, 0, None) == -2                 # 2^31 views
    assert lib.dva_mapping_image_stats(None, None, None, 8, 1, 1, 1, None, None) == -2
    assert lib.dva_mapping_image_stats(None, None, None, 2, 1, 1, 1, None, None) == -1
