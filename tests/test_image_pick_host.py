"""No GPU: the yardsticks of the image picks.  The numpy restatements of CenterRoll's offsets and of the dense coverage
matrix (tests/image_pick_ref.py) against the reference's own run (tests/golden/transforms.npz) and against the torch
expressions of the kept compositions; the three integer identities the kernels rest on; the C ABI; the argument checks
of the wrappers that need no device."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from image_pick_ref import (WIDTHS, DenseCoverage, candidates, center_rollings_integer, center_rollings_reference,
                            col8_float, mapping_from_views, random_mapping, roll_pixels_reference,
                            view_images_of_atoms)

SYMBOLS = ("dva_mapping_center_workspace_bytes", "dva_mapping_center_rollings", "dva_mapping_roll_pixels",
           "dva_mapping_coverage_group_items", "dva_mapping_coverage_hist_images", "dva_mapping_coverage_step")


def torch_center_rollings(image_of_atom, x_of_atom, num_images, width, angular_res):
    """The composition's expressions (CenterRoll._process_composition) on host tensors, without its assertion."""
    col8 = (torch.from_numpy(x_of_atom).float() * 256 / width).long()
    img, col8 = torch.unique(torch.stack([torch.from_numpy(image_of_atom), col8], dim=1), dim=0).unbind(1)   # lexunique
    cand = torch.arange(0, 256, int(256 / angular_res))
    rolled = (col8.view(-1, 1) + cand.view(1, -1)) % 256
    tgt = img.view(-1, 1).expand_as(rolled)
    lo = torch.full((num_images, cand.numel()), 255, dtype=torch.long).scatter_reduce_(0, tgt, rolled, 'amin')
    hi = torch.zeros((num_images, cand.numel()), dtype=torch.long).scatter_reduce_(0, tgt, rolled, 'amax')
    cost = (hi - lo).int() + ((hi.float() + lo) / 2. - 128).abs().int()
    best = cand[cost.min(dim=1).indices]
    return (best.float() / 256. * width).long().numpy()


def test_restatements_reproduce_the_reference_rollings():
    g = load_golden("transforms")
    width, n_img = int(g["ref_size"][0]), g["x"].shape[0]
    img, x = g["image_ids"].astype(np.int64), g["pixels_dense"][:, 0]
    for fn in (center_rollings_reference, center_rollings_integer):
        rollings, empty = fn(img, x, n_img, width, 16)
        assert empty == 0 and np.array_equal(rollings, g["roll_rollings"])
    assert np.array_equal(torch_center_rollings(img, x.astype(np.int64), n_img, width, 16), g["roll_rollings"])


@pytest.mark.parametrize("angular_res", [1, 3, 16, 100, 256])
def test_restatements_equal_the_torch_expressions(angular_res):
    rng = np.random.default_rng(angular_res)
    ties = 0
    for width in (64, 1000, 1408, 32767):
        for span in (None, 5, width // 3):
            pointers, images, atom_ptr, pixels = random_mapping(rng, 60, 7, width, span=span)
            img, x = view_images_of_atoms(images, atom_ptr), pixels[:, 0].astype(np.int64)
            present = np.unique(img)
            ref, _ = center_rollings_reference(img, x, 7, width, angular_res)
            integer, _ = center_rollings_integer(img, x, 7, width, angular_res)
            got = torch_center_rollings(img, x, 7, width, angular_res)
            assert np.array_equal(ref, integer)
            assert np.array_equal(ref[present], got[present])      # (the torch expressions leave no entry for the rest)
            ties += 1
    assert ties == 12


def test_integer_identities():
    for width in WIDTHS + tuple(range(2, 2200, 10)):
        x = np.arange(width, dtype=np.int64)
        col = (torch.from_numpy(x).float() * 256 / width).long().numpy()
        assert np.array_equal(col, (x * 256) // width) and np.array_equal(col, col8_float(x, width))
        r = np.arange(256, dtype=np.int64)
        rolling = (torch.from_numpy(r).float() / 256. * width).long().numpy()
        assert np.array_equal(rolling, (r * width) >> 8)
    hi, lo = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    centre = ((torch.from_numpy(hi).float() + torch.from_numpy(lo)) / 2. - 128).abs().int().numpy()
    assert np.array_equal(centre, np.abs(hi + lo - 256) >> 1)


def test_candidates_of_a_resolution_that_does_not_divide_256():
    assert candidates(3).tolist() == [0, 85, 170, 255]
    assert candidates(100).size == 128 and candidates(256).size == 256 and candidates(1).tolist() == [0]


def test_roll_reference_equals_the_torch_expression():
    rng = np.random.default_rng(3)
    pointers, images, atom_ptr, pixels = random_mapping(rng, 40, 5, 1000)
    rollings = np.array([0, 999, 1, 500, 250], dtype=np.int64)
    pix = torch.from_numpy(pixels.copy())
    roll = torch.from_numpy(rollings)[torch.from_numpy(images)].repeat_interleave(torch.from_numpy(np.diff(atom_ptr)))
    pix[:, 0] = ((pix[:, 0].long() + roll) % 1000).to(pix.dtype)
    assert np.array_equal(pix.numpy(), roll_pixels_reference(images, atom_ptr, pixels, rollings, 1000))


def test_dense_coverage_restatement_equals_the_composition_loop():
    rng = np.random.default_rng(11)
    a = random_mapping(rng, 65, 6, 64)
    b = random_mapping(rng, 50, 3, 64)
    items = [(a[0], a[1], 6), (b[0], b[1], 3)]
    dense = DenseCoverage(items, 65)
    # the composition's own construction and updates, on the host
    seen = torch.zeros(9, 65, dtype=torch.bool)
    first = 0
    for pointers, images, k in items:
        ptr = torch.from_numpy(pointers)
        pts = torch.arange(ptr.shape[0] - 1).repeat_interleave(ptr[1:] - ptr[:-1])
        seen[torch.from_numpy(images) + first, pts] = True
        first += k
    unseen = seen.numpy()
    assert np.array_equal(dense.step(-1), unseen.sum(axis=1))
    assert np.array_equal(dense.step(-1), np.concatenate([np.bincount(a[1], minlength=6), np.bincount(b[1], minlength=3)]))
    for pick in (7, 2, 2, 0):
        unseen &= ~unseen[pick]
        assert np.array_equal(dense.step(pick), unseen.sum(axis=1))


def test_header_declares_the_entries_and_the_library_exports_them():
    from deepviewagg_amd import _lib
    with open(os.path.join(ROOT, "include", "dva.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES
    assert "struct dva_coverage_item" in header
    lib = _lib.load()
    assert lib.dva_version() >= 329
    assert lib.dva_mapping_coverage_group_items() == 32
    assert lib.dva_mapping_coverage_hist_images() >= 64
    assert lib.dva_mapping_center_workspace_bytes(64) >= 64 * 32
    assert lib.dva_mapping_center_workspace_bytes(-1) == -1


def test_entries_reject_bad_arguments_before_any_device_call():
    import ctypes
    from deepviewagg_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)       # never dereferenced: the checks come first
    bad = [dict(angular_res=0), dict(angular_res=257), dict(width=0), dict(pixel_bytes=3), dict(n_views=-1)]
    for kw in bad:
        a = dict(pixel_bytes=2, n_views=1, n_atoms=1, n_images=1, width=64, angular_res=16)
        a.update(kw)
        rc = lib.dva_mapping_center_rollings(one, one, one, a["pixel_bytes"], a["n_views"], a["n_atoms"], a["n_images"],
                                             a["width"], a["angular_res"], one, one, one, 1 << 20, None)
        assert rc == -1, kw
    assert lib.dva_mapping_center_rollings(one, one, one, 4, 1, 1, 1, 64, 16, one, one, one, 1 << 20, None) == -2
    assert lib.dva_mapping_center_rollings(one, one, one, 2, 1, 1, 1, 32768, 16, one, one, one, 1 << 20, None) == -2
    assert lib.dva_mapping_roll_pixels(one, one, one, 2, 1, 1, one, 1, 0, None) == -1
    assert lib.dva_mapping_roll_pixels(one, one, one, 8, 1, 1, one, 1, 64, None) == -2
    item = (_lib.DvaCoverageItem * 2)()
    for d, base in zip(item, (0, 3)):
        d.pointers, d.images, d.n_points, d.n_views, d.n_images, d.image_base = 16, 16, 4, 2, 3, base
    step = lambda n_items, n_points, n_images, pick: lib.dva_mapping_coverage_step(item, n_items, n_points, n_images,
                                                                                  pick, one, one, None, None)
    assert step(2, 4, 6, 6) == -1 and step(2, 4, 6, -2) == -1      # pick out of range
    assert step(2, 3, 6, 0) == -1                                   # an item with more points than the state
    assert step(2, 4, 5, 0) == -1                                   # images past the total
    assert step(0, 4, 6, 0) == -1
    item[1].image_base = 2                                          # overlapping bases
    assert step(2, 4, 6, 0) == -1
    assert lib.dva_mapping_coverage_step(item, 1, 4, 6, 0, one, one, one, None) == -1      # counts == clear


def test_wrappers_reject_bad_arguments():
    from deepviewagg_amd import ops
    from deepviewagg_amd._lib import DvaError
    pointers, images, atom_ptr, pixels = (torch.from_numpy(a) for a in mapping_from_views(2, [(0, 0, [1]), (1, 0, [2])]))
    for res in (0, 257, -1, 16.0, True):
        with pytest.raises(ValueError):
            ops.mapping_center_rollings(images, atom_ptr, pixels, 1, 64, res)
    # pixels other than int16 and indices other than int64 are declined with DVA_ERR_UNSUPPORTED
    for call in (lambda: ops.mapping_center_rollings(images, atom_ptr, pixels.int(), 1, 64, 16),
                 lambda: ops.mapping_center_rollings(images.int(), atom_ptr, pixels, 1, 64, 16),
                 lambda: ops.roll_mapping_pixels(images, atom_ptr, pixels.long(), torch.zeros(1, dtype=torch.int64), 64)):
        with pytest.raises(DvaError) as e:
            call()
        assert e.value.code == -2
    # host tensors: no CPU fallback in the product path
    with pytest.raises(DvaError) as e:
        ops.mapping_center_rollings(images, atom_ptr, pixels, 1, 64, 16)
    assert e.value.code is None
    with pytest.raises(DvaError):
        ops.roll_mapping_pixels(images, atom_ptr, pixels, torch.zeros(1, dtype=torch.int64), 64)
    with pytest.raises(DvaError):
        ops.MappingCoverage([(pointers, images, 1)], 2)
    with pytest.raises(ValueError):
        ops.MappingCoverage([], 2)


def test_transforms_keep_their_compositions_and_switches():
    from deepviewagg_amd.core.data_transform.multimodal.image import CenterRoll, PickImagesFromMemoryCredit
    for cls in (CenterRoll, PickImagesFromMemoryCredit):
        assert cls.ON_DEVICE is True and callable(cls._process_composition)


def test_host_mappings_take_the_compositions():
    """A host ImageData goes through today's code."""
    from deepviewagg_amd.core.data_transform.multimodal.image import PickImagesFromMemoryCredit
    from deepviewagg_amd.core.multimodal.csr import CSRData
    from deepviewagg_amd.core.multimodal.image import ImageData, ImageMapping, SameSettingImageData

    class Data:
        pass
    rng = np.random.default_rng(5)
    pointers, images, atom_ptr, pixels = random_mapping(rng, 80, 6, 64, span=9)
    present = np.unique(images)
    assert present.size == 6
    tt = torch.from_numpy
    m = ImageMapping(tt(pointers), tt(images), CSRData(tt(atom_ptr), tt(pixels.copy()), dense=False), dense=False,
                     is_index_value=[True, False])
    sd = SameSettingImageData(path=np.array([f"i{i}" for i in range(6)]), pos=torch.zeros(6, 3), ref_size=(64, 8),
                              proj_upscale=1, mappings=m)
    data = Data()
    data.pos, data.num_nodes = torch.zeros(80, 3), 80
    want, _ = center_rollings_reference(view_images_of_atoms(images, atom_ptr), pixels[:, 0], 6, 64, 16)
    sd.update_rollings(tt(want), on_device=True)          # a host mapping: the expression, whatever the flag says
    assert np.array_equal(sd.mappings.pixels.numpy(), roll_pixels_reference(images, atom_ptr, pixels, want, 64))
    np.random.seed(2)
    _, picked = PickImagesFromMemoryCredit(credit=64 * 8 * 3, k_coverage=2)(data, ImageData([sd]))
    assert picked.num_views == 3
