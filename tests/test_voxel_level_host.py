"""CPU tests of the strided voxel level (csrc/voxel_level.hip, ``ops.voxel_level``): the numpy restatement of its
contract (tests/voxel_level_ref.py) against the oracles -- ``downsample_coords``, ``kernel_map_sorted`` in both
directions, ``voxel_parent_index`` -- on the cases the device test runs, the argument checks of the C entries before any
HIP call, and the cache class the parents ride in."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import sparseconv_oracle as O
from oracle import voxel_oracle as VO
from voxel_level_ref import FLAG_KEY, FLAG_STRIDE, level_cases, unit_cases, voxel_level_ref

CASES = level_cases()


@pytest.mark.parametrize("name,coords,ratio,in_stride", CASES, ids=[c[0] for c in CASES])
def test_restatement_is_the_oracles(name, coords, ratio, in_stride):
    ref = voxel_level_ref(coords, ratio, in_stride)
    n = coords.shape[0]
    assert ref["flags"] == 0
    assert np.array_equal(ref["out_coords"], O.downsample_coords(coords, ratio).numpy().reshape(-1, 4))
    assert np.array_equal(ref["parent"], VO.voxel_parent_index(coords, ref["out_coords"], ratio).reshape(-1))
    if ratio != 2 * in_stride:
        assert ref["nbr"] is None and ref["nbr_t"] is None
        return
    offs = O.kernel_offsets(2, in_stride, 1)
    assert ref["nbr"].shape == (8, ref["out_coords"].shape[0]) and ref["nbr_t"].shape == (8, n)
    assert np.array_equal(ref["nbr"], O.kernel_map_sorted(coords, ref["out_coords"], offs).numpy())
    assert np.array_equal(ref["nbr_t"], O.kernel_map_sorted(ref["out_coords"], coords, -offs).numpy())


def test_the_cases_hold_what_they_are_named_for():
    u = unit_cases()
    count = lambda c: np.bincount(voxel_level_ref(c, 2, 1)["parent"])
    assert voxel_level_ref(u["n1_minus_one"], 2, 1)["out_coords"].tolist() == [[-2, -2, -2, 0]]
    assert count(u["sparse_n_out_is_n"]).max() == 1 and u["sparse_n_out_is_n"].shape[0] > 256
    assert count(u["full_parent_and_singles"]).max() == 8 and count(u["full_parent_and_singles"]).min() == 1
    assert count(u["one_parent"]).tolist() == [5]
    ends = np.cumsum(count(u["straddle_63_and_255"]))                      # sorted positions at which a run ends
    assert 64 not in ends and 256 not in ends and ends[-1] > 257
    two = voxel_level_ref(u["two_batches_same_xyz"], 2, 1)["out_coords"]
    assert any((two[:, :3] == r[:3]).all(1).sum() == 2 for r in two)     # one xyz, two batches: two parents
    assert any(c[:, :3].min() < 0 for c in u.values() if c.shape[0])


def test_restatement_flags_and_duplicates():
    odd = np.array([[0, 0, 0, 0], [2, 1, 0, 0], [4, 4, 4, 0]], dtype=np.int32)          # y = 1 at tensor stride 2
    ref = voxel_level_ref(odd, 4, 2)
    assert ref["flags"] == FLAG_STRIDE and ref["nbr"] is None
    assert np.array_equal(ref["out_coords"], O.downsample_coords(odd, 4).numpy())
    assert np.array_equal(ref["parent"], VO.voxel_parent_index(odd, ref["out_coords"], 4))
    dup = np.array([[1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [5, 5, 5, 1], [0, 0, 0, 0]], dtype=np.int32)
    ref = voxel_level_ref(dup, 2, 1)
    offs = O.kernel_offsets(2, 1, 1)
    assert ref["flags"] == 0 and ref["nbr"][6, 0] == 0 and ref["nbr"][0, 0] == 1      # the smallest row wins
    assert np.array_equal(ref["nbr"], O.kernel_map_sorted(dup, ref["out_coords"], offs).numpy())
    assert np.array_equal(ref["nbr"], O.kernel_map(dup, ref["out_coords"], offs).numpy())
    assert np.array_equal(ref["nbr_t"], O.kernel_map_sorted(ref["out_coords"], dup, -offs).numpy())
    far = np.array([[-2 ** 30, -2 ** 30, -2 ** 30, 0], [2 ** 30, 2 ** 30, 2 ** 30, 3]], dtype=np.int32)
    assert voxel_level_ref(far, 2, 1)["flags"] == FLAG_KEY


def test_level_argument_validation_without_gpu():
    """Bad arguments are refused before any HIP call, in the order of the other voxel entries."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    assert lib.dva_version() >= 334
    big = 0x3fffffff + 1
    assert lib.dva_voxel_level_workspace_bytes(-1) == -1
    assert lib.dva_voxel_level_workspace_bytes(big) == -2
    assert lib.dva_voxel_level_workspace_bytes(0) > 0
    assert lib.dva_voxel_level_workspace_bytes(1000) >= 1000 * (8 + 8 + 4 + 4 + 4)
    bounds = (ctypes.c_int64 * 8)(0, 0, 0, 0, 2, 2, 2, 0)
    assert lib.dva_voxel_bounds(None, -1, None, None, 0, None) == -1
    assert lib.dva_voxel_bounds(None, big, None, None, 0, None) == -2
    assert lib.dva_voxel_bounds(None, 0, None, None, 0, None) == 0
    assert lib.dva_voxel_bounds(None, 4, None, None, 0, None) == -1                      # null pointers
    assert lib.dva_voxel_level(None, -1, 2, 1, bounds, None, None, None, None, 0, None) == -1
    assert lib.dva_voxel_level(None, 4, 0, 1, bounds, None, None, None, None, 0, None) == -1    # ratio <= 0
    assert lib.dva_voxel_level(None, 4, 2, 0, bounds, None, None, None, None, 0, None) == -1    # in_stride <= 0
    assert lib.dva_voxel_level(None, big, 2, 1, bounds, None, None, None, None, 0, None) == -2
    assert lib.dva_voxel_level(None, 0, 2, 1, None, None, None, None, None, 0, None) == 0       # n == 0: nothing read
    assert lib.dva_voxel_level(None, 4, 2, 1, bounds, None, None, None, None, 0, None) == -1    # null pointers
    assert lib.dva_voxel_level_maps(None, None, -1, 0, 2, 1, None, None, None) == -1
    assert lib.dva_voxel_level_maps(None, None, 4, 5, 2, 1, None, None, None) == -1             # n_out > n
    assert lib.dva_voxel_level_maps(None, None, 4, 2, 3, 1, None, None, None) == -1             # not kernel 2 / stride 2
    assert lib.dva_voxel_level_maps(None, None, big, 2, 2, 1, None, None, None) == -2
    assert lib.dva_voxel_level_maps(None, None, 0, 0, 2, 1, None, None, None) == 0
    assert lib.dva_voxel_level_maps(None, None, 4, 2, 2, 1, None, None, None) == -1             # null pointers


def test_level_entries_refuse_misaligned_rows_and_bad_bounds_without_gpu():
    """Rows are read as int4, and the bounds are host values: both are looked at before any HIP call."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 256)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ok, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    good = (ctypes.c_int64 * 8)(0, 0, 0, 0, 2, 2, 2, 0)
    assert lib.dva_voxel_bounds(off, 4, ok, ok, 1 << 20, None) == -1
    assert lib.dva_voxel_level(off, 4, 2, 1, good, ok, ok, ok, ok, 1 << 20, None) == -1
    assert lib.dva_voxel_level(ok, 4, 2, 1, good, off, ok, ok, ok, 1 << 20, None) == -1
    assert lib.dva_voxel_level_maps(off, ok, 4, 2, 2, 1, ok, ok, None) == -1
    for bad in ((0, 0, 0, 1, 2, 2, 2, 0), (0, 0, 0, 0, 2 ** 31, 2, 2, 0), (-2 ** 31 - 1, 0, 0, 0, 2, 2, 2, 0)):
        assert lib.dva_voxel_level(ok, 4, 2, 1, (ctypes.c_int64 * 8)(*bad), ok, ok, ok, ok, 1 << 20, None) == -1
    assert lib.dva_voxel_level(ok, 4, 2, 1, good, ok, ok, ok, ok, 16, None) == -1           # workspace too small


def test_ops_voxel_level_rejects_cpu_tensors():
    from deepviewagg_amd import _lib, ops
    c = torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(_lib.DvaError):
        ops.voxel_level(c, 2, 1)
    with pytest.raises(_lib.DvaError):
        ops.voxel_bounds(c)


def test_coord_maps_is_a_dict_that_carries_the_parents():
    """The caches keep the shape the other tests pin (plain keys = tensor strides); parents and bounds ride outside the
    keys and survive ``.to()``; a CPU tensor builds its maps by the composition and caches no parents."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    coords = torch.from_numpy(unit_cases()["n65"])
    x = snn.SparseVoxelTensor(torch.zeros(65, 3), coords)
    assert isinstance(x.coord_maps, snn.CoordMaps) and isinstance(x.coord_maps, dict)
    assert set(x.coord_maps) == {1} and x.coord_maps[1] is x.C and x.coord_maps.parents == {} and x.coord_maps.bounds is None
    x.coord_maps.parents[(1, 2)] = torch.arange(65)
    x.coord_maps.bounds = (1, (0, 0, 0, 0), (1, 1, 1, 1))
    y = x.like(x.F).to("cpu")
    assert isinstance(y.coord_maps, snn.CoordMaps) and set(y.coord_maps) == {1}
    assert torch.equal(y.coord_maps.parents[(1, 2)], torch.arange(65)) and y.coord_maps.bounds == x.coord_maps.bounds
    lazy = snn.cat(x, x, lazy=True).to("cpu")
    assert isinstance(lazy.coord_maps, snn.CoordMaps) and (1, 2) in lazy.coord_maps.parents
    plain = snn.SparseVoxelTensor(torch.zeros(65, 3), coords, coord_maps={}).to("cpu")
    assert type(plain.coord_maps) is dict
    assert snn.LEVEL_ON_DEVICE is True
