"""CPU tests of the mapping merge: the numpy restatement of its contract (tests/mapping_merge_ref.py) against the
reference's own run (the merge_* arrays of tests/golden/mapping_build.npz), and the argument validation of the new
C entries, which happens before any HIP call."""
import ctypes

import numpy as np

from conftest import load_golden
from mapping_merge_ref import cases, golden_case, merge_reference


def per_view_sets(pixels, atom_ptr):
    return [sorted(map(tuple, pixels[a:b].tolist())) for a, b in zip(atom_ptr[:-1], atom_ptr[1:])]


def test_restatement_matches_the_reference_run():
    g = load_golden("mapping_build")
    mapping, idx = golden_case(g)
    out = merge_reference(*mapping, idx)
    assert np.array_equal(out["pointers"], g["merge_pointers"])
    assert np.array_equal(out["images"], g["merge_images"])
    assert np.array_equal(out["atom_ptr"], g["merge_atom_pointers"])
    assert per_view_sets(out["pixels"], out["atom_ptr"]) == per_view_sets(g["merge_pixels"], g["merge_atom_pointers"])
    err = np.abs(out["features"] - g["merge_features"]).max()
    print("max |restatement - reference| on the merged features:", err)
    np.testing.assert_allclose(out["features"], g["merge_features"], rtol=0, atol=3e-7)


def test_restatement_properties_on_the_shared_cases():
    from deepviewagg_amd import ops
    for name, (mapping, idx) in cases(ops.MERGE_TILE_ATOMS).items():
        out = merge_reference(*mapping, idx)
        assert out is not None, name
        m = int(idx.max()) + 1
        assert len(out["pointers"]) == m + 1 and out["pointers"][0] == 0 and out["pointers"][-1] == len(out["images"])
        assert np.all(np.diff(out["pointers"]) >= 0) and np.all(np.diff(out["atom_ptr"]) >= 1), name
        for a, b in zip(out["pointers"][:-1], out["pointers"][1:]):
            assert np.all(np.diff(out["images"][a:b]) > 0), name      # ascending distinct images per voxel
        # every source atom is in the merged view of its (voxel, image), and nothing else is
        pointers, images, atom_ptr, pixels, _ = mapping
        want = set()
        for i in range(len(pointers) - 1):
            for v in range(pointers[i], pointers[i + 1]):
                want.update((int(idx[i]), int(images[v]), int(x), int(y)) for x, y in pixels[atom_ptr[v]:atom_ptr[v + 1]])
        vox = np.repeat(np.arange(m), np.diff(out["pointers"]))
        rep = np.diff(out["atom_ptr"])
        got = list(zip(np.repeat(vox, rep).tolist(), np.repeat(out["images"], rep).tolist(),
                       out["pixels"][:, 0].tolist(), out["pixels"][:, 1].tolist()))
        assert len(got) == len(set(got)) and set(got) == want, name
        assert got == sorted(got), name                                # (voxel, image, x, y) ascending: canonical
    # the straddle case holds what it says
    mapping, idx = cases(ops.MERGE_TILE_ATOMS)["tile_straddle"]
    per_voxel = np.zeros(int(idx.max()) + 1, dtype=np.int64)
    np.add.at(per_voxel, idx, [mapping[2][mapping[0][i + 1]] - mapping[2][mapping[0][i]] for i in range(len(idx))])
    t = ops.MERGE_TILE_ATOMS
    assert {t - 1, t, t + 1} <= set(per_voxel.tolist()) and sorted(per_voxel.tolist())[-3:] == [t - 1, t, t + 1]


def test_restatement_guards():
    mapping, idx = cases(64)["nofeat"]
    assert merge_reference(*mapping, idx[:-1]) is None
    missing = idx.copy()
    missing[missing == 5] = 6
    assert merge_reference(*mapping, missing) is None


def test_ops_surface_and_tile_constant():
    from deepviewagg_amd import _lib, ops
    lib = _lib.load()
    assert lib.dva_version() >= 316
    assert callable(ops.merge_mapping)
    assert ops.MERGE_TILE_ATOMS == lib.dva_mapping_merge_tile_atoms()


def test_merge_entries_validate_arguments_without_gpu():
    """Null, negative and oversized arguments are refused before any HIP call."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED = -1, -2
    assert lib.dva_mapping_merge_workspace_bytes(0, 0, 0) == INVALID
    assert lib.dva_mapping_merge_workspace_bytes(4, -1, 0) == INVALID
    assert lib.dva_mapping_merge_workspace_bytes(4, 1 << 31, 8) == UNSUPPORTED
    assert lib.dva_mapping_merge_workspace_bytes(4, 8, 1 << 31) == UNSUPPORTED
    assert lib.dva_mapping_merge_workspace_bytes(1 << 31, 8, 8) == UNSUPPORTED
    small = lib.dva_mapping_merge_workspace_bytes(4, 8, 8)
    assert small > 0 and lib.dva_mapping_merge_workspace_bytes(4, 8, 9) >= small + 8
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    count, fill = lib.dva_mapping_merge_count, lib.dva_mapping_merge_fill
    assert count(None, None, None, None, 2, None, 4, 8, 8, None, None, 0, None) == INVALID          # null pointers
    assert count(p, p, p, p, 2, p, 0, 8, 8, p, p, 1 << 20, None) == INVALID                        # no points
    assert count(p, p, p, p, 2, p, 4, 1 << 31, 8, p, p, 1 << 20, None) == UNSUPPORTED              # V >= 2^31
    assert count(p, p, p, p, 2, p, 4, 8, 1 << 31, p, p, 1 << 20, None) == UNSUPPORTED              # P >= 2^31
    assert count(p, p, p, p, 4, p, 4, 8, 8, p, p, 1 << 20, None) == UNSUPPORTED                    # int32 pixels
    assert count(p, p, p, p, 3, p, 4, 8, 8, p, p, 1 << 20, None) == INVALID                        # no such dtype
    assert count(p, p, p, p, 2, p, 4, 8, 8, p, p, small - 1, None) == INVALID                      # workspace too small
    args = (4, 8, 8, 2, 3, 3)
    assert fill(None, None, None, None, 2, None, 0, *args, None, None, None, None, None, None, 0, None) == INVALID
    assert fill(p, p, p, p, 2, None, 0, 4, 1 << 31, 8, 2, 3, 3, p, p, p, p, None, p, 1 << 20, None) == UNSUPPORTED
    assert fill(p, p, p, p, 8, None, 0, *args, p, p, p, p, None, p, 1 << 20, None) == UNSUPPORTED  # int64 pixels
    assert fill(p, p, p, p, 2, None, 0, 4, 8, 8, 5, 3, 3, p, p, p, p, None, p, 1 << 20, None) == INVALID    # M > N
    assert fill(p, p, p, p, 2, None, 0, 4, 8, 8, 2, 9, 3, p, p, p, p, None, p, 1 << 20, None) == INVALID    # V' > V
    assert fill(p, p, p, p, 2, p, 6, *args, p, p, p, p, None, p, 1 << 20, None) == INVALID         # features without out
    assert fill(p, p, p, p, 2, p, 1 << 17, *args, p, p, p, p, p, p, 1 << 20, None) == UNSUPPORTED  # F beyond the kernels
    assert fill(p, p, p, p, 2, None, 0, *args, p, p, p, p, None, p, small - 1, None) == INVALID
