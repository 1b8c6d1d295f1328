"""-m gpu: the device mapping merge (``ops.merge_mapping``, C ABI dva_mapping_merge_count / _fill) behind
``ImageMapping.select_points(mode='merge')``.  Every case is held to the numpy restatement of the contract
(tests/mapping_merge_ref.py) with ``torch.equal`` on all five tensors, the features bit for bit, and to the kept torch
composition: indices equal, features within (c + n) * 2^-24 * max|f| -- c source views and n atoms of the merged view
are the lengths of the composition's two fp32 means (the kernel has only the first), each addition rounding once."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, t
from mapping_merge_ref import cases, golden_case, merge_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tile():
    from deepviewagg_amd import ops
    return ops.MERGE_TILE_ATOMS


def device_mapping(arrays):
    from deepviewagg_amd.core.multimodal.csr import CSRData
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    pointers, images, atom_ptr, pixels, feats = arrays
    values = [t(images, DEV), CSRData(t(atom_ptr, DEV), t(pixels, DEV), dense=False)]
    if feats is not None:
        values.append(t(feats, DEV))
    return ImageMapping(t(pointers, DEV), *values, dense=False, is_index_value=[True, False, False][:len(values)])


@contextlib.contextmanager
def composition_forced():
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    ImageMapping.MERGE_ON_DEVICE = False
    try:
        yield
    finally:
        ImageMapping.MERGE_ON_DEVICE = True


def check_case(arrays, idx):
    m = device_mapping(arrays)
    didx = t(idx, DEV)
    got = m.select_points(didx, mode='merge')
    ref = merge_reference(*arrays, idx)
    assert torch.equal(got.pointers.cpu(), t(ref["pointers"]))
    assert torch.equal(got.images.cpu(), t(ref["images"]))
    assert torch.equal(got.values[1].pointers.cpu(), t(ref["atom_ptr"]))
    assert got.pixels.dtype == torch.int16 and torch.equal(got.pixels.cpu(), t(ref["pixels"]))
    assert got.has_features == (arrays[4] is not None)
    if got.has_features:
        assert got.features.dtype == torch.float32 and got.features.shape == ref["features"].shape
        assert torch.equal(got.features.cpu(), t(ref["features"]))         # bit for bit
    assert got.is_index_value.tolist() == [True, False, False][:len(got.values)]
    assert type(got).__name__ == "ImageMapping" and got.device == m.device
    got.debug()
    with composition_forced():
        comp = m.select_points(didx, mode='merge')
    assert torch.equal(got.pointers, comp.pointers) and torch.equal(got.images, comp.images)
    assert torch.equal(got.values[1].pointers, comp.values[1].pointers) and torch.equal(got.pixels, comp.pixels)
    assert got.is_index_value.tolist() == comp.is_index_value.tolist() and type(got) is type(comp)
    if got.has_features:
        assert comp.features.dtype == got.features.dtype and comp.features.shape == got.features.shape
        n = np.diff(ref["atom_ptr"])
        bound = (ref["c"] + n).astype(np.float64) * 2.0 ** -24 * float(np.abs(arrays[4]).max())
        err = (got.features.double() - comp.features.double()).abs().cpu().numpy().reshape(len(n), -1).max(axis=1)
        print("kernel vs composition: max err / bound", (err / bound).max(initial=0.0))
        assert np.all(err <= bound)
    return got


CASES = None


def shared_cases():
    global CASES
    if CASES is None:
        CASES = cases(_tile())
    return CASES


@pytest.mark.parametrize("name", ["n1", "dedupe64", "dedupe65", "empty_voxels", "unseen_mixed", "same_pixels",
                                  "tile_straddle", "one_image", "images300", "nofeat", "feat1", "feat1d", "feat8",
                                  "idx_sorted"])
def test_merge_matches_restatement_and_composition(name):
    arrays, idx = shared_cases()[name]
    got = check_case(arrays, idx)
    if name == "same_pixels":
        # k members, identical pixels: one atom; k different pixels: k atoms in (x, y) order
        assert got.values[1].pointers.tolist() == [0, 1, 6]
        assert got.pixels.tolist() == [[9, 9], [0, 32767], [7, 1], [7, 2], [7, 3], [32767, 0]]
    if name == "empty_voxels":
        sizes = (got.pointers[1:] - got.pointers[:-1]).tolist()
        assert [sizes[j] for j in (2, 3, 8, 9)] == [0, 0, 0, 0] and got.num_groups == 10


def test_merge_golden_fixture():
    g = load_golden("mapping_build")
    arrays, idx = golden_case(g)
    got = check_case(arrays, idx)
    assert got.num_groups == 700 and len(idx) == 3000
    assert np.array_equal(got.pointers.cpu().numpy(), g["merge_pointers"])
    np.testing.assert_allclose(got.features.cpu().numpy(), g["merge_features"], rtol=0, atol=3e-7)


def test_merge_guards_return_a_clone():
    arrays, idx = shared_cases()["feat8"]
    m = device_mapping(arrays)
    missing = idx.copy()
    missing[missing == 5] = 6
    for bad in (missing, idx[:-1]):
        assert merge_reference(*arrays, bad) is None
        out = m.select_points(t(bad, DEV), mode='merge')
        assert out is not m and torch.equal(out.pointers, m.pointers) and torch.equal(out.images, m.images)
        assert torch.equal(out.values[1].pointers, m.values[1].pointers) and torch.equal(out.pixels, m.pixels)
        assert torch.equal(out.features, m.features)


def test_merge_many_single_point_voxels_wrap_the_grid():
    """M = 70 000 single-point voxels (more than the blocks of one launch): the idx-permuted input."""
    from deepviewagg_amd import ops
    n = 70000
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 3, size=n)
    pointers = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    v = int(pointers[-1])
    images = np.concatenate([np.sort(rng.choice(9, size=s, replace=False)) for s in sizes]).astype(np.int64)
    atom_ptr = np.arange(v + 1, dtype=np.int64)
    pixels = rng.integers(0, 500, size=(v, 2)).astype(np.int16)
    feats = rng.standard_normal((v, 3)).astype(np.float32)
    idx = rng.permutation(n).astype(np.int64)
    out = ops.merge_mapping(*(t(a, DEV) for a in (pointers, images, atom_ptr, pixels, feats, idx)))
    assert out[5] is True
    inv = np.argsort(idx)                                  # voxel j is point inv[j]
    view_of = np.concatenate([np.arange(pointers[i], pointers[i + 1]) for i in inv]).astype(np.int64)
    assert torch.equal(out[0].cpu(), t(np.concatenate([[0], np.cumsum(sizes[inv])]).astype(np.int64)))
    assert torch.equal(out[1].cpu(), t(images[view_of]))
    assert torch.equal(out[2].cpu(), t(atom_ptr))
    assert torch.equal(out[3].cpu(), t(pixels[view_of]))
    assert torch.equal(out[4].cpu(), t(feats[view_of]))


def test_merge_is_deterministic():
    from deepviewagg_amd import ops
    arrays, idx = shared_cases()["tile_straddle"]
    args = [t(a, DEV) for a in arrays] + [t(idx, DEV)]
    a, b = ops.merge_mapping(*args), ops.merge_mapping(*args)
    assert a[5] and b[5]
    assert all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))


@contextlib.contextmanager
def merge_calls():
    """Counts the launches of the merge entries (the kernels, not the composition, must be what ran)."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    calls = {"dva_mapping_merge_count": 0, "dva_mapping_merge_fill": 0}
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


def test_select_points_merge_launches_the_device_entries():
    arrays, idx = shared_cases()["feat8"]
    m = device_mapping(arrays)
    with merge_calls() as calls:
        m.select_points(t(idx, DEV), mode='merge')
        assert calls == {"dva_mapping_merge_count": 1, "dva_mapping_merge_fill": 1}
        with composition_forced():
            m.select_points(t(idx, DEV), mode='merge')
        assert calls == {"dva_mapping_merge_count": 1, "dva_mapping_merge_fill": 1}


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


def test_select_points_merge_synchronises_at_most_once():
    arrays, idx = shared_cases()["feat8"]
    m, didx = device_mapping(arrays), t(idx, DEV)
    m.select_points(didx, mode='merge')                    # library load, allocator warm-up
    with composition_forced():
        n_comp = count_syncs(lambda: m.select_points(didx, mode='merge'))
    assert n_comp >= 5, f"the sync counter sees {n_comp} synchronisations of the composition: it does not count"
    n_dev = count_syncs(lambda: m.select_points(didx, mode='merge'))
    print("host synchronisations: composition", n_comp, "device op", n_dev)
    assert n_dev <= 1


def test_multimodal_block_down_same_output_as_with_the_composition():
    from test_gpu_voxel import _StridedBlock
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    from deepviewagg_amd.modules.multimodal.modules import MultimodalBlockDown, SparseVoxels, IdentityBranch
    g = load_golden("mapping_build")
    n_pts = len(g["pointers"]) - 1
    m = ImageMapping.from_dense(t(g["dense_point_ids"], DEV), t(g["dense_image_ids"], DEV),
                                t(g["dense_pixels"], DEV), t(g["dense_features"], DEV), num_points=n_pts)
    gen = torch.Generator().manual_seed(3)
    side = int(np.ceil(n_pts ** (1 / 3))) + 1
    lin = torch.randperm(side ** 3, generator=gen)[:n_pts]
    coords = torch.stack([lin % side, (lin // side) % side, lin // (side * side), torch.zeros_like(lin)], 1).int()
    x_seen = (m.pointers[1:] > m.pointers[:-1])
    feats = torch.randn(n_pts, 4, generator=gen).to(DEV)

    class _Mod:
        def __init__(self, mapping):
            self.mapping = mapping

        def select_points(self, idx, mode='pick'):
            return _Mod(self.mapping.select_points(idx, mode=mode))

    def run():
        block = MultimodalBlockDown(_StridedBlock(), None, image=IdentityBranch())
        return block(dict(x_3d=SparseVoxels(feats, coords.to(DEV), 1), x_seen=x_seen, modalities=dict(image=_Mod(m))))

    with merge_calls() as calls:
        out = run()
        assert calls["dva_mapping_merge_fill"] == 1
        with composition_forced():
            exp = run()
        assert calls["dva_mapping_merge_fill"] == 1
    a, b = out['modalities']['image'].mapping, exp['modalities']['image'].mapping
    # the test double sums the voxel features with index_add_, an atomic scatter: equal up to the order of the additions
    assert torch.allclose(out['x_3d'].F, exp['x_3d'].F, rtol=1e-5, atol=1e-5) and torch.equal(out['x_3d'].C, exp['x_3d'].C)
    assert torch.equal(out['x_seen'], exp['x_seen'])
    assert torch.equal(a.pointers, b.pointers) and torch.equal(a.images, b.images)
    assert torch.equal(a.values[1].pointers, b.values[1].pointers) and torch.equal(a.pixels, b.pixels)
    n = (b.values[1].pointers[1:] - b.values[1].pointers[:-1]).double()
    c = 8.0                                                # a stride-2 voxel holds at most 2^3 points
    bound = (c + n) * 2.0 ** -24 * float(m.features.abs().max())
    assert bool(((a.features.double() - b.features.double()).abs().amax(dim=1) <= bound).all())
    assert a.num_groups == out['x_3d'].C.shape[0]
