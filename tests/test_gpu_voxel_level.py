"""The strided voxel level on the device (csrc/voxel_level.hip, ``ops.voxel_level``, ``Conv3d._build`` with
``snn.LEVEL_ON_DEVICE``): output coordinates, parents and the kernel_size 2 / stride 2 maps from one sort, held bit for
bit to the numpy restatement (tests/voxel_level_ref.py, itself held to the oracles on the CPU), to the oracles and to the
routes they replace (``snn.downsample_coords``, ``ops.voxel_parent_index``, ``ops.voxel_kernel_map``).  Every comparison
is an equality of integer tensors, or of the outputs and gradients of the same kernels fed equal maps."""
import contextlib
import copy
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, t
from oracle import sparseconv_oracle as O
from oracle import voxel_oracle as VO
from voxel_level_ref import level_cases, random_cloud, unit_cases, voxel_level_ref

sys.path.insert(0, os.path.join(ROOT, "tools"))
from measure import launch_counter, sync_warnings   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = level_cases()


@contextlib.contextmanager
def level_on_device(on):
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    found, snn.LEVEL_ON_DEVICE = snn.LEVEL_ON_DEVICE, on
    try:
        yield
    finally:
        snn.LEVEL_ON_DEVICE = found


def composition(coords, ratio, in_stride):
    """(out_coords, parent, nbr, nbr_t) by the routes ``ops.voxel_level`` replaces."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    out = snn.downsample_coords(coords, ratio)
    offs = snn.kernel_offsets(2, in_stride, 1)
    return (out, ops.voxel_parent_index(coords, out, ratio), ops.voxel_kernel_map(coords, out, offs),
            ops.voxel_kernel_map(out, coords, -offs))


def check_level(coords, ratio, in_stride, oracles=True, bounds=None):
    """``ops.voxel_level`` on ``coords`` (numpy) against the restatement, the device routes and the oracles."""
    from deepviewagg_amd import ops
    c = torch.from_numpy(coords).to(DEV)
    n = coords.shape[0]
    lv = ops.voxel_level(c, ratio, in_stride, bounds=bounds)
    ref = voxel_level_ref(coords, ratio, in_stride)
    k2s2 = ratio == 2 * in_stride
    assert lv.out_coords.dtype == torch.int32 and lv.out_coords.is_contiguous() and lv.parent.dtype == torch.int64
    assert lv.out_coords.shape == (ref["out_coords"].shape[0], 4) and lv.parent.shape == (n,)
    assert np.array_equal(lv.out_coords.cpu().numpy(), ref["out_coords"])
    assert np.array_equal(lv.parent.cpu().numpy(), ref["parent"])
    assert lv.direct is k2s2
    out_d, parent_d, nbr_d, nbr_t_d = composition(c, ratio, in_stride)
    assert torch.equal(lv.out_coords, out_d.reshape(-1, 4)) and torch.equal(lv.parent, parent_d)
    if k2s2:
        assert lv.nbr.dtype == torch.int32 and lv.nbr.shape == (8, lv.out_coords.shape[0]) and lv.nbr_t.shape == (8, n)
        assert np.array_equal(lv.nbr.cpu().numpy(), ref["nbr"]) and np.array_equal(lv.nbr_t.cpu().numpy(), ref["nbr_t"])
        assert torch.equal(lv.nbr, nbr_d) and torch.equal(lv.nbr_t, nbr_t_d)
    else:
        assert lv.nbr is None and lv.nbr_t is None
    if oracles:
        assert np.array_equal(lv.out_coords.cpu().numpy(), O.downsample_coords(coords, ratio).numpy().reshape(-1, 4))
        assert np.array_equal(lv.parent.cpu().numpy(), VO.voxel_parent_index(coords, ref["out_coords"], ratio).reshape(-1))
        if k2s2:
            offs = O.kernel_offsets(2, in_stride, 1)
            assert np.array_equal(lv.nbr.cpu().numpy(), O.kernel_map_sorted(coords, ref["out_coords"], offs).numpy())
            assert np.array_equal(lv.nbr_t.cpu().numpy(), O.kernel_map_sorted(ref["out_coords"], coords, -offs).numpy())
    return lv


@pytest.mark.parametrize("name,coords,ratio,in_stride", CASES, ids=[c[0] for c in CASES])
def test_level_is_the_restatement_the_oracles_and_the_composition(name, coords, ratio, in_stride):
    check_level(coords, ratio, in_stride)


@pytest.mark.parametrize("ratio,in_stride", [(2, 1), (4, 2), (8, 4), (3, 1)])
def test_level_large_property(ratio, in_stride):
    """About 2 * 10^5 voxels in +-2000 over 4 batches, shuffled: several hundred blocks, a sort of more than one pass,
    runs across every kind of boundary."""
    coords = random_cloud(200_000, 2000, 4, 31)
    coords[:, :3] *= in_stride
    lv = check_level(coords, ratio, in_stride, oracles=False)
    fl = torch.from_numpy(coords).clone()
    fl[:, :3] = torch.div(fl[:, :3], ratio, rounding_mode="floor") * ratio
    assert int(lv.parent.min()) >= 0 and torch.equal(lv.out_coords[lv.parent].cpu(), fl)


def test_any_valid_bounds_give_the_same_level():
    """The bounds only size the key: those of a finer tensor, or looser ones, change no result."""
    from deepviewagg_amd import ops
    coords = unit_cases()["n5000"]
    lo, hi = ops.voxel_bounds(torch.from_numpy(coords).to(DEV))
    assert lo == tuple(int(v) for v in coords.min(0)) and hi == tuple(int(v) for v in coords.max(0))
    check_level(coords, 2, 1, oracles=False, bounds=(lo, hi))
    check_level(coords, 2, 1, oracles=False, bounds=(tuple(v - 7 for v in lo), tuple(v + 1001 for v in hi)))
    coarse = voxel_level_ref(coords, 2, 1)["out_coords"]
    check_level(coarse, 4, 2, oracles=False, bounds=(lo, hi))              # the finer tensor's bounds, floored on the host


def test_stale_bounds_and_an_unpackable_key_decline():
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    coords = torch.from_numpy(unit_cases()["n257"]).to(DEV)
    lv = ops.voxel_level(coords, 2, 1, bounds=((0, 0, 0, 0), (1, 1, 1, 0)))
    assert lv.out_coords is None and lv.parent is None and lv.nbr is None and lv.direct is False
    far = torch.tensor([[-2 ** 30, -2 ** 30, -2 ** 30, 0], [2 ** 30, 2 ** 30, 2 ** 30, 3]], dtype=torch.int32, device=DEV)
    lv = ops.voxel_level(far, 2, 1)
    assert lv.out_coords is None and lv.direct is False
    for on in (True, False):                                             # the old route raises, as it did
        with level_on_device(on), pytest.raises(AssertionError, match="too large to pack"):
            snn.Conv3d(2, 2, kernel_size=2, stride=2).to(DEV)(snn.SparseVoxelTensor(torch.zeros(2, 2, device=DEV), far))
    # a cache whose bounds are stale falls back to the composition and gives its tensors
    x = snn.SparseVoxelTensor(torch.zeros(257, 2, device=DEV), coords)
    x.coord_maps.bounds = (1, (0, 0, 0, 0), (1, 1, 1, 0))
    snn.Conv3d._build(x, (1, 2, 2, 1), 2)
    exp = composition(coords, 2, 1)
    assert torch.equal(x.coord_maps[2], exp[0]) and x.coord_maps.parents == {} and x.coord_maps.bounds is None
    assert torch.equal(x.kernel_maps[(1, 2, 2, 1)][0], exp[2]) and torch.equal(x.kernel_maps[(1, 2, 2, 1)][1], exp[3])


def built(coords, in_stride, key, on):
    """The caches ``Conv3d._build`` leaves on a fresh tensor, with the parent index its consumer would use."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    x = snn.SparseVoxelTensor(torch.zeros(coords.shape[0], 1, device=DEV), coords, in_stride)
    out_stride = in_stride * key[2]
    with level_on_device(on):
        snn.Conv3d._build(x, key, out_stride)
    parent = x.coord_maps.parents.get((in_stride, out_stride))
    if parent is None:
        parent = ops.voxel_parent_index(x.coord_maps[in_stride], x.coord_maps[out_stride], out_stride)
    return x, parent


def same_caches(a, b):
    assert set(a.coord_maps) == set(b.coord_maps) and set(a.kernel_maps) == set(b.kernel_maps)
    for s in a.coord_maps:
        assert a.coord_maps[s].dtype == b.coord_maps[s].dtype and torch.equal(a.coord_maps[s], b.coord_maps[s]), s
    for key in a.kernel_maps:
        for m, w in zip(a.kernel_maps[key], b.kernel_maps[key]):
            assert m.dtype == w.dtype and torch.equal(m, w), key


def test_coordinates_off_the_input_stride_give_the_compositions_tensors():
    from deepviewagg_amd import ops
    coords = unit_cases()["n257"].copy()
    coords[:, :3] *= 2
    coords[5, 1] += 1                                                    # not a multiple of the tensor stride 2
    coords[200, 2] -= 1
    c = torch.from_numpy(coords).to(DEV)
    lv = ops.voxel_level(c, 4, 2)
    exp = composition(c, 4, 2)
    assert lv.direct is False and lv.nbr is None and lv.nbr_t is None
    assert torch.equal(lv.out_coords, exp[0]) and torch.equal(lv.parent, exp[1])
    on, p_on = built(c, 2, (2, 2, 2, 1), True)
    off, p_off = built(c, 2, (2, 2, 2, 1), False)
    same_caches(on, off)
    assert (2, 4) in on.coord_maps.parents and off.coord_maps.parents == {} and torch.equal(p_on, p_off)
    assert torch.equal(on.kernel_maps[(2, 2, 2, 1)][0], exp[2]) and torch.equal(on.kernel_maps[(2, 2, 2, 1)][1], exp[3])


def test_duplicate_rows_the_smallest_row_wins():
    from deepviewagg_amd import ops
    base = unit_cases()["n257"]
    coords = np.concatenate([base, base[40:140][::-1], base[:7]])          # 107 rows twice, at larger row ids
    c = torch.from_numpy(coords).to(DEV)
    lv = check_level(coords, 2, 1)
    assert lv.direct is True
    first = {}
    for i, r in enumerate(coords.tolist()):
        first.setdefault(tuple(r), i)
    listed = lv.nbr[lv.nbr >= 0].cpu().tolist()
    assert sorted(listed) == sorted(first.values()) and max(listed) < 257
    on, p_on = built(c, 1, (1, 2, 2, 1), True)
    off, p_off = built(c, 1, (1, 2, 2, 1), False)
    same_caches(on, off)
    assert torch.equal(p_on, p_off)


@pytest.mark.parametrize("key", [(1, 3, 2, 1), (1, 2, 2, 2), (2, 2, 3, 1), (1, 1, 2, 1)],
                         ids=["k3s2", "k2s2d2", "k2s3", "k1s2"])
def test_other_strided_kernels_take_coordinates_and_parents_only(key):
    """Any strided kernel but kernel_size 2 / stride 2 / dilation 1: the level's coordinates and parents, the maps by
    the hash query -- the composition's caches."""
    coords = unit_cases()["n5000"].copy()
    coords[:, :3] *= key[0]
    c = torch.from_numpy(coords).to(DEV)
    with launch_counter() as launches:
        on, p_on = built(c, key[0], key, True)
    assert launches.names.count("voxel_level") == 1 and launches.names.count("voxel_kernel_map") == 2
    assert "voxel_level_maps" not in launches.names and "voxel_parent_index" not in launches.names
    off, p_off = built(c, key[0], key, False)
    same_caches(on, off)
    assert torch.equal(p_on, p_off)


def _features(n, c, seed):
    return torch.randn(n, c, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _run(modules, forward, coords, feats, on):
    """Outputs, input and parameter gradients and the caches of ``forward(modules, x)`` on fresh copies."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    mods = [copy.deepcopy(m) for m in modules]
    f = feats.clone().requires_grad_(True)
    x = snn.SparseVoxelTensor(f, coords)
    with level_on_device(on):
        outs = forward(mods, x)
        sum(o.F.square().sum() for o in outs).backward()
    grads = [f.grad] + [p.grad for m in mods for p in m.parameters()]
    return [o.F.detach() for o in outs] + [o.C for o in outs], grads, x


def _same_run(modules, forward, coords, feats, parameter_grads=True):
    """Both routes on the same inputs: equal caches, outputs and gradients, bit for bit.

    The two routes hand the SAME kernels the same maps (``same_caches``), so any difference would be those kernels' own
    run-to-run freedom, and only the weight gradient has one: ``sconv_wgrad_kernel`` adds one fp32 partial per wavefront
    to each element with atomics, and a wavefront has a partial once there are 32 destination rows for it.  Up to 64
    destination rows there are at most two partials per element, whose sum does not depend on their order; the tests
    that compare parameter gradients stay at or below that, and the larger ones compare everything else."""
    out_on, g_on, x_on = _run(modules, forward, coords, feats, True)
    out_off, g_off, x_off = _run(modules, forward, coords, feats, False)
    same_caches(x_on, x_off)
    assert x_on.coord_maps.parents and not x_off.coord_maps.parents
    for i, (a, b) in enumerate(zip(out_on, out_off)):
        assert a.shape == b.shape and torch.equal(a, b), f"output {i}"
    assert len(g_on) == len(g_off)
    for i, (a, b) in enumerate(zip(g_on, g_off)):
        if i > 0 and not parameter_grads:
            assert a.shape == b.shape
            continue
        assert a is not None and torch.equal(a, b), f"gradient {i}: max |a - b| = {float((a - b).abs().max()):.3e}"
    return x_on


@pytest.mark.parametrize("case", ["n63", "n257"])
def test_conv_and_its_transpose_are_the_same_on_either_route(case):
    """n63: outputs, the input gradient and every parameter gradient; n257 (several tiles per wavefront): outputs and
    the input gradient."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    torch.manual_seed(3)
    coords = torch.from_numpy(unit_cases()[case]).to(DEV)
    n = coords.shape[0]
    mods = [snn.Conv3d(8, 16, kernel_size=2, stride=2, bias=True).to(DEV),
            snn.Conv3dTranspose(16, 8, kernel_size=2, stride=2).to(DEV)]

    def forward(m, x):
        y = m[0](x)
        z = m[1](y)
        assert y.coord_maps is x.coord_maps and z.coord_maps is x.coord_maps and z.C is x.C and y.s == 2 and z.s == 1
        return [y, z]
    x = _same_run(mods, forward, coords, _features(n, 8, 4), parameter_grads=n <= 64)
    assert set(x.coord_maps) == {1, 2} and set(x.kernel_maps) == {(1, 2, 2, 1)} and x.coord_maps[1] is x.C


def test_resnet_down_and_up_are_the_same_on_either_route():
    from deepviewagg_amd.modules.SparseConv3d import ResNetDown, ResNetUp
    torch.manual_seed(5)
    coords = torch.from_numpy(unit_cases()["n63"]).to(DEV)
    mods = [ResNetDown(down_conv_nn=[8, 16], N=1).to(DEV), ResNetDown(down_conv_nn=[16, 16], N=1).to(DEV),
            ResNetUp(up_conv_nn=[16, 16, 16], N=1).to(DEV), ResNetUp(up_conv_nn=[16, 8, 8], N=1).to(DEV)]

    def forward(m, x):
        d1 = m[0](x)
        d2 = m[1](d1)
        u1 = m[2](d2, d1)
        return [d1, d2, u1, m[3](u1, x)]
    x = _same_run(mods, forward, coords, _features(63, 8, 6))
    assert set(x.coord_maps) == {1, 2, 4} and set(x.coord_maps.parents) == {(1, 2), (2, 4)}
    assert x.coord_maps.bounds[0] == 1


def test_multimodal_block_down_uses_the_cached_parents():
    """The HIP stage between the multimodal branches: the same ``x_seen`` and mappings on either route, and on the new
    one neither hash query runs."""
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    from deepviewagg_amd.modules.multimodal.modules import MultimodalBlockDown, IdentityBranch
    from deepviewagg_amd.modules.SparseConv3d import ResNetDown, nn as snn
    g = load_golden("mapping_build")
    n_pts = len(g["pointers"]) - 1
    m = ImageMapping.from_dense(t(g["dense_point_ids"], DEV), t(g["dense_image_ids"], DEV),
                                t(g["dense_pixels"], DEV), t(g["dense_features"], DEV), num_points=n_pts)
    gen = torch.Generator().manual_seed(2)
    side = int(np.ceil(n_pts ** (1 / 3))) + 1
    lin = torch.randperm(side ** 3, generator=gen)[:n_pts]
    coords = torch.stack([lin % side - 3, (lin // side) % side, lin // (side * side) - 2, torch.zeros_like(lin)], 1).int()
    x_seen = (m.pointers[1:] > m.pointers[:-1])

    class _Mod:
        def __init__(self, mapping):
            self.mapping = mapping

        def select_points(self, idx, mode='pick'):
            return _Mod(self.mapping.select_points(idx, mode=mode))

    torch.manual_seed(0)
    stage = ResNetDown(down_conv_nn=[4, 16], N=1).to(DEV)
    feats = _features(n_pts, 4, 8)

    def run(on, block):
        x = snn.SparseTensor(feats.cpu(), coords[:, :3], coords[:, 3], DEV)     # as multimodal_input builds it
        assert isinstance(x.coord_maps, snn.CoordMaps) and x.coord_maps[1] is x.C and x.C.is_cuda
        with level_on_device(on), launch_counter() as launches, torch.no_grad():
            out = MultimodalBlockDown(copy.deepcopy(block), None, image=IdentityBranch())(
                dict(x_3d=x, x_seen=x_seen.clone(), modalities=dict(image=_Mod(m))))
        return out, launches.names
    # the level alone (one kernel_size 2 / stride 2 convolution as the block): no hash query at all
    _, names_on = run(True, snn.Conv3d(4, 16, kernel_size=2, stride=2).to(DEV))
    _, names_off = run(False, snn.Conv3d(4, 16, kernel_size=2, stride=2).to(DEV))
    assert "voxel_kernel_map" not in names_on and "voxel_parent_index" not in names_on
    assert names_on.count("voxel_level") == 1 and names_on.count("voxel_level_maps") == 1
    assert names_off.count("voxel_kernel_map") == 2 and names_off.count("voxel_parent_index") == 1
    # the stage: its 3x3x3 stride-1 convolutions keep their hash query, the level adds none
    on, names_on = run(True, stage)
    off, names_off = run(False, stage)
    assert "voxel_parent_index" not in names_on and names_off.count("voxel_parent_index") == 1
    assert names_on.count("voxel_kernel_map") == names_off.count("voxel_kernel_map") - 2
    assert torch.equal(on['x_seen'], off['x_seen']) and on['x_seen'].dtype == off['x_seen'].dtype
    assert torch.equal(on['x_3d'].C, off['x_3d'].C) and on['x_3d'].s == 2 and on['x_3d'].F.shape == off['x_3d'].F.shape
    a, b = on['modalities']['image'].mapping, off['modalities']['image'].mapping
    assert torch.equal(a.pointers, b.pointers) and torch.equal(a.images, b.images)
    assert torch.equal(a.values[1].pointers, b.values[1].pointers) and torch.equal(a.pixels, b.pixels)
    assert torch.equal(a.features, b.features)
    ref_idx = torch.from_numpy(VO.voxel_parent_index(coords.numpy(), on['x_3d'].C.cpu().numpy(), 2))
    assert torch.equal(on['x_3d'].coord_maps.parents[(1, 2)].cpu(), ref_idx)


def test_one_synchronisation_per_level_and_one_per_input_tensor():
    """By construction: the record (n_out and the flags) is one host read per strided level, the bounds one per input
    tensor; a level whose maps are cached reads nothing."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    coords = torch.from_numpy(unit_cases()["n5000"]).to(DEV)
    convs = [snn.Conv3d(4, 4, kernel_size=2, stride=2).to(DEV) for _ in range(3)]
    x = snn.SparseVoxelTensor(_features(5000, 4, 9), coords)
    counts = []
    with torch.no_grad():
        for conv in convs:
            with sync_warnings() as syncs:
                x = conv(x)
            counts.append(len(syncs))
        print(f"synchronisations per level: {counts}")
        assert counts[0] <= 2 and counts[1] <= 1 and counts[2] <= 1 and x.s == 8
        again = snn.SparseVoxelTensor(_features(5000, 4, 9), coords, 1, x.coord_maps, x.kernel_maps)
        with sync_warnings() as syncs:
            convs[0](again)
        assert len(syncs) == 0
