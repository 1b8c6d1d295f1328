"""Sphere and cylinder sampling on the device (csrc/ball.hip through ops.radius_query): the reference's own outputs
(tests/golden/sampling_*.npz, tools/gen_golden_sampling.py) with torch.equal on every attribute, for CPU and device
input; the inclusive boundary on a 1/8 lattice; the empty and the all-points sphere; 2^22 points x 64 centres against
a float64 torch restatement of the predicate written here; identical bytes from identical calls; the Grid* tilings with
the reference's samples, order and center_label; GridSampling3D -> SaveOriginalPosId -> SphereSampling ->
SelectMappingFromPointId end to end."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden, t
from deepviewagg_amd import ops
from deepviewagg_amd.core.data_transform import grid_transform as G
from deepviewagg_amd.core.data_transform import transforms as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEVICES = ["cpu", DEV]
BAND = 1e-9          # pairs with |d - r^2| <= BAND r^2 are left out of the comparison with the restatement


def check(got, want, what, device):
    want = torch.as_tensor(want)
    assert got.device.type == torch.device(device).type, (what, got.device)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got.cpu(), want), what


def inputs_of(g):
    inp = {k[3:]: t(v) for k, v in g.items() if k.startswith("in_")}
    inp["origin_id"] = torch.arange(inp["pos"].shape[0])
    return inp


def to(inp, device):
    return SimpleNamespace(**{k: v.to(device) for k, v in inp.items()})


def check_sample(out, inp, idx, out_pos, what, device):
    idx = torch.as_tensor(idx)
    check(out.origin_id, idx, what + ":origin_id", device)
    check(out.pos, out_pos, what + ":pos", device)
    for k in ("rgb", "y"):
        check(getattr(out, k), inp[k][idx], f"{what}:{k}", device)
    check(out.meta, inp["meta"], what + ":meta", device)
    assert not hasattr(out, "kd_tree")


def sampler_of(name, tag):
    if name == "sampling_sphere_room" or tag.startswith("sphere"):
        return T.SphereSampling
    return T.CylinderSampling


# ---------------------------------------------------------------------------------------------------------------
# the reference's outputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", ["sampling_sphere_room", "sampling_cylinder_street", "sampling_edges"])
def test_samples_match_the_reference(name, device):
    g = load_golden(name)
    inp = inputs_of(g)
    for tag in (str(c) for c in g["cases"]):
        data = to(inp, device)
        meta_in = data.meta
        sampler = sampler_of(name, tag)(float(g[f"{tag}_radius"]), g[f"{tag}_centre"],
                                        align_origin=bool(g[f"{tag}_align"]))
        out = sampler(data)
        assert isinstance(out, SimpleNamespace) and out is not data
        check_sample(out, inp, g[f"{tag}_idx"], g[f"{tag}_out_pos"], f"{name}:{tag}", device)
        assert out.meta is not meta_in                                        # other tensors are cloned
        # the input is left as it was: no tree attached, nothing shifted
        assert not hasattr(data, "kd_tree") and torch.equal(data.pos.cpu(), inp["pos"])


def test_lattice_pins_the_inclusive_boundary():
    g = load_golden("sampling_edges")
    pos = t(g["in_pos"], DEV)
    for tag, dims in (("sphere_boundary", 3), ("sphere_boundary_shifted", 3), ("cylinder_boundary", 2),
                      ("cylinder_boundary_shifted", 2)):
        c = g[f"{tag}_centre"][:dims]
        r = float(g[f"{tag}_radius"])
        ptr, idx = ops.radius_query(pos, c, r, dims=dims)
        assert torch.equal(idx.cpu(), t(g[f"{tag}_idx"])), tag
        d = ((g["in_pos"][:, :dims].astype(np.float64) - c) ** 2).sum(1)      # exact on the lattice
        on = torch.from_numpy(np.nonzero(d == r * r)[0])
        assert on.shape[0] == int(g[f"{tag}_on_boundary"]) >= 20
        assert bool(torch.isin(on, idx.cpu()).all()), tag                      # d == r r is inside
        # the next float64 below r leaves exactly the boundary points out
        ptr2, idx2 = ops.radius_query(pos, c, float(np.nextafter(r, 0.0)), dims=dims)
        assert int(ptr2[1]) == int(ptr[1]) - on.shape[0], tag
        assert not bool(torch.isin(on, idx2.cpu()).any()), tag


def test_empty_and_all_points_spheres():
    g = load_golden("sampling_edges")
    pos = t(g["in_pos"], DEV)
    n = pos.shape[0]
    ptr, idx = ops.radius_query(pos, g["sphere_empty_centre"], float(g["sphere_empty_radius"]))
    assert ptr.tolist() == [0, 0] and idx.shape == (0,) and idx.dtype == torch.int64 and idx.is_cuda
    ptr, idx = ops.radius_query(pos, g["sphere_all_centre"], float(g["sphere_all_radius"]))
    assert ptr.tolist() == [0, n] and torch.equal(idx.cpu(), torch.arange(n))
    # both in one call, with an empty one between two full ones
    c = np.stack([g["sphere_all_centre"], g["sphere_empty_centre"], g["sphere_all_centre"]])
    ptr, idx = ops.radius_query(pos, c, np.array([50.0, 1.0, 50.0]))
    assert ptr.tolist() == [0, n, n, 2 * n] and torch.equal(idx.cpu(), torch.arange(n).repeat(2))
    # no centres, no points
    ptr, idx = ops.radius_query(pos, np.zeros((0, 3)), 1.0)
    assert ptr.tolist() == [0] and idx.shape == (0,) and ptr.is_cuda
    ptr, idx = ops.radius_query(pos[:0], np.zeros((3, 2)), 1.0, dims=2)
    assert ptr.tolist() == [0, 0, 0, 0] and idx.shape == (0,)
    out = T.SphereSampling(1.0, g["sphere_empty_centre"])(SimpleNamespace(pos=pos, y=torch.arange(n, device=DEV)))
    assert out.pos.shape == (0, 3) and out.y.shape == (0,) and out.pos.is_cuda


def test_non_finite_points_are_never_members():
    pos = torch.rand(5000, 3, generator=torch.Generator().manual_seed(3))
    bad = torch.tensor([5, 77, 640, 4999])
    pos[bad[0], 0] = float("nan")
    pos[bad[1], 1] = float("inf")
    pos[bad[2], 2] = float("-inf")
    pos[bad[3]] = float("nan")
    for dims in (2, 3):
        ptr, idx = ops.radius_query(pos.to(DEV), np.full((1, dims), 0.5), float("inf"), dims=dims)
        keep = torch.ones(5000, dtype=torch.bool)
        keep[bad] = False
        assert torch.equal(idx.cpu(), torch.nonzero(keep).flatten()), dims


# ---------------------------------------------------------------------------------------------------------------
# 2^22 points against a float64 restatement of the predicate
# ---------------------------------------------------------------------------------------------------------------
def restated(pos, centres, radii, dims):
    """Yields per centre (members, band) as bool [n] on the CPU: d = ((dx dx) + dy dy) + dz dz in float64,
    one torch operation per product and per sum, so that each is rounded on its own; d <= r r."""
    p = pos.double()
    for c, r in zip(centres, radii):
        dx, dy = p[:, 0] - c[0], p[:, 1] - c[1]
        d = dx * dx
        d = d + dy * dy
        if dims == 3:
            dz = p[:, 2] - c[2]
            d = d + dz * dz
        r2 = torch.tensor(float(r), dtype=torch.float64)
        r2 = r2 * r2
        yield d <= r2, (d - r2).abs() <= BAND * r2


@pytest.mark.parametrize("dims", [3, 2])
def test_large_cloud_equals_the_float64_restatement(dims):
    n, B = 1 << 22, 64
    gen = torch.Generator().manual_seed(2200 + dims)
    pos = torch.rand(n, 3, generator=gen) * torch.tensor([60.0, 40.0, 8.0]) + torch.tensor([1153.25, 3907.5, 115.875])
    centres = (torch.rand(B, dims, generator=gen, dtype=torch.float64)
               * torch.tensor([60.0, 40.0, 8.0], dtype=torch.float64)[:dims]
               + torch.tensor([1153.25, 3907.5, 115.875], dtype=torch.float64)[:dims])
    centres[:8] = pos[torch.randint(0, n, (8,), generator=gen), :dims].double()      # centres on points
    radii = torch.rand(B, generator=gen, dtype=torch.float64) * 5.5 + 0.5
    radii[-1] = 0.0                                                                   # a centre off points: empty
    pos_dev = pos.to(DEV)
    ptr, idx = ops.radius_query(pos_dev, centres, radii, dims=dims)
    ptr2, idx2 = ops.radius_query(pos_dev, centres, radii, dims=dims)
    assert ptr.dtype == idx.dtype == torch.int64 and ptr.is_cuda and idx.is_cuda
    # the same call twice: identical bytes
    assert torch.equal(ptr, ptr2) and torch.equal(idx, idx2)
    ptr, idx = ptr.cpu(), idx.cpu()
    assert ptr.shape == (B + 1,) and int(ptr[0]) == 0 and int(ptr[-1]) == idx.shape[0]
    want = restated(pos, centres.tolist(), radii.tolist(), dims)
    members = excluded = 0
    exact_ptr, exact_idx = [0], []
    for b, (inside, band) in enumerate(want):
        got = idx[ptr[b]:ptr[b + 1]]
        assert bool((got[1:] > got[:-1]).all()), b                                    # ascending, distinct
        got_mask = torch.zeros(n, dtype=torch.bool)
        got_mask[got] = True
        assert torch.equal(got_mask | band, inside | band), b
        members += int(inside.sum())
        excluded += int(band.sum())
        exact_idx.append(torch.nonzero(inside).flatten())
        exact_ptr.append(exact_ptr[-1] + exact_idx[-1].shape[0])
    print(f"dims={dims}: {members} members, {excluded} pairs inside the 1e-9 band")
    assert members > 100000 and excluded <= 1e-6 * members
    if excluded == 0:
        assert ptr.tolist() == exact_ptr and torch.equal(idx, torch.cat(exact_idx))
    # one radius for all centres, and the centres split into several launches, give the same rows
    r = float(radii[3])
    p1, i1 = ops.radius_query(pos_dev, centres, r, dims=dims)
    budget = ops._RADIUS_TABLE_BYTES
    ops._RADIUS_TABLE_BYTES = 4 * ((n + 511) // 512) * 24                             # 24 centres per launch
    try:
        p2, i2 = ops.radius_query(pos_dev, centres.float().double().numpy(), r, dims=dims)
        p3, i3 = ops.radius_query(pos_dev, centres, radii, dims=dims)
    finally:
        ops._RADIUS_TABLE_BYTES = budget
    assert torch.equal(p3.cpu(), ptr) and torch.equal(i3.cpu(), idx)
    lo, hi = int(p1[3]), int(p1[4])
    assert torch.equal(i1[lo:hi].cpu(), idx[ptr[3]:ptr[4]])
    # float32-representable centres: the split call sees the same float64 values as an unsplit one
    p4, i4 = ops.radius_query(pos_dev, centres.float(), r, dims=dims)
    assert torch.equal(p2, p4) and torch.equal(i2, i4)


# ---------------------------------------------------------------------------------------------------------------
# the Grid* tilings
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", ["sampling_grid_sphere", "sampling_grid_cylinder"])
def test_grid_tilings_match_the_reference(name, device):
    g = load_golden(name)
    inp = inputs_of(g)
    cls = T.GridSphereSampling if name.endswith("sphere") else T.GridCylinderSampling
    data = to(inp, device)
    data.kd_tree = "a tree"
    samples = cls(float(g["radius"]), grid_size=float(g["grid_size"]), center=bool(g["center"]))(data)
    assert not hasattr(data, "kd_tree")                                       # delattr_kd_tree
    ptr = g["ptr"]
    assert isinstance(samples, list) and len(samples) == ptr.shape[0] - 1
    for b, s in enumerate(samples):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        check_sample(s, inp, g["idx"][lo:hi], g["out_pos"][lo:hi], f"{name}:{b}", device)
        check(s.center_label, g["center_label"][b:b + 1], f"{name}:{b}:center_label", device)
    assert torch.equal(data.pos.cpu(), inp["pos"])
    # a list input is processed element by element and flattened
    both = cls(float(g["radius"]), grid_size=float(g["grid_size"]), center=bool(g["center"]))(
        [to(inp, device), to(inp, device)])
    assert len(both) == 2 * len(samples)
    for s, s2 in zip(samples + samples, both):
        assert torch.equal(s.origin_id, s2.origin_id) and torch.equal(s.pos, s2.pos)


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
def test_grid_save_id_sphere_select_mapping_end_to_end():
    from test_gpu_transforms import scene, views_as_set
    from deepviewagg_amd.core.data_transform.multimodal.image import SelectMappingFromPointId
    _, sd, _ = scene()
    n = sd.mappings.num_groups
    # two points in each of n distinct voxels: the grid sampling leaves exactly the n points the mappings describe
    gen = torch.Generator().manual_seed(9)
    side = 1
    while side ** 3 < 2 * n:
        side += 1
    cells = torch.randperm(side ** 3, generator=gen)[:n]
    coords = torch.stack([cells % side, (cells // side) % side, cells // (side * side)], 1).float()
    size = 0.25
    pos = torch.cat([(coords + 0.2) * size, (coords - 0.2) * size])[torch.randperm(2 * n, generator=gen)]
    data = SimpleNamespace(pos=pos.to(DEV))
    data = G.GridSampling3D(size, mode="mean")(data)
    assert data.pos.shape[0] == n
    data = G.SaveOriginalPosId(key="mapping_index")(data)
    centre = data.pos[n // 2].cpu().numpy()
    radius = (0.3 * side + 0.0517) * size             # no voxel centre near the boundary (asserted below)
    voxel_pos = data.pos.cpu()
    data = T.SphereSampling(radius, centre, align_origin=False)(data)
    picked = data.mapping_index.clone()
    d = ((voxel_pos.double() - torch.from_numpy(centre).double()) ** 2).sum(1)
    near = (d - radius * radius).abs() <= 1e-9 * radius * radius
    assert not bool(near.any())
    assert torch.equal(picked.cpu(), torch.nonzero(d <= radius * radius).flatten()) and 0 < picked.shape[0] < n
    want = sd.select_points(picked, mode="pick")
    data, out = SelectMappingFromPointId()(data, sd)
    assert torch.equal(data.mapping_index.cpu(), torch.arange(picked.shape[0]))
    assert views_as_set(out.mappings) == views_as_set(want.mappings)
