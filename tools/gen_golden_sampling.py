#!/usr/bin/env python
"""Write tests/golden/sampling_*.npz by running the REFERENCE's own SphereSampling / CylinderSampling /
GridSphereSampling / GridCylinderSampling (torch_points3d/core/data_transform/transforms.py:99-232, :301-405) over
the real scikit-learn KDTree.

TEST INFRASTRUCTURE: needs the reference source tree (argument 1, default ../reference next to this repository) and
scikit-learn; nothing in the package, the tests, smoke() or bench.py runs it; the tests read the committed .npz files.

The reference's transforms.py is loaded as a single file next to its grid_transform.py (loaded as in
tools/gen_golden_grid_sampling.py, whose stand-ins of torch_cluster / torch_scatter are reused).  The other modules it
imports at the top and that the five classes never touch are empty stand-ins.  The shim Data of oracle/shims gains
``clone`` (the Grid* transforms grid-sample a clone).

The reference returns the members of a sample in its KD-tree's order, which is unspecified.  Every input carries
``origin_id = arange(N)``; the tool asserts that every per-point output attribute equals the input rows that the
output's ``origin_id`` names (``pos``: after adding the float32 centre back is NOT assumed; the shifted ``pos`` is
stored), and stores the member indices SORTED, with the shifted ``pos`` in that order.

Files (seeded):
  sampling_sphere_room      ~20 k room points; centres on and off points, align_origin both ways
  sampling_cylinder_street  ~20 k street points at KITTI-360 world offsets; 2- and 3-vector centres
  sampling_edges            a 1/8 lattice with radius 25/8 (many points exactly on the boundary, sphere and cylinder),
                            a sphere that is empty and a sphere that holds every point
  sampling_grid_sphere      GridSphereSampling of a small labelled room: the list of samples
  sampling_grid_cylinder    GridCylinderSampling of a small labelled street
  sampling_repr             the reference's repr strings of the four classes

Conditions on the inputs (asserted; a scene or centre that fails is redrawn from the next seed):
  - outside the lattice scene no (point, centre) pair has |d - r^2| <= 1e-9 r^2, d = ((dx dx) + dy dy) + dz dz in
    float64: no other rounding of the distance can decide a membership;
  - for every Grid centre the nearest point beats the second nearest by more than 1e-5 relative in squared distance:
    float32 against float64 and tie order cannot decide ``center_label``;
  - in every query the sorted ``query_radius`` result equals the predicate d <= r r.

Usage:  python tools/gen_golden_sampling.py [REFERENCE_ROOT]
"""
import importlib.util
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden_grid_sampling as GG  # noqa: E402  (also puts oracle/shims on sys.path)

BAND = 1e-9
MARGIN = 1e-5


def load_reference_transforms(ref_root):
    G, GridData = GG.load_reference_grid_transform(ref_root)

    class Data(GridData):
        def clone(self):
            return Data(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})

    def module(name, is_pkg=False, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        if is_pkg and not hasattr(m, "__path__"):
            m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    unused = lambda *a, **k: None                                            # noqa: E731
    sys.modules["torch_geometric.data"].Data = Data
    module("torch_geometric.nn.pool", is_pkg=True)
    module("torch_geometric.nn.pool.pool", pool_pos=unused, pool_batch=unused)
    module("torch_geometric.transforms", FixedPoints=object)
    module("torch_points_kernels", is_pkg=True)
    module("torch_points_kernels.points_cpu", ball_query=unused)
    module("torch_points3d.datasets", is_pkg=True)
    module("torch_points3d.datasets.multiscale_data", MultiScaleData=object)
    module("torch_points3d.datasets.registration", is_pkg=True)
    module("torch_points3d.datasets.registration.pair", Pair=object)
    module("torch_points3d.utils", is_pkg=True, is_iterable=unused)
    module("torch_points3d.utils.transform_utils", SamplingStrategy=object)
    module("torch_points3d.utils.config", is_list=unused)
    module("torch_points3d.core.data_transform.features", Random3AxisRotation=object)
    name = "torch_points3d.core.data_transform.transforms"
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ref_root, "torch_points3d", "core", "data_transform", "transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod, Data


# ---------------------------------------------------------------------------------------------------------------
# the predicate and the conditions on the inputs
# ---------------------------------------------------------------------------------------------------------------
def sq_dist(pos, centre):
    """d = ((dx dx) + dy dy) + dz dz in float64, every operation rounded on its own; 2 columns for the cylinder."""
    c = np.asarray(centre, dtype=np.float64).reshape(-1)
    p = pos.numpy().astype(np.float64)
    dx, dy = p[:, 0] - c[0], p[:, 1] - c[1]
    d = dx * dx + dy * dy
    if c.shape[0] == 3:
        dz = p[:, 2] - c[2]
        d = d + dz * dz
    return d


def clear_of_band(pos, centre, radius):
    r2 = float(radius) * float(radius)
    return not bool((np.abs(sq_dist(pos, centre) - r2) <= BAND * r2).any())


def nearest_is_clear(pos, centre):
    d = np.sort(sq_dist(pos, centre))
    return d.shape[0] < 2 or (d[1] - d[0]) > MARGIN * d[1]


def members_of(pos, centre, radius):
    return np.nonzero(sq_dist(pos, centre) <= float(radius) * float(radius))[0]


def make_inputs(pos, gen, with_y=True):
    n = pos.shape[0]
    inputs = dict(pos=pos, rgb=torch.randint(0, 16, (n, 3), generator=gen).float() / 15,
                  origin_id=torch.arange(n), meta=torch.tensor([3.0, 1.0, 4.0]))
    if with_y:
        inputs["y"] = torch.randint(0, 9, (n,), generator=gen)
    return inputs


def run_sampler(Data, sampler, inputs):
    """The reference's sample -> (sorted member indices, shifted pos in that order); asserts the rest."""
    n = inputs["pos"].shape[0]
    out = sampler(Data(**{k: v.clone() for k, v in inputs.items()}))
    assert not hasattr(out, "kd_tree")
    ind = out.origin_id
    order = torch.argsort(ind)
    ind = ind[order]
    assert ind.shape[0] == torch.unique(ind).shape[0]
    for k, v in inputs.items():
        got = getattr(out, k)
        if k == "pos":
            assert got.shape == (ind.shape[0], 3) and got.dtype == v.dtype
        elif v.shape[0] == n:
            assert torch.equal(got[order], v[ind]), k
        else:
            assert torch.equal(got, v), k
    return ind, out.pos[order]


def store_inputs(arrays, inputs, prefix="in_"):
    for k, v in inputs.items():
        if k != "origin_id":                       # arange(N): the tests rebuild it
            arrays[prefix + k] = v


# ---------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------
def gen_single(T, Data, gen, name, pos, cls, cases):
    """cases: (tag, centre or a callable gen -> centre, radius, align_origin).  A centre drawn by a callable is redrawn
    until no pair lies in the band."""
    inputs = make_inputs(pos, gen)
    arrays = {}
    store_inputs(arrays, inputs)
    tags = []
    for tag, centre, radius, align in cases:
        for _ in range(100):
            c = np.asarray(centre(gen) if callable(centre) else centre)
            if clear_of_band(pos, c[:2] if cls is T.CylinderSampling else c, radius):
                break
            assert callable(centre), (name, tag, "a fixed centre has a pair in the band")
        else:
            raise AssertionError((name, tag))
        ind, out_pos = run_sampler(Data, cls(radius, c, align_origin=align), inputs)
        want = members_of(pos, c[:2] if cls is T.CylinderSampling else c, radius)
        assert np.array_equal(ind.numpy(), want), (name, tag)
        arrays[f"{tag}_centre"] = c
        arrays[f"{tag}_radius"] = np.float64(radius)
        arrays[f"{tag}_align"] = np.bool_(align)
        arrays[f"{tag}_idx"] = ind
        arrays[f"{tag}_out_pos"] = out_pos
        tags.append(tag)
        print(f"    {name}:{tag}  {ind.shape[0]} members")
    arrays["cases"] = np.array(tags)
    GG.save(name, arrays)


def gen_room(T, Data, gen):
    pos = GG.room_scene(gen, n=20000)
    on = lambda g: pos[int(torch.randint(0, pos.shape[0], (1,), generator=g))].numpy()            # noqa: E731
    off = lambda g: (torch.rand(3, generator=g, dtype=torch.float64)                               # noqa: E731
                     * torch.tensor([4.0, 3.0, 2.5], dtype=torch.float64)).numpy()
    gen_single(T, Data, gen, "sampling_sphere_room", pos, T.SphereSampling, [
        ("on_aligned", on, 0.5, True),
        ("on_plain", on, 0.75, False),
        ("off_aligned", off, 0.8, True),
        ("off_plain", off, 0.6, False),
        ("off32_aligned", lambda g: off(g).astype(np.float32), 0.7, True),
    ])


def gen_street(T, Data, gen):
    pos = GG.street_scene(gen, n=20000)
    lo = GG.KITTI_OFFSET.numpy()
    off = lambda g: lo + (torch.rand(3, generator=g, dtype=torch.float64)                          # noqa: E731
                          * torch.tensor([12.0, 6.0, 4.0], dtype=torch.float64)).numpy()
    on = lambda g: pos[int(torch.randint(0, pos.shape[0], (1,), generator=g))].numpy()            # noqa: E731
    gen_single(T, Data, gen, "sampling_cylinder_street", pos, T.CylinderSampling, [
        ("xyz_aligned", off, 2.0, True),
        ("xyz_plain", off, 1.5, False),
        ("xy_aligned", lambda g: off(g)[:2], 2.5, True),
        ("on_plain", on, 1.0, False),
        ("on32_aligned", lambda g: on(g)[:2], 3.0, True),
    ])


def gen_edges(T, Data, gen):
    """1/8 lattice: every coordinate, difference, product and sum is exact, so the boundary test is decided by the
    comparison alone."""
    ax = torch.arange(-26, 27, dtype=torch.float32) / 8
    az = torch.arange(-2, 3, dtype=torch.float32) / 8
    pos = torch.stack(torch.meshgrid(ax, ax, az, indexing="ij"), -1).reshape(-1, 3)
    pos = pos[torch.randperm(pos.shape[0], generator=gen)].contiguous()
    inputs = make_inputs(pos, gen)
    arrays = {}
    store_inputs(arrays, inputs)
    r = 25 / 8
    cases = [
        ("sphere_boundary", T.SphereSampling, np.array([0.0, 0.0, 0.0]), r, True),
        ("sphere_boundary_shifted", T.SphereSampling, np.array([0.125, -0.125, 0.125]), r, False),
        ("cylinder_boundary", T.CylinderSampling, np.array([0.0, 0.0]), r, True),
        ("cylinder_boundary_shifted", T.CylinderSampling, np.array([-0.125, 0.125, 7.0]), r, False),
        ("sphere_empty", T.SphereSampling, np.array([40.0, 40.0, 40.0]), 1.0, True),
        ("sphere_all", T.SphereSampling, np.array([0.25, 0.25, 0.0]), 50.0, True),
    ]
    tags = []
    for tag, cls, c, radius, align in cases:
        cq = c[:2] if cls is T.CylinderSampling else c
        d = sq_dist(pos, cq)
        on_boundary = int((d == radius * radius).sum())
        if "boundary" in tag:          # 20 lattice points on the sphere, 20 x 5 on the cylinder
            assert on_boundary >= (100 if cls is T.CylinderSampling else 20), (tag, on_boundary)
        ind, out_pos = run_sampler(Data, cls(radius, c, align_origin=align), inputs)
        assert np.array_equal(ind.numpy(), members_of(pos, cq, radius)), tag
        if tag == "sphere_empty":
            assert ind.shape[0] == 0
        if tag == "sphere_all":
            assert ind.shape[0] == pos.shape[0]
        arrays[f"{tag}_centre"] = c
        arrays[f"{tag}_radius"] = np.float64(radius)
        arrays[f"{tag}_align"] = np.bool_(align)
        arrays[f"{tag}_idx"] = ind
        arrays[f"{tag}_out_pos"] = out_pos
        arrays[f"{tag}_on_boundary"] = np.int64(on_boundary)
        tags.append(tag)
        print(f"    sampling_edges:{tag}  {ind.shape[0]} members, {on_boundary} on the boundary")
    arrays["cases"] = np.array(tags)
    GG.save("sampling_edges", arrays)


def small_room(gen, n):
    return (torch.rand(n, 3, generator=gen) * torch.tensor([4.0, 3.0, 2.5])).contiguous()


def small_street(gen, n):
    xyz = torch.rand(n, 3, generator=gen, dtype=torch.float64) * torch.tensor([12.0, 6.0, 3.0], dtype=torch.float64)
    return (xyz + GG.KITTI_OFFSET).float().contiguous()


def gen_grid(T, Data, name, cls, scene, n, radius, grid_size, center, seed):
    """Redraws the scene from the next seed until the reference's own centres satisfy both conditions."""
    cyl = cls is T.GridCylinderSampling
    while True:
        gen = torch.Generator().manual_seed(seed)
        pos = scene(gen, n)
        inputs = make_inputs(pos, gen)
        data = Data(**{k: v.clone() for k, v in inputs.items()})
        samples = cls(radius, grid_size=grid_size, center=center)(data)
        centres, ok = [], True
        ptr, idx, out_pos, labels = [0], [], [], []
        for s in samples:
            ind = s.origin_id
            order = torch.argsort(ind)
            ind = ind[order]
            for k, v in inputs.items():
                if k != "pos" and v.shape[0] == n:
                    assert torch.equal(getattr(s, k)[order], v[ind]), k
            assert torch.equal(s.meta, inputs["meta"])
            idx.append(ind)
            out_pos.append(s.pos[order])
            labels.append(s.center_label.reshape(-1))
            ptr.append(ptr[-1] + ind.shape[0])
        # the centres themselves: the reference's grid sampling of a clone, as its _process does
        grid = T.GridSampling3D(size=grid_size if grid_size else radius)(
            Data(**{k: v.clone() for k, v in inputs.items()}))
        centres = np.unique(grid.pos[:, :-1], axis=0) if cyl else np.asarray(grid.pos)
        assert len(samples) == centres.shape[0]
        search = pos.clone()
        if cyl:
            search = search[:, :2]
        for b, c in enumerate(centres):
            ok = ok and clear_of_band(search, c, radius) and nearest_is_clear(search, c)
            assert np.array_equal(idx[b].numpy(), members_of(search, c, radius)), (name, b)
            near = int(np.argmin(sq_dist(search, c)))
            assert int(labels[b]) == int(inputs["y"][near]), (name, b)
        if ok:
            break
        seed += 1
    arrays = {}
    store_inputs(arrays, inputs)
    arrays.update(radius=np.float64(radius), grid_size=np.float64(grid_size), center=np.bool_(center),
                  seed=np.int64(seed), centres=centres, ptr=np.asarray(ptr, dtype=np.int64), idx=torch.cat(idx),
                  out_pos=torch.cat(out_pos), center_label=torch.cat(labels))
    print(f"    {name}: {len(samples)} samples, {ptr[-1]} members, seed {seed}")
    GG.save(name, arrays)


def gen_repr(T):
    arrays = {
        "sphere": repr(T.SphereSampling(0.5, np.array([1.0, 2.0, 3.0]))),
        "sphere_plain": repr(T.SphereSampling(2, np.array([[1.5, -2.25, 3.0]], dtype=np.float32), align_origin=False)),
        "cylinder": repr(T.CylinderSampling(6.0, np.array([1153.25, 3907.5, 115.875]))),
        "cylinder_xy": repr(T.CylinderSampling(6, torch.tensor([1.0, 2.0]), align_origin=False)),
        "grid_sphere": repr(T.GridSphereSampling("2 * 0.5", grid_size="1.5")),
        "grid_sphere_plain": repr(T.GridSphereSampling(2, grid_size=1, center=False)),
        "grid_cylinder": repr(T.GridCylinderSampling(3.0, grid_size=2.0)),
        "grid_cylinder_plain": repr(T.GridCylinderSampling("6", grid_size="6 / 2", center=False)),
    }
    GG.save("sampling_repr", {k: np.array(v) for k, v in arrays.items()})


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    T, Data = load_reference_transforms(ref_root)
    gen = torch.Generator().manual_seed(1916)
    gen_room(T, Data, gen)
    gen_street(T, Data, gen)
    gen_edges(T, Data, gen)
    gen_grid(T, Data, "sampling_grid_sphere", T.GridSphereSampling, small_room, 3000, 1.0, 1.5, True, 41)
    gen_grid(T, Data, "sampling_grid_cylinder", T.GridCylinderSampling, small_street, 4000, 2.0, 3.0, False, 51)
    gen_repr(T)


if __name__ == "__main__":
    main()
