"""SphereSampling / CylinderSampling / GridSphereSampling / GridCylinderSampling / Select without a GPU (reference
core/data_transform/transforms.py:99-232, :301-432): constructors, repr against the reference's recorded strings,
the drop-in names, the C-ABI argument checks of the dva_radius_* entries, the checks ops.radius_query makes before any
device work, and the committed fixtures tests/golden/sampling_*.npz (tools/gen_golden_sampling.py)."""
import importlib
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from deepviewagg_amd import _lib, ops
from deepviewagg_amd.core.data_transform import transforms as T

NAMES = ["CylinderSampling", "GridCylinderSampling", "GridSphereSampling", "Select", "SphereSampling"]


def test_public_namespace_is_the_five_classes():
    assert sorted(k for k in vars(T) if not k.startswith("_")) == NAMES
    for cls in (T.SphereSampling, T.CylinderSampling, T.GridSphereSampling, T.GridCylinderSampling):
        assert cls.KDTREE_KEY == "kd_tree"


def test_sampler_constructors():
    s = T.SphereSampling(0.5, np.array([1.0, 2.0, 3.0]))
    assert s._radius == 0.5 and s._align_origin is True
    assert isinstance(s._centre, np.ndarray) and s._centre.shape == (1, 3) and s._centre.dtype == np.float64
    s = T.SphereSampling(2, torch.tensor([[1.5, -2.25, 3.0]]), align_origin=False)
    assert s._centre.shape == (1, 3) and s._centre.dtype == np.float32 and s._align_origin is False
    assert T.SphereSampling(1.0, [0.0, 0.0, 0.0])._centre.shape == (1, 3)


def test_cylinder_centre_loses_its_z():
    c = T.CylinderSampling(6.0, np.array([1153.25, 3907.5, 115.875]))
    assert c._centre.shape == (1, 2) and c._centre.tolist() == [[1153.25, 3907.5]]
    c = T.CylinderSampling(6.0, torch.tensor([1.0, 2.0, 3.0]))
    assert c._centre.tolist() == [[1.0, 2.0]]
    c = T.CylinderSampling(6.0, np.array([1.0, 2.0]))                # an xy centre stays as it is
    assert c._centre.tolist() == [[1.0, 2.0]]


def test_grid_constructors_take_numbers_and_strings():
    g = T.GridSphereSampling("2 * 0.5", grid_size="1.5")
    assert g._radius == 1.0 and g._grid_sampling._grid_size == 1.5 and g._grid_sampling._mode == "mean"
    assert g._delattr_kd_tree is True and g._center is True
    g = T.GridCylinderSampling("6", grid_size="6 / 2", delattr_kd_tree=False, center=False)
    assert g._radius == 6 and g._grid_sampling._grid_size == 3.0
    assert g._delattr_kd_tree is False and g._center is False
    g = T.GridSphereSampling(2, grid_size=1)
    assert isinstance(g._radius, float) and g._radius == 2.0 and g._grid_sampling._grid_size == 1.0
    assert T.GridSphereSampling(2.0)._grid_sampling._grid_size == 2.0            # no grid size: the radius
    assert T.GridCylinderSampling(3.0, grid_size=None)._grid_sampling._grid_size == 3.0
    with pytest.raises(Exception):
        T.GridSphereSampling("__import__('os').getcwd()")                        # arithmetic only


def test_repr_equals_the_references_strings():
    want = {k: str(v) for k, v in load_golden("sampling_repr").items()}
    got = {
        "sphere": repr(T.SphereSampling(0.5, np.array([1.0, 2.0, 3.0]))),
        "sphere_plain": repr(T.SphereSampling(2, np.array([[1.5, -2.25, 3.0]], dtype=np.float32), align_origin=False)),
        "cylinder": repr(T.CylinderSampling(6.0, np.array([1153.25, 3907.5, 115.875]))),
        "cylinder_xy": repr(T.CylinderSampling(6, torch.tensor([1.0, 2.0]), align_origin=False)),
        "grid_sphere": repr(T.GridSphereSampling("2 * 0.5", grid_size="1.5")),
        "grid_sphere_plain": repr(T.GridSphereSampling(2, grid_size=1, center=False)),
        "grid_cylinder": repr(T.GridCylinderSampling(3.0, grid_size=2.0)),
        "grid_cylinder_plain": repr(T.GridCylinderSampling("6", grid_size="6 / 2", center=False)),
    }
    assert got == want
    assert want["sphere"] == "SphereSampling(radius=0.5, center=[[1. 2. 3.]], align_origin=True)"


def test_select_without_a_device():
    n = 10
    data = SimpleNamespace(pos=torch.rand(n, 3), y=torch.arange(n), meta=torch.tensor([1.0, 2.0]), kd_tree=object(),
                           name="room")
    idx = torch.tensor([7, 2, 2, 9])
    out = T.Select(idx)(data)
    assert isinstance(out, SimpleNamespace) and not hasattr(out, "kd_tree") and out.name == "room"
    assert torch.equal(out.pos, data.pos[idx]) and torch.equal(out.y, idx)
    assert torch.equal(out.meta, data.meta) and out.meta is not data.meta
    mask = torch.arange(n) % 2 == 0
    out = T.Select(mask)({"pos": data.pos, "y": data.y})
    assert isinstance(out, dict) and torch.equal(out["y"], torch.arange(0, n, 2))


def _clear():
    for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
        del sys.modules[k]


@pytest.mark.parametrize("patch_existing", [False, True])
def test_dropin_resolves_the_five_names_on_both_paths(patch_existing):
    from deepviewagg_amd import dropin
    from deepviewagg_amd.core.data_transform import grid_transform as G
    _clear()
    try:
        names = dropin.install(patch_existing=patch_existing)
        assert "torch_points3d.core.data_transform.transforms" in names
        mod = importlib.import_module("torch_points3d.core.data_transform.transforms")
        pkg = importlib.import_module("torch_points3d.core.data_transform")
        for k in NAMES:
            assert getattr(mod, k) is getattr(T, k), k
            assert getattr(pkg, k) is getattr(T, k), k
        # the earlier aliases are unchanged
        assert pkg.GridSampling3D is G.GridSampling3D and pkg.SaveOriginalPosId is G.SaveOriginalPosId
        # a config-style lookup by name on the package (instantiate_transform)
        tr = getattr(pkg, "GridSphereSampling")(radius="2", grid_size="1")
        assert repr(tr) == "GridSphereSampling(radius=2, center=True)"
    finally:
        _clear()


def test_abi_entries_reject_bad_arguments():
    lib = _lib.load()
    assert lib.dva_version() >= 310
    one, big = 1, 1 << 30
    assert lib.dva_radius_query_workspace_bytes(-1, 4) == -1
    assert lib.dva_radius_query_workspace_bytes(4, -1) == -1
    assert lib.dva_radius_query_workspace_bytes(1 << 31, 4) == -2
    assert lib.dva_radius_query_workspace_bytes((1 << 31) - 1, 1) > 0
    assert lib.dva_radius_query_workspace_bytes(0, 0) >= 256
    assert lib.dva_radius_query_workspace_bytes(1 << 20, 64) >= (1 << 20) // 512 * 64 * 4
    # null pointers
    assert lib.dva_radius_count(None, 10, None, 4, 3, 1.0, None, None, None, 0, None) == -1
    assert lib.dva_radius_count(None, 10, one, 4, 3, 1.0, None, one, one, big, None) == -1     # pos
    assert lib.dva_radius_count(one, 10, None, 4, 3, 1.0, None, one, one, big, None) == -1     # centres
    assert lib.dva_radius_count(one, 10, one, 4, 3, 1.0, None, None, one, big, None) == -1     # ptr
    assert lib.dva_radius_count(one, 10, one, 4, 3, 1.0, None, one, None, big, None) == -1     # workspace
    # negative sizes, dims outside {2, 3}, a negative or NaN radius, a workspace that is too small, n >= 2^31
    assert lib.dva_radius_count(one, -1, one, 4, 3, 1.0, None, one, one, big, None) == -1
    assert lib.dva_radius_count(one, 10, one, -4, 3, 1.0, None, one, one, big, None) == -1
    for dims in (0, 1, 4, -3):
        assert lib.dva_radius_count(one, 10, one, 4, dims, 1.0, None, one, one, big, None) == -1
        assert lib.dva_radius_fill(one, 10, one, 4, dims, 1.0, None, one, one, 8, one, big, None) == -1
    assert lib.dva_radius_count(one, 10, one, 4, 3, -1.0, None, one, one, big, None) == -1
    assert lib.dva_radius_count(one, 10, one, 4, 3, float("nan"), None, one, one, big, None) == -1
    assert lib.dva_radius_count(one, 10, one, 4, 3, 1.0, None, one, one, 8, None) == -1
    assert lib.dva_radius_count(one, 1 << 31, one, 4, 3, 1.0, None, one, one, big, None) == -2
    assert lib.dva_radius_fill(None, 10, None, 4, 3, 1.0, None, None, None, 0, None, 0, None) == -1
    assert lib.dva_radius_fill(one, 10, one, 4, 3, 1.0, None, None, one, 8, one, big, None) == -1    # ptr
    assert lib.dva_radius_fill(one, 10, one, 4, 3, 1.0, None, one, None, 8, one, big, None) == -1    # idx
    assert lib.dva_radius_fill(one, 10, one, 4, 3, 1.0, None, one, one, -8, one, big, None) == -1    # capacity
    assert lib.dva_radius_fill(one, -10, one, 4, 3, 1.0, None, one, one, 8, one, big, None) == -1
    assert lib.dva_radius_fill(one, 10, one, 4, 2, 1.0, None, one, one, 8, one, 8, None) == -1       # workspace


def test_radius_query_checks_its_arguments_before_device_work():
    pos = torch.rand(10, 3)
    c = np.zeros((2, 3))
    with pytest.raises(TypeError, match="float64.*float32"):
        ops.radius_query(pos.double(), c, 1.0)
    with pytest.raises(TypeError, match="float32"):
        ops.radius_query(pos.half(), c, 1.0)
    with pytest.raises(ValueError, match="dims"):
        ops.radius_query(pos, c, 1.0, dims=4)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        ops.radius_query(pos[:, :2], c, 1.0)
    with pytest.raises(ValueError, match="centres"):
        ops.radius_query(pos, c, 1.0, dims=2)                        # [B, 3] centres for the cylinder
    with pytest.raises(ValueError, match="radius"):
        ops.radius_query(pos, c, -1.0)
    with pytest.raises(ValueError, match="radius"):
        ops.radius_query(pos, c, float("nan"))
    with pytest.raises(ValueError, match="radii"):
        ops.radius_query(pos, c, np.array([1.0, 2.0, 3.0]))


FIXTURE_CASES = {
    "sampling_sphere_room": ["on_aligned", "on_plain", "off_aligned", "off_plain", "off32_aligned"],
    "sampling_cylinder_street": ["xyz_aligned", "xyz_plain", "xy_aligned", "on_plain", "on32_aligned"],
    "sampling_edges": ["sphere_boundary", "sphere_boundary_shifted", "cylinder_boundary", "cylinder_boundary_shifted",
                       "sphere_empty", "sphere_all"],
}


def test_fixtures_load_with_the_documented_keys():
    for name, cases in FIXTURE_CASES.items():
        g = load_golden(name)
        assert [str(c) for c in g["cases"]] == cases, name
        n = g["in_pos"].shape[0]
        assert g["in_pos"].dtype == np.float32 and g["in_rgb"].shape == (n, 3) and g["in_y"].shape == (n,)
        assert g["in_meta"].shape == (3,)
        for c in cases:
            idx = g[f"{c}_idx"]
            assert idx.dtype == np.int64 and (np.diff(idx) > 0).all(), (name, c)       # sorted, distinct
            assert g[f"{c}_out_pos"].shape == (idx.shape[0], 3) and g[f"{c}_out_pos"].dtype == np.float32
            assert g[f"{c}_radius"].dtype == np.float64 and g[f"{c}_align"].dtype == np.bool_
    assert float(load_golden("sampling_cylinder_street")["in_pos"][:, 1].min()) > 3000          # world offsets
    e = load_golden("sampling_edges")
    n = e["in_pos"].shape[0]
    assert e["sphere_empty_idx"].shape[0] == 0 and np.array_equal(e["sphere_all_idx"], np.arange(n))
    assert (e["in_pos"] * 8 == np.round(e["in_pos"] * 8)).all()                                 # the 1/8 lattice
    for c in FIXTURE_CASES["sampling_edges"][:4]:
        assert int(e[f"{c}_on_boundary"]) >= 20, c
        # the boundary points are members: the lattice makes the float64 distance exact
        cen = e[f"{c}_centre"][:2] if c.startswith("cylinder") else e[f"{c}_centre"]
        d = ((e["in_pos"][:, :cen.shape[0]].astype(np.float64) - cen) ** 2).sum(1)
        r2 = float(e[f"{c}_radius"]) ** 2
        on = np.nonzero(d == r2)[0]
        assert on.shape[0] == int(e[f"{c}_on_boundary"]) and np.isin(on, e[f"{c}_idx"]).all(), c
        assert np.array_equal(np.nonzero(d <= r2)[0], e[f"{c}_idx"]), c
    for name in ("sampling_grid_sphere", "sampling_grid_cylinder"):
        g = load_golden(name)
        B = g["centres"].shape[0]
        assert g["ptr"].shape == (B + 1,) and g["ptr"][-1] == g["idx"].shape[0] == g["out_pos"].shape[0]
        assert g["center_label"].shape == (B,) and g["center_label"].dtype == np.int64 and B >= 10
        assert g["centres"].dtype == np.float32 and g["centres"].shape[1] == (3 if name.endswith("sphere") else 2)
    cyl = load_golden("sampling_grid_cylinder")["centres"]
    assert np.array_equal(cyl, np.unique(cyl, axis=0))                                          # sorted unique xy rows
