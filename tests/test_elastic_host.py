"""ElasticDistortion without a GPU (reference core/data_transform/grid_transform.py:194-256): the class's constructor,
repr and gate, the drop-in names, the C-ABI argument checks of the dva_minmax3_* / dva_elastic_* entries, and the
committed fixtures tests/golden/elastic_*.npz (tools/gen_golden_elastic.py)."""
import glob
import importlib
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from deepviewagg_amd import _lib

FIXTURES = ("elastic_room", "elastic_street", "elastic_planar", "elastic_single", "elastic_lattice", "elastic_gate")
COMMON_KEYS = ("pos", "seed_random", "seed_numpy", "granularity", "magnitude", "applied", "levels", "repr")
LEVEL_KEYS = ("noise_dim", "ax0", "ax1", "ax2", "noise", "field", "out_pos")


def test_class_imports_without_a_device_and_has_the_reference_repr():
    from deepviewagg_amd.core.data_transform.grid_transform import ElasticDistortion
    from deepviewagg_amd.core.data_transform import grid_transform as G
    assert G.ElasticDistortion is ElasticDistortion
    assert ElasticDistortion.__name__ == "ElasticDistortion" and ElasticDistortion.__module__ == G.__name__
    e = ElasticDistortion()
    assert (e._apply_distorsion, e._granularity, e._magnitude) == (True, [0.2, 0.8], [0.4, 1.6])
    assert repr(e) == "ElasticDistortion(apply_distorsion=True, granularity=[0.2, 0.8], magnitude=[0.4, 1.6])"
    for name in FIXTURES:
        g = load_golden(name)
        e = ElasticDistortion(granularity=g["granularity"].tolist(), magnitude=g["magnitude"].tolist())
        assert repr(e) == str(g["repr"]), name
    e = ElasticDistortion(apply_distorsion=False, granularity=[0.5], magnitude=[2])
    assert repr(e) == "ElasticDistortion(apply_distorsion=False, granularity=[0.5], magnitude=[2])"
    assert callable(ElasticDistortion.elastic_distortion)
    with pytest.raises(AttributeError):
        G.NoSuchTransform


def test_constructor_rejects_lists_of_unequal_length():
    from deepviewagg_amd.core.data_transform.grid_transform import ElasticDistortion
    with pytest.raises(AssertionError):
        ElasticDistortion(granularity=[0.2, 0.8], magnitude=[0.4])
    with pytest.raises(AssertionError):
        ElasticDistortion(granularity=[0.2], magnitude=[0.4, 1.6])


def test_skipped_transform_touches_nothing_and_needs_no_device():
    """apply_distorsion=False and a seed that fails the 0.95 gate return the data as it is, before any device work."""
    from deepviewagg_amd.core.data_transform.grid_transform import ElasticDistortion
    g = load_golden("elastic_gate")
    assert not bool(g["applied"]) and int(g["levels"]) == 0
    pos = torch.from_numpy(g["pos"])
    data = SimpleNamespace(pos=pos, y=torch.arange(pos.shape[0]))
    np.random.seed(int(g["seed_numpy"]))
    before = np.random.get_state()
    random.seed(int(g["seed_random"]))
    out = ElasticDistortion()(data)
    assert out is data and out.pos is pos
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    random.seed(int(g["seed_random"]))
    assert not random.random() < 0.95                       # the seed is one the gate rejects
    state = random.getstate()
    out = ElasticDistortion(apply_distorsion=False)(data)   # no draw from `random` either
    assert out is data and out.pos is pos and random.getstate() == state


def _clear():
    for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
        del sys.modules[k]


@pytest.mark.parametrize("patch_existing", [False, True])
def test_dropin_resolves_the_name_on_module_and_package(patch_existing):
    from deepviewagg_amd import dropin
    from deepviewagg_amd.core.data_transform import grid_transform as G
    _clear()
    try:
        dropin.install(patch_existing=patch_existing)
        mod = importlib.import_module("torch_points3d.core.data_transform.grid_transform")
        pkg = importlib.import_module("torch_points3d.core.data_transform")
        assert mod.ElasticDistortion is G.ElasticDistortion
        assert pkg.ElasticDistortion is G.ElasticDistortion
        assert pkg.GridSampling3D is G.GridSampling3D                      # the earlier names are unchanged
        tr = getattr(pkg, "ElasticDistortion")(granularity=[0.2], magnitude=[0.4])
        assert repr(tr) == "ElasticDistortion(apply_distorsion=True, granularity=[0.2], magnitude=[0.4])"
        # install() leaves the eagerly listed names of our module alone
        assert sorted(k for k in vars(G) if not k.startswith("_")) == ["GridSampling3D", "SaveOriginalPosId"]
    finally:
        _clear()


def test_dropin_patches_an_importable_reference_module_by_name():
    """With a torch_points3d of its own already imported, install() overwrites its ElasticDistortion."""
    import types
    from deepviewagg_amd import dropin
    from deepviewagg_amd.core.data_transform import grid_transform as G
    _clear()
    try:
        for name in ("torch_points3d", "torch_points3d.core", "torch_points3d.core.data_transform"):
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
        theirs = types.ModuleType("torch_points3d.core.data_transform.grid_transform")
        theirs.ElasticDistortion = object
        theirs.GridSampling3D = object
        sys.modules[theirs.__name__] = theirs
        sys.modules["torch_points3d.core.data_transform"].grid_transform = theirs
        dropin.install(patch_existing=True)
        assert theirs.ElasticDistortion is G.ElasticDistortion and theirs.GridSampling3D is G.GridSampling3D
        assert sys.modules["torch_points3d.core.data_transform"].ElasticDistortion is G.ElasticDistortion
    finally:
        _clear()


def test_abi_entries_reject_bad_arguments():
    lib = _lib.load()
    assert lib.dva_version() >= 311
    one = 1
    big = 1 << 30
    assert lib.dva_minmax3_workspace_bytes() >= 256 * 6 * 4
    assert lib.dva_minmax3_f32(None, 10, one, one, big, None) == -1
    assert lib.dva_minmax3_f32(one, 0, one, one, big, None) == -1               # an empty cloud has no bounds
    assert lib.dva_minmax3_f32(one, -1, one, one, big, None) == -1
    assert lib.dva_minmax3_f32(one, 10, None, one, big, None) == -1
    assert lib.dva_minmax3_f32(one, 10, one, None, big, None) == -1
    assert lib.dva_minmax3_f32(one, 10, one, one, 16, None) == -1               # workspace
    assert lib.dva_minmax3_f32(one, 1 << 30, one, one, big, None) == -2         # 3 n >= 2^31
    assert lib.dva_elastic_workspace_bytes(0, 3, 3) == -1
    assert lib.dva_elastic_workspace_bytes(3, -1, 3) == -1
    assert lib.dva_elastic_workspace_bytes(1 << 12, 1 << 12, 1 << 6) == -2      # 3 * 2^30 elements
    assert lib.dva_elastic_workspace_bytes(1 << 40, 1 << 40, 1 << 40) == -2
    assert lib.dva_elastic_workspace_bytes(22, 17, 15) >= 2 * 22 * 17 * 15 * 3 * 4
    assert lib.dva_elastic_smooth(None, 3, 3, 3, one, one, big, None) == -1
    assert lib.dva_elastic_smooth(one, 3, 3, 3, None, one, big, None) == -1
    assert lib.dva_elastic_smooth(one, 3, 3, 3, one, None, big, None) == -1
    assert lib.dva_elastic_smooth(one, 3, 0, 3, one, one, big, None) == -1
    assert lib.dva_elastic_smooth(one, 3, 3, 3, one, one, 64, None) == -1       # workspace
    assert lib.dva_elastic_smooth(one, 1 << 12, 1 << 12, 1 << 6, one, one, big, None) == -2
    assert lib.dva_elastic_displace(None, 10, one, one, 3, 3, 3, 0.4, one, None) == -1
    assert lib.dva_elastic_displace(one, 10, None, one, 3, 3, 3, 0.4, one, None) == -1
    assert lib.dva_elastic_displace(one, 10, one, None, 3, 3, 3, 0.4, one, None) == -1
    assert lib.dva_elastic_displace(one, 10, one, one, 3, 3, 3, 0.4, None, None) == -1
    assert lib.dva_elastic_displace(one, -1, one, one, 3, 3, 3, 0.4, one, None) == -1
    assert lib.dva_elastic_displace(one, 10, one, one, 3, 1, 3, 0.4, one, None) == -1      # a cell needs two knots
    assert lib.dva_elastic_displace(one, 1 << 30, one, one, 3, 3, 3, 0.4, one, None) == -2
    assert lib.dva_elastic_displace(None, 0, one, one, 3, 3, 3, 0.4, None, None) == 0      # no points: nothing to do


def test_ops_reject_bad_arguments_before_any_device_work():
    from deepviewagg_amd import ops
    with pytest.raises(TypeError, match="float32"):
        ops.elastic_smooth(np.zeros((3, 3, 3, 3)))
    with pytest.raises(ValueError, match=r"\[Dx, Dy, Dz, 3\]"):
        ops.elastic_smooth(np.zeros((3, 3, 3), dtype=np.float32))
    with pytest.raises(TypeError, match="float32"):
        ops.elastic_distortion(torch.zeros(4, 3, dtype=torch.float64), 0.2, 0.4)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        ops.elastic_displace(torch.zeros(4, 2), np.zeros((3, 3, 3, 3), dtype=np.float32), [np.arange(3.0)] * 3, 0.4)


def test_every_fixture_carries_the_documented_keys_and_data_only():
    files = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "elastic_*.npz")))
    assert files == sorted(FIXTURES)
    for name in files:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 700 * 1024, name
        g = load_golden(name)                                   # allow_pickle=False: arrays of plain data only
        levels = int(g["levels"])
        want = list(COMMON_KEYS) + [f"l{l}_{k}" for l in range(levels) for k in LEVEL_KEYS]
        assert sorted(g) == sorted(want), name
        for k, v in g.items():
            assert v.dtype.kind in "fiubU", (name, k, v.dtype)
        n = g["pos"].shape[0]
        assert g["pos"].dtype == np.float32 and g["pos"].shape == (n, 3)
        assert g["granularity"].shape == g["magnitude"].shape and g["granularity"].dtype == np.float64
        assert levels == (g["granularity"].shape[0] if bool(g["applied"]) else 0), name
        random.seed(int(g["seed_random"]))
        assert (random.random() < 0.95) == bool(g["applied"]), name
        for l in range(levels):
            dim = tuple(int(d) for d in g[f"l{l}_noise_dim"])
            assert g[f"l{l}_noise"].shape == dim + (3,) and g[f"l{l}_noise"].dtype == np.float32
            assert g[f"l{l}_field"].shape == dim + (3,) and g[f"l{l}_field"].dtype == np.float32
            for k in range(3):
                ax = g[f"l{l}_ax{k}"]
                assert ax.dtype == np.float64 and ax.shape == (dim[k],) and (np.diff(ax) > 0).all()
            assert g[f"l{l}_out_pos"].shape == (n, 3) and g[f"l{l}_out_pos"].dtype == np.float32
        # the recorded noise is what the recorded numpy seed draws, level after level
        np.random.seed(int(g["seed_numpy"]))
        for l in range(levels):
            drawn = np.random.randn(*g[f"l{l}_noise"].shape).astype(np.float32)
            assert drawn.tobytes() == g[f"l{l}_noise"].tobytes(), (name, l)


def test_fixture_scenes_are_the_documented_ones():
    room = load_golden("elastic_room")
    assert 15000 <= room["pos"].shape[0] <= 25000 and room["granularity"].tolist() == [0.2, 0.8]
    assert room["magnitude"].tolist() == [0.4, 1.6] and int(room["levels"]) == 2
    street = load_golden("elastic_street")
    assert float(street["pos"][:, 1].min()) > 3000 and float(street["pos"][:, 0].min()) > 1000      # world offsets
    planar = load_golden("elastic_planar")
    assert float(planar["pos"][:, 2].min()) == float(planar["pos"][:, 2].max()) and int(planar["l0_noise_dim"][2]) == 3
    single = load_golden("elastic_single")
    assert single["pos"].shape[0] == 1 and single["l0_noise_dim"].tolist() == [3, 3, 3]
    assert single["l1_noise_dim"].tolist() == [3, 3, 3]
    lat = load_golden("elastic_lattice")
    for k in range(3):                                       # every point on a knot, the largest on knot d - 2
        ax, x = lat[f"l0_ax{k}"], lat["pos"][:, k].astype(np.float64)
        assert np.isin(x, ax).all() and float(x.max()) == float(ax[-2]) and float(x.min()) == float(ax[1])
    # the first level moved every cloud, by less than the noise's magnitude
    for name in FIXTURES[:-1]:
        g = load_golden(name)
        shift = np.abs(g["l0_out_pos"].astype(np.float64) - g["pos"]).max()
        assert 0 < shift < float(g["magnitude"][0]), (name, shift)
