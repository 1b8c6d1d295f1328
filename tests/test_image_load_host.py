"""CPU tests of the image loading path: the numpy restatement (tests/image_load_ref.py) against the fixture
tests/golden/image_load.npz (the reference's own read_images and NonStaticMask over Pillow) and against live Pillow, the
product's host-side pieces (coefficient tables, pass plans, argument checks, the PIL route, the transforms' state edits)
against the restatement, and the drop-in names."""
import importlib
import json
import sys

import numpy as np
import pytest
import torch

import image_load_ref as R
from conftest import load_golden

GOLD = load_golden("image_load")
CASES = {c["name"]: c for c in json.loads(str(GOLD["cases"]))}
MASK_CASES = {c["name"]: c for c in json.loads(str(GOLD["mask_cases"]))}
ONE_SIZE = [n for n in CASES if n != "two_sizes"]


def case_idx(spec):
    if spec is None or isinstance(spec, int):
        return spec
    if spec[0] == "slice":
        return slice(*spec[1:])
    return torch.tensor(spec)


def case_sources(c):
    src = [GOLD[f"src/{n}"] for n in c["sources"]]
    idx = case_idx(c.get("idx"))
    if idx is not None:
        sel = np.arange(len(src))[idx.numpy() if torch.is_tensor(idx) else idx]
        src = [src[i] for i in np.atleast_1d(sel)]
    return src


def case_args(c, tensors=True):
    kw = dict(downscale=c.get("downscale"))
    if c.get("rollings") is not None:
        kw["rollings"] = torch.tensor(c["rollings"], dtype=torch.int64) if tensors else c["rollings"]
    if c.get("crop_size") is not None:
        kw["crop_size"] = tuple(c["crop_size"])
        kw["crop_offsets"] = torch.tensor(c["crop_offsets"], dtype=torch.int64) if tensors else c["crop_offsets"]
    return kw


def setting(tmp_path, names, **kw):
    from deepviewagg_amd.core.multimodal.image import SameSettingImageData
    paths = []
    for i, n in enumerate(names):
        paths.append(str(tmp_path / f"{i}_{n}.npy"))
        np.save(paths[-1], GOLD[f"src/{n}"])
    return SameSettingImageData(path=np.array(paths), pos=torch.zeros(len(names), 3), **kw)


def test_fixture_is_the_references_and_holds_arrays_only():
    assert str(GOLD["producer"]) == "reference" and str(GOLD["pillow_version"])
    assert len(CASES) >= 25 and sorted(MASK_CASES) == ["mask_n1", "mask_n2", "mask_n5"]
    assert all(GOLD[f"out/{n}"].dtype == np.uint8 and GOLD[f"out/{n}"].shape[1] == 3 for n in CASES)
    assert {int(GOLD[f"src/{n}"].min()) for n in ["chk"]} == {0} and int(GOLD["src/chk"].max()) == 255


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_fixture(name):
    c = CASES[name]
    got = R.read_images(case_sources(c), c["size"], **case_args(c, tensors=False))
    assert got.dtype == np.uint8 and np.array_equal(got, GOLD[f"out/{name}"])


def test_restatement_shows_the_identity_of_a_box_at_scale_one():
    """A box that is not the whole image, resized to its own size, goes through the resample: its table is one tap of
    weight 2^22 at the output's own source pixel, so the result is the crop."""
    for in_size, start, length in ((77, 37, 40), (19, 8, 11), (40, 0, 17), (40, 23, 17)):
        ksize, bounds, kk = R.coefficients(in_size, start, start + length, length)
        rows = np.arange(length)
        assert ksize == 5 and np.array_equal(kk[rows, start + rows - bounds[:, 0]], np.full(length, 1 << 22))
        assert np.count_nonzero(kk) == length
    assert np.array_equal(GOLD["out/crop"], GOLD["out/crop_ds1"])


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for _ in range(40):
        H, W = (int(v) for v in rng.integers(1, 60, 2))
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if rng.random() < 0.3:
            a = (a > 127).astype(np.uint8) * 255
        size = tuple(int(v) for v in rng.integers(1, 80, 2))
        box = None
        if rng.random() < 0.5:
            x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
            box = (x0, y0, int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1)))
        want = np.asarray(Image.fromarray(a).resize(size, box=box))
        assert np.array_equal(R.resize(a, size, box), want), (H, W, size, box)


def test_table_builder_equals_the_restatement():
    from deepviewagg_amd import ops
    rng = np.random.default_rng(11)
    cases = [(301, 0, 301, 77), (67, 0, 67, 19), (160, 0, 160, 20), (40, 0, 40, 100), (77, 37, 77, 16), (19, 8, 19, 4),
             (40, 0.5, 33.75, 11), (5, 0, 5, 1100), (11, 0, 11, 1), (1, 0, 1, 7), (2048, 0, 2048, 1024)]
    for _ in range(60):
        n = int(rng.integers(1, 400))
        a = int(rng.integers(0, n))
        cases.append((n, a, int(rng.integers(a + 1, n + 1)), int(rng.integers(1, 400))))
    for in_size, in0, in1, out in cases:
        ksize, bounds, kk = R.coefficients(in_size, in0, in1, out)
        coeffs, b = ops.image_resample_tables(in_size, in0, in1, out)
        assert coeffs.dtype == np.int32 and b.dtype == np.int32 and coeffs.shape == (out, ksize)
        assert np.array_equal(coeffs, kk) and np.array_equal(b, bounds), (in_size, in0, in1, out)


@pytest.mark.parametrize("name", ONE_SIZE)
def test_pass_plan_equals_the_fixture(name):
    """The passes ops.read_images_u8 would launch (tables, table index, shifts, periods), run through the restatement of
    one launch: the roll and the crop folded into the passes give the reference's bytes, in one to four passes."""
    from deepviewagg_amd import ops
    c = CASES[name]
    cur = np.stack(case_sources(c))
    kw = case_args(c)
    passes, (eh, ew) = ops._read_images_plan(cur.shape[0], cur.shape[1], cur.shape[2], tuple(c["size"]), kw.get("rollings"),
                                             kw.get("crop_size"), kw.get("crop_offsets"), kw.get("downscale"))
    assert 1 <= len(passes) <= 4
    for p in passes:
        cur = R.resample_pass(cur, p.axis, p.coeffs, p.bounds, p.table_index, p.shifts, p.periods, p.out_hw)
    assert cur.shape[1:3] == (eh, ew)
    assert np.array_equal(cur.transpose(0, 3, 1, 2), GOLD[f"out/{name}"])


def test_plan_argument_checks():
    from deepviewagg_amd import ops
    plan = ops._read_images_plan
    with pytest.raises(ValueError):
        plan(1, 30, 40, (40, 30), None, (20, 10), None, None)                       # crop_size without crop_offsets
    with pytest.raises(ValueError):
        plan(1, 30, 40, (40, 30), None, (41, 10), torch.zeros((1, 2), dtype=torch.int64), None)
    with pytest.raises(ValueError):
        plan(1, 30, 40, (40, 30), None, (20, 10), torch.tensor([[21, 0]]), None)    # the box leaves the image
    with pytest.raises(ValueError):
        plan(1, 30, 40, (40, 30), None, None, None, 0.5)
    with pytest.raises(TypeError):
        plan(1, 30, 40, (40, 30), torch.zeros(1, dtype=torch.int32), None, None, None)
    with pytest.raises(ValueError):
        plan(2, 30, 40, (40, 30), torch.zeros(1, dtype=torch.int64), None, None, None)


def test_entries_validate_before_any_hip_call():
    from deepviewagg_amd import _lib
    lib = _lib.load()
    assert lib.dva_version() >= 328
    ok = [None, 1, 4, 4, 48, 12, 3, 1, None, 4, 4, 48, 12, 3, 1, 0, None, None, 1, 4, 5, None, None, 0, 0, 0, None]

    def call(**changes):
        names = ["src", "B", "src_h", "src_w", "sb", "sy", "sx", "sc", "dst", "dst_h", "dst_w", "db", "dy", "dx", "dc", "axis",
                 "coeffs", "bounds", "n_tables", "table_rows", "ksize", "table_index", "shifts", "out_period",
                 "src_period", "other_period", "stream"]
        args = list(ok)
        for k, v in changes.items():
            args[names.index(k)] = v
        return lib.dva_image_resample_u8(*args)
    assert call() == -1                                       # null pointers
    assert call(B=0) == 0                                     # nothing to do
    assert call(B=-1) == -1 and call(axis=2) == -1 and call(ksize=0) == -1 and call(n_tables=0) == -1
    assert call(B=0, sx=0) == -1 and call(B=0, dc=0) == -1
    assert call(B=0, src_period=3) == -1                      # a period is the length of its axis
    assert call(B=0, src_period=4) == 0 and call(B=0, other_period=4) == 0
    assert call(B=0, out_period=5) == -1 and call(B=0, out_period=4) == 0
    assert call(src_w=1 << 31) == -2 or call(src_w=1 << 31) == -1
    assert lib.dva_image_resample_workspace_bytes(2, 3, 5) >= 90 and lib.dva_image_resample_workspace_bytes(-1, 3, 5) == -1
    assert lib.dva_image_resample_workspace_bytes(1 << 20, 1 << 20, 1 << 20) == -2
    assert lib.dva_image_nonstatic_mask(None, 2, 4, 4, None, None) == -1
    assert lib.dva_image_nonstatic_mask(None, 0, 4, 4, None, None) == -1
    assert lib.dva_image_nonstatic_mask(None, 2, 0, 4, None, None) == 0


def test_ops_refuse_host_tensors():
    from deepviewagg_amd import ops
    from deepviewagg_amd._lib import DvaError
    with pytest.raises(DvaError):
        ops.image_resample(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), (2, 2))
    with pytest.raises(DvaError):
        ops.read_images_u8(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), (2, 2))
    with pytest.raises(DvaError):
        ops.image_nonstatic_mask(torch.zeros((2, 3, 4, 4), dtype=torch.uint8))


@pytest.mark.parametrize("name", list(CASES))
def test_host_route_reproduces_the_fixture(name, tmp_path):
    """SameSettingImageData.read_images on the host (the PIL composition) from .npy sources."""
    pytest.importorskip("PIL")
    c = CASES[name]
    got = setting(tmp_path, c["sources"]).read_images(idx=case_idx(c.get("idx")), size=tuple(c["size"]), **case_args(c))
    assert got.dtype == torch.uint8 and not got.is_cuda
    assert np.array_equal(got.numpy(), GOLD[f"out/{name}"])


def test_decode_hook(tmp_path):
    """decode_image is looked up in the module at every call; .npy paths need no PIL."""
    from deepviewagg_amd.core.multimodal import image as I
    a = GOLD["src/d0"]
    np.save(str(tmp_path / "a.npy"), a)
    assert np.array_equal(I.decode_image(str(tmp_path / "a.npy")), a)
    np.save(str(tmp_path / "bad.npy"), a[..., 0])
    with pytest.raises(ValueError):
        I.decode_image(str(tmp_path / "bad.npy"))
    images = I.SameSettingImageData(path=np.array(["x://1", "x://2"]), pos=torch.zeros(2, 3), ref_size=(11, 9))
    seen = []
    held = I.decode_image
    I.decode_image = lambda p: (seen.append(p), a)[1]
    try:
        pytest.importorskip("PIL")
        images.load()
    finally:
        I.decode_image = held
    assert seen == ["x://1", "x://2"] and torch.equal(images.x, torch.from_numpy(a).permute(2, 0, 1).expand(2, -1, -1, -1))


def test_load_images_edits_the_state_as_the_reference(tmp_path):
    pytest.importorskip("PIL")
    from deepviewagg_amd.core.data_transform.multimodal.image import LoadImages
    c = CASES["crop_ds2"]
    images = setting(tmp_path, c["sources"])
    assert images.ref_size == (512, 256)
    images.rollings = torch.tensor(c["rollings"], dtype=torch.int64)
    tr = LoadImages(ref_size=tuple(c["size"]), crop_size=tuple(c["crop_size"]),
                    crop_offsets=torch.tensor(c["crop_offsets"], dtype=torch.int64), downscale=2)
    assert repr(tr).startswith("LoadImages(ref_size=(77, 19), crop_size=(40, 11)")
    data = object()
    d, out = tr(data, images)
    assert d is data and out is images
    assert out.ref_size == (77, 19) and out.crop_size == (40, 11) and out.downscale == 2 and out.img_size == (20, 5)
    assert torch.equal(out.crop_offsets, torch.tensor(c["crop_offsets"]))
    assert np.array_equal(out.x.numpy(), GOLD["out/crop_ds2"])
    # the state is frozen once x exists, as in the reference
    with pytest.raises(AssertionError):
        out.crop_size = (30, 11)
    with pytest.raises(AssertionError):
        out.crop_offsets = torch.zeros((3, 2), dtype=torch.int64)
    out.crop_size = (40, 11)                                   # the same value is accepted
    # defaults: nothing edited, load() at the object's own state
    plain = setting(tmp_path, ["b0", "b1"], ref_size=(40, 30))
    LoadImages()(None, plain)
    assert plain.ref_size == (40, 30) and plain.downscale == 1
    assert np.array_equal(plain.x.numpy(), np.stack([GOLD["src/b0"], GOLD["src/b1"]]).transpose(0, 3, 1, 2))
    # through an ImageData
    from deepviewagg_amd.core.multimodal.image import ImageData
    both = ImageData([setting(tmp_path, ["b0"], ref_size=(40, 30)), setting(tmp_path, ["d0"], ref_size=(11, 9))])
    _, both = LoadImages()(None, both)
    assert [tuple(x.shape) for x in both.x] == [(1, 3, 30, 40), (1, 3, 9, 11)]
    assert both.load() is both


@pytest.mark.parametrize("name", list(MASK_CASES))
def test_nonstatic_mask_on_the_host_matches_the_reference(name, tmp_path):
    pytest.importorskip("PIL")
    from deepviewagg_amd.core.data_transform.multimodal.image import NonStaticMask
    c = MASK_CASES[name]
    images = setting(tmp_path, c["sources"])
    tr = NonStaticMask(ref_size=tuple(c["ref_size"]), proj_upscale=c["proj_upscale"], n_sample=c["n_sample"])
    torch.manual_seed(c["seed"])
    _, out = tr(None, images)
    assert out.ref_size == tuple(c["ref_size"]) and out.proj_upscale == c["proj_upscale"] and out.crop_size == out.ref_size
    assert out.mask.dtype == torch.bool and tuple(out.mask.shape) == out.proj_size == (16, 12)
    assert np.array_equal(out.mask.numpy(), GOLD[f"mask/{name}"])
    assert torch.equal(torch.get_rng_state(), torch.from_numpy(GOLD[f"rng/{name}"]))
    if c["n_sample"] == 1:
        assert bool(out.mask.all())


def test_restatement_mask_equals_the_fixture():
    """The views the reference drew are recovered from the generator; the restated mask over them is the fixture's."""
    for name, c in MASK_CASES.items():
        if c["n_sample"] < 2:
            continue
        torch.manual_seed(c["seed"])
        idx = torch.multinomial(torch.arange(len(c["sources"]), dtype=torch.float), c["n_sample"])
        assert 0 not in idx.tolist()                              # view 0 has weight 0
        views = np.stack([GOLD[f"src/{c['sources'][i]}"] for i in idx.tolist()]).transpose(0, 3, 1, 2)
        assert np.array_equal(R.nonstatic_mask(views), GOLD[f"mask/{name}"])


# the image transforms the reference's four multimodal data configs name (s3disfused-sparse, scannet-sparse,
# kitti360-sparse, kitti360-sparse-nodynamicbatch), pre_transform and per-sample chains
CONFIG_IMAGE_TRANSFORMS = ["LoadImages", "NonStaticMask", "MapImages", "NeighborhoodBasedMappingFeatures",
                           "SelectMappingFromPointId", "PickImagesFromMappingArea", "PickImagesFromMemoryCredit",
                           "JitterMappingFeatures", "CenterRoll", "CropImageGroups", "ColorJitter", "RandomHorizontalFlip",
                           "ToFloatImage", "Normalize", "ToImageData"]


def test_dropin_resolves_every_image_transform_of_the_shipped_configs():
    from deepviewagg_amd import dropin
    from deepviewagg_amd.core.data_transform.multimodal import image as ours
    for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
        del sys.modules[k]
    try:
        dropin.install(patch_existing=False)
        mod = importlib.import_module("torch_points3d.core.data_transform.multimodal.image")
        for name in CONFIG_IMAGE_TRANSFORMS:
            assert getattr(mod, name) is getattr(ours, name), name
        from torch_points3d.core.data_transform.multimodal.image import LoadImages, NonStaticMask
        assert LoadImages is ours.LoadImages and NonStaticMask is ours.NonStaticMask
        data_mod = importlib.import_module("torch_points3d.core.multimodal.image")
        assert hasattr(data_mod.SameSettingImageData, "read_images") and hasattr(data_mod.SameSettingImageData, "load")
        assert hasattr(data_mod.ImageData, "load") and callable(data_mod.decode_image)
    finally:
        for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
            del sys.modules[k]
