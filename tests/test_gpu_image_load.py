"""-m gpu: the image loading ops (csrc/image_load.hip) against the fixture tests/golden/image_load.npz -- what the
reference's own read_images and NonStaticMask gave over Pillow -- and against the numpy restatement
tests/image_load_ref.py.  Every comparison is torch.equal on uint8 / bool: there is no tolerance.  Needs neither PIL nor
the reference: sources come as arrays or as .npy files in tmp_path."""
import ctypes
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import image_load_ref as R
from conftest import load_golden, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = load_golden("image_load")
CASES = {c["name"]: c for c in json.loads(str(GOLD["cases"]))}
MASK_CASES = {c["name"]: c for c in json.loads(str(GOLD["mask_cases"]))}
ONE_SIZE = [n for n in CASES if n != "two_sizes"]


def ops():
    from deepviewagg_amd import ops as o
    return o


def same(got, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (got.dtype, got.shape, want.dtype, want.shape)
    assert torch.equal(got.cpu(), want)


def case_idx(spec):
    if spec is None or isinstance(spec, int):
        return spec
    if spec[0] == "slice":
        return slice(*spec[1:])
    return torch.tensor(spec)


def case_args(c):
    kw = dict(downscale=c.get("downscale"))
    if c.get("rollings") is not None:
        kw["rollings"] = torch.tensor(c["rollings"], dtype=torch.int64)
    if c.get("crop_size") is not None:
        kw["crop_size"] = tuple(c["crop_size"])
        kw["crop_offsets"] = torch.tensor(c["crop_offsets"], dtype=torch.int64)
    return kw


def setting(tmp_path, names, device=DEV, **kw):
    """A SameSettingImageData whose 'files' are the fixture's decoded sources as .npy."""
    from deepviewagg_amd.core.multimodal.image import SameSettingImageData
    paths = []
    for i, n in enumerate(names):
        paths.append(str(tmp_path / f"{i}_{n}.npy"))
        np.save(paths[-1], GOLD[f"src/{n}"])
    return SameSettingImageData(path=np.array(paths), pos=torch.zeros(len(names), 3, device=device), **kw)


@pytest.mark.parametrize("name", ONE_SIZE)
def test_read_images_u8_matches_the_reference(name):
    """ops.read_images_u8 on the decoded sources == the reference's read_images over Pillow, byte for byte: non-integer
    and x8 downscales (ksize 33), upscale, one pass skipped, the copy, an output wider than a workgroup's 1024 pixels,
    widths 1 / 3 / 5, the 0 / 255 checkerboard (both ends of the clamp), three rollings (negative, >= W), three crop
    offsets (each border), downscale None / 1 / 2 / 2.5."""
    c = CASES[name]
    src = np.stack([GOLD[f"src/{n}"] for n in c["sources"]])
    idx = case_idx(c.get("idx"))
    if idx is not None:
        src = src[np.atleast_1d(np.arange(len(src))[idx if not torch.is_tensor(idx) else idx.numpy()])]
    got = ops().read_images_u8(t(src, DEV), tuple(c["size"]), **case_args(c))
    same(got, GOLD[f"out/{name}"])


@pytest.mark.parametrize("name", ["two_sizes", "idx_int", "idx_tensor", "idx_slice", "crop_ds2p5", "same"])
def test_read_images_of_the_class_matches_the_reference(name, tmp_path):
    """SameSettingImageData.read_images on the device: idx as int, tensor and slice, two source sizes in one call (one
    batch each, placed in idx order)."""
    c = CASES[name]
    images = setting(tmp_path, c["sources"])
    got = images.read_images(idx=case_idx(c.get("idx")), size=tuple(c["size"]), **case_args(c))
    assert got.is_cuda
    same(got, GOLD[f"out/{name}"])


def test_read_images_launch_counts():
    """One to four launches: only the passes Pillow would run, and one copy pass when it would run none."""
    o = ops()
    src = t(GOLD["src/b0"][None], DEV)
    seen = []

    class Timer:
        def launch(self, name, nbytes):
            seen.append(name)
            return o._NO_TIMER
    held, o.TIMER = o.TIMER, Timer()
    try:
        for kw, n in ((dict(size=(40, 30)), 1), (dict(size=(40, 30), downscale=1), 1), (dict(size=(100, 30)), 1),
                      (dict(size=(100, 77)), 2), (dict(size=(100, 77), downscale=2), 4),
                      (dict(size=(40, 30), crop_size=(20, 30), crop_offsets=torch.tensor([[3, 0]]), downscale=1), 1)):
            del seen[:]
            o.read_images_u8(src, **kw)
            assert seen == ["image_resample"] * n, (kw, seen)
    finally:
        o.TIMER = held


BOXES = [((40, 30), (21, 13), None), ((40, 30), (20, 10), (3, 4, 23, 14)), ((40, 30), (9, 7), (5, 2, 40, 30)),
         ((40, 30), (11, 9), (0.5, 1.25, 33.75, 29.5)), ((37, 23), (37, 23), (0, 0, 37, 23)),
         ((37, 23), (36, 23), (1, 0, 37, 23)), ((37, 23), (37, 5), (0, 2, 37, 7))]


@pytest.mark.parametrize("src_size,size,box", BOXES)
def test_image_resample_matches_the_restatement(src_size, size, box):
    """ops.image_resample == Image.resize(size, box=box) as restated: integer and fractional boxes, a box at scale 1."""
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (2, src_size[1], src_size[0], 3), dtype=np.uint8)
    want = np.stack([R.resize(a, size, box) for a in src]).transpose(0, 3, 1, 2)
    same(ops().image_resample(t(src, DEV), size, box), want)


@pytest.mark.parametrize("width", [1, 2, 3, 4, 5, 6, 7, 9, 13])
def test_every_row_alignment(width):
    """Rows of 3 w bytes start at every address mod 4 and the 4-pixel chunks end in every tail length: both passes, both
    destination layouts, packed loads and stores against the restatement."""
    rng = np.random.default_rng(width)
    src = rng.integers(0, 256, (3, 7, width, 3), dtype=np.uint8)
    for size in ((width, 5), (width + 2, 7), (width + 3, 4), (max(1, width - 1), 9)):
        want = np.stack([R.resize(a, size) for a in src]).transpose(0, 3, 1, 2)
        same(ops().image_resample(t(src, DEV), size), want)
    rolls = torch.tensor([1, -2, width + 1])
    want = R.read_images(list(src), (width, 7), rolls.numpy(), None, None, 2 if width > 1 else 1)
    same(ops().read_images_u8(t(src, DEV), (width, 7), rollings=rolls, downscale=2 if width > 1 else 1), want)


@pytest.mark.parametrize("axis", [0, 1])
def test_resample_entry_with_planar_strides(axis):
    """The C entry reads any byte strides: a planar [B, 3, h, w] source into an HWC destination, with all three shifts
    and their periods, against the restatement of one launch."""
    from deepviewagg_amd import _lib
    o = ops()
    rng = np.random.default_rng(5 + axis)
    B, h, w = 2, 11, 14
    src = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    n_in = w if axis == 0 else h
    n_out = 6
    tables = [o.image_resample_tables(n_in, s, s + 9, n_out + 3) for s in (0, 2)]
    coeffs, bounds = np.stack([a for a, _ in tables]), np.stack([b for _, b in tables])
    table_index = np.array([1, 0], dtype=np.int32)
    shifts = np.array([[2, 3, 5], [1, 9, 0]], dtype=np.int32)
    n_other_src = h if axis == 0 else w
    periods = (n_out + 3, n_in, n_other_src)
    out_hw = (7, n_out) if axis == 0 else (n_out, 9)
    want = R.resample_pass(src, axis, coeffs, bounds, table_index, shifts, periods, out_hw)
    planar = t(src.transpose(0, 3, 1, 2), DEV)
    dst = torch.zeros((B,) + out_hw + (3,), dtype=torch.uint8, device=DEV)
    dev = [t(a, DEV) for a in (coeffs, bounds, table_index, shifts)]
    rc = _lib.load().dva_image_resample_u8(
        _lib.ptr(planar), B, h, w, 3 * h * w, w, 1, h * w, _lib.ptr(dst), out_hw[0], out_hw[1],
        out_hw[0] * out_hw[1] * 3, out_hw[1] * 3, 3, 1, axis, _lib.ptr(dev[0]), _lib.ptr(dev[1]), 2, n_out + 3,
        coeffs.shape[2], _lib.ptr(dev[2]), _lib.ptr(dev[3]), *periods, _lib.stream_of(dst))
    assert rc == 0
    same(dst, want)


def test_load_images_transform_on_the_device(tmp_path):
    """LoadImages edits the state as the reference and load() fills x on the device: the fixture's crop + downscale 2."""
    from deepviewagg_amd.core.data_transform.multimodal.image import LoadImages
    c = CASES["crop_ds2"]
    images = setting(tmp_path, c["sources"])
    images.rollings = torch.tensor(c["rollings"], dtype=torch.int64, device=DEV)
    tr = LoadImages(ref_size=tuple(c["size"]), crop_size=tuple(c["crop_size"]),
                    crop_offsets=torch.tensor(c["crop_offsets"], dtype=torch.int64), downscale=2)
    _, out = tr(None, images)
    assert out is images and out.ref_size == (77, 19) and out.crop_size == (40, 11) and out.downscale == 2
    assert out.img_size == (20, 5) and out.crop_offsets.is_cuda and out.x.is_cuda
    same(out.x, GOLD["out/crop_ds2"])


def test_host_route_gives_the_same_bytes(tmp_path):
    """LOAD_ON_DEVICE off: the PIL composition on the host, the yardstick of the device route."""
    pytest.importorskip("PIL")
    from deepviewagg_amd.core.multimodal.image import SameSettingImageData
    c = CASES["crop_ds2p5"]
    images = setting(tmp_path, c["sources"])
    held = SameSettingImageData.LOAD_ON_DEVICE
    SameSettingImageData.LOAD_ON_DEVICE = False
    try:
        host = images.read_images(size=tuple(c["size"]), **case_args(c))
    finally:
        SameSettingImageData.LOAD_ON_DEVICE = held
    assert not host.is_cuda
    same(images.read_images(size=tuple(c["size"]), **case_args(c)), host.contiguous().numpy())


@pytest.mark.parametrize("shape", [(2, 12, 16), (3, 70, 131), (5, 64, 64), (1, 9, 5)])
def test_nonstatic_mask_op_matches_the_restatement(shape):
    """mask[x, y] over more than one tile, odd sizes, n = 1 (all False); pixels differing in one, two and three
    channels."""
    rng = np.random.default_rng(shape[1])
    n, H, W = shape
    imgs = np.repeat(rng.integers(0, 256, (1, 3, H, W), dtype=np.uint8), n, axis=0)
    for i in range(1, n):
        for channels in (1, 2, 3):
            ys, xs = rng.integers(0, H, 25), rng.integers(0, W, 25)
            imgs[i, :channels, ys, xs] ^= 0xFF
    got = ops().image_nonstatic_mask(t(imgs, DEV))
    assert got.dtype == torch.bool and tuple(got.shape) == (W, H)
    same(got, R.nonstatic_mask(imgs))


@pytest.mark.parametrize("name", list(MASK_CASES))
def test_nonstatic_mask_transform_matches_the_reference(name, tmp_path):
    """NonStaticMask with n_sample 1, 2 and 5: the reference's mask in its [W, H] orientation, the same views drawn, the
    same host generator state afterwards."""
    from deepviewagg_amd.core.data_transform.multimodal.image import NonStaticMask
    c = MASK_CASES[name]
    images = setting(tmp_path, c["sources"])
    tr = NonStaticMask(ref_size=tuple(c["ref_size"]), proj_upscale=c["proj_upscale"], n_sample=c["n_sample"])
    torch.manual_seed(c["seed"])
    _, out = tr(None, images)
    assert out.ref_size == tuple(c["ref_size"]) and out.proj_upscale == c["proj_upscale"]
    assert tuple(out.mask.shape) == out.proj_size == (16, 12) and out.mask.is_cuda
    same(out.mask, GOLD[f"mask/{name}"])
    assert torch.equal(torch.get_rng_state(), torch.from_numpy(GOLD[f"rng/{name}"]))


def test_nonstatic_mask_feeds_map_images(tmp_path):
    """NonStaticMask -> MapImages on the toy scene of mapping_build.npz: views that differ everywhere give the all-True
    mask and the reference's mapping unchanged; views that are static on the left half map no pixel there."""
    from deepviewagg_amd.core.data_transform.multimodal import MapImages
    from deepviewagg_amd.core.data_transform.multimodal.image import NonStaticMask
    from deepviewagg_amd.core.multimodal.image import SameSettingImageData
    from test_gpu_data import mapping_equals
    g = load_golden("mapping_build")
    ref_size, up = tuple(int(v) for v in g["ref_size"]), int(g["proj_upscale"])
    Wp, Hp = ref_size[0] * up, ref_size[1] * up
    cams = t(g["cams"])
    n = g["xyz"].shape[0]
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (Hp, Wp, 3), dtype=np.uint8)

    def run(static_left):
        paths = []
        for i in range(len(cams)):
            a = base.copy()
            a[:, (Wp // 2 if static_left else 0):] += np.uint8(i)            # view i differs from view 0 by i, mod 256
            paths.append(str(tmp_path / f"{int(static_left)}_{i}.npy"))
            np.save(paths[-1], a)
        images = SameSettingImageData(path=np.array(paths), pos=cams.to(DEV), opk=torch.zeros(len(cams), 3, device=DEV),
                                      ref_size=ref_size, proj_upscale=up)
        data = SimpleNamespace(pos=t(g["xyz"]), mapping_index=torch.arange(n), linearity=t(g["linearity"]),
                               planarity=t(g["planarity"]), scattering=t(g["scattering"]), norm=t(g["normals"]))
        torch.manual_seed(1)
        _, images = NonStaticMask(ref_size=ref_size, proj_upscale=up, n_sample=3)(data, images)
        mask = images.mask.clone()
        tr = MapImages(method="SplattingVisibility", r_max=10.0, r_min=0.2, voxel=0.05, k_swell=1.0, d_swell=1000,
                       exact=True)
        return mask, tr(data, images)[1]
    mask, out = run(False)
    assert tuple(mask.shape) == (Wp, Hp) and bool(mask.all())
    mapping_equals(out.mappings, g)
    mask, out = run(True)
    assert not bool(mask[:Wp // 2].any()) and bool(mask[Wp // 2:].all())
    assert out.mappings.pixels.shape[0] > 0 and int(out.mappings.pixels[:, 0].min()) >= ref_size[0] // 2
