"""-m gpu: every branch the batched visibility build (dva_visibility_batch) picks by image size, survivor count and camera
model, held to the C oracle and to the single-image build (dva_visibility).

Tolerances are those of tests/test_gpu_mapping.py: idx / x / y / depth bit for bit against the oracle, float projections
within 1e-9 px, mapping features within 2.5e-7; a batch's rows equal the single-image build under torch.equal.  The
scenes and the preconditions that say they reach their branch are in tests/mapping_scenes.py; each test asserts them
(S.check_*) before it compares.
"""
import numpy as np
import pytest
import torch

import mapping_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROW_KEYS = ("idx", "x", "y", "depth", "features", "x_proj", "y_proj")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture
def single_image_kernels():
    """Single-camera calls on the single-image kernels of dva_visibility (64-bit atomic z-buffer plane), not on a batch of
    one: the two implementations check each other."""
    from deepviewagg_amd.core.multimodal import visibility as V
    old, V.SINGLE_VIA_BATCH = V.SINGLE_VIA_BATCH, False
    yield
    V.SINGLE_VIA_BATCH = old


class Run:
    """One scene on the device: the model, the uploaded cloud and cameras, batched and single builds."""

    def __init__(self, scene, exact, with_attrs=False):
        self.scene, self.exact, self.with_attrs = scene, exact, with_attrs
        self.model = S.model_of(scene, exact)
        self.xyz = dev(scene.xyz)
        self.pos = dev(scene.img_xyz)
        self.kw = {k: dev(v) for k, v in scene.per_image.items()}
        self.mask = None if scene.mask is None else dev(scene.mask)
        self.attrs = {k: dev(v) for k, v in scene.attrs.items()} if with_attrs else {}

    def batch(self, images=None):
        sel = slice(None) if images is None else list(images)
        return self.model.batch(self.xyz, self.pos[sel], img_mask=self.mask, **self.attrs,
                                **{k: v[sel] for k, v in self.kw.items()})

    def single(self, i):
        return self.model(self.xyz, self.pos[i], img_mask=self.mask, **self.attrs,
                          **{k: v[i] for k, v in self.kw.items()})


def check_layout(out, B):
    rp = out["row_ptr"].cpu().numpy()
    assert rp.shape == (B + 1,) and rp[0] == 0 and rp[-1] == out["idx"].shape[0] and (np.diff(rp) >= 0).all(), rp
    assert np.array_equal(out["image"].cpu().numpy(), np.repeat(np.arange(B), np.diff(rp)))
    for k in ("idx", "x", "y"):
        assert out[k].dtype == torch.int64
    return rp


def check_equals_single(out, a, b, one, what):
    """Rows [a, b) of a batch against the single-image build of that camera."""
    assert b - a == one["idx"].shape[0], (what, b - a, one["idx"].shape[0])
    if b == a:
        return
    for k in ROW_KEYS:
        assert torch.equal(out[k][a:b], one[k]), (what, k)


def check_equals_oracle(run, out, a, b, i, ref, what):
    """Rows [a, b) of a build against the oracle's rows ``ref`` of camera i."""
    assert b - a == len(ref["idx"]), (what, b - a, len(ref["idx"]))
    if b == a:
        return
    for k in ("idx", "x", "y", "depth"):
        assert np.array_equal(out[k][a:b].cpu().numpy(), ref[k]), (what, k)
    for k in ("x_proj", "y_proj"):
        np.testing.assert_allclose(out[k][a:b].cpu().numpy(), ref[k], rtol=0, atol=1e-9, err_msg=str((what, k)))
    feats = S.oracle_features(run.scene, i, ref, run.with_attrs)
    assert tuple(out["features"][a:b].shape) == feats.shape
    np.testing.assert_allclose(out["features"][a:b].cpu().numpy(), feats, rtol=0, atol=2.5e-7, err_msg=str(what))


def check_batch(run, oracle_images=None, rows_of=None):
    """The batch of all cameras of the scene: layout, every image against its single build, the images
    ``oracle_images`` (default: all) against the oracle.  Returns (out, row_ptr)."""
    sc = run.scene
    out = run.batch()
    rp = check_layout(out, sc.B)
    for i in range(sc.B):
        check_equals_single(out, rp[i], rp[i + 1], run.single(i), (sc.name, "single", i))
    for i in (range(sc.B) if oracle_images is None else oracle_images):
        ref = rows_of(i) if rows_of else S.oracle_rows(sc, i, run.exact)
        check_equals_oracle(run, out, rp[i], rp[i + 1], i, ref, (sc.name, "oracle", i))
    return out, rp


# ---------------------------------------------------------------------------------------------------------------
# 1. camera models at scale
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("camera", list(S.CAMERA_MODELS))
def test_camera_models_at_scale(camera, exact, single_image_kernels):
    """scannet 320 x 240, kitti360_perspective 1408 x 376 (cropped to 325 rows, masked) and kitti360_fisheye 1400 x 1400,
    four poses, 56 k points: image 0 has more large boxes than its large-box list holds, so the fallback plane is filled
    and merged; every image equals its single build and the oracle, with all four point attributes."""
    sc = S.check_camera_model_scene(camera)
    out, rp = check_batch(Run(sc, exact, with_attrs=True), rows_of=lambda i: S.cached_oracle_rows(camera, i, exact))
    assert (np.diff(rp) >= S.MIN_ROWS).all()


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("camera", list(S.CAMERA_MODELS))
def test_camera_models_batch_of_one(camera, exact, single_image_kernels):
    """Image 0 of the same scenes as a batch of one: its tile lists (4 entries per candidate) overflow as well."""
    sc = S.check_camera_model_scene(camera)
    run = Run(sc, exact, with_attrs=True)
    solo = run.batch([0])
    rp = check_layout(solo, 1)
    check_equals_single(solo, 0, rp[1], run.single(0), (camera, "solo single"))
    check_equals_oracle(run, solo, 0, rp[1], 0, S.cached_oracle_rows(camera, 0, exact), (camera, "solo oracle"))


@pytest.mark.parametrize("camera", list(S.CAMERA_MODELS))
def test_camera_models_single_image_dense(camera, single_image_kernels):
    """The single-image kernels in non-exact mode on the pinhole and fisheye cameras, against the oracle."""
    sc = S.check_camera_model_scene(camera)
    run = Run(sc, False, with_attrs=True)
    for i in range(sc.B):
        one = run.single(i)
        ref = S.cached_oracle_rows(camera, i, False)
        assert len(ref["idx"]) > len(S.cached_oracle_rows(camera, i, True)["idx"])       # dense: more rows than exact
        check_equals_oracle(run, one, 0, one["idx"].shape[0], i, ref, (camera, "single dense", i))


# ---------------------------------------------------------------------------------------------------------------
# 2. tile-counter placement
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("img_size", list(S.COUNTER_SIZES), ids=S.size_id)
def test_tile_counter_placement(img_size, exact, single_image_kernels):
    """T = 4096 (two images of counters in LDS, the 64 KiB request), 4224 (one), 8192 (one, 64 KiB), 8320 (none)."""
    sc = S.check_tile_counter_scene(img_size, 30_000, 3)
    check_batch(Run(sc, exact))


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("img_size", [(4096, 1056), (4096, 2080)], ids=S.size_id)
def test_tile_counter_placement_short_images(img_size, exact, single_image_kernels):
    """1500 survivors per image, five images: every chunk of 2048 survivors crosses an image boundary, so with one image
    of counters in LDS about half of the entries, and with none all of them, go through the global counters."""
    sc = S.check_tile_counter_scene(img_size, 1500, 5)
    check_batch(Run(sc, exact))


# ---------------------------------------------------------------------------------------------------------------
# 3. second sweep of the bin kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
def test_bin_kernels_second_sweep(exact, single_image_kernels):
    """32 images x 270 k survivors: more than 4096 blocks x 2048 survivors, so the blocks of the bin kernels go round
    their chunk loop a second time."""
    sc = S.check_second_sweep_scene()
    check_batch(Run(sc, exact), oracle_images=(0, 15, 31))


# ---------------------------------------------------------------------------------------------------------------
# 4. atomic-plane batch path, and the 16-bit box packing at its limit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("width", [65536, 65535])
def test_wide_images(width, exact, single_image_kernels):
    """65536 x 32: too wide for 16-bit box corners, the batch takes the atomic plane (quarter-wavefront and whole-wavefront
    sweeps, seen / winners kernels over B planes).  65535 x 32: the widest tiled image, boxes reach x1 = 65535."""
    sc = S.check_wide_scene(width)
    check_batch(Run(sc, exact))


# ---------------------------------------------------------------------------------------------------------------
# 5. empty images inside a batch
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("seeing", [(1, 3), (2,)], ids=["seen_by_1_3", "seen_by_2"])
@pytest.mark.parametrize("camera", ["s3dis_equirectangular", "scannet"])
def test_empty_images_inside_a_batch(camera, seeing, exact, single_image_kernels):
    sc = S.check_empty_images_scene(camera, seeing)
    out, rp = check_batch(Run(sc, exact, with_attrs=True))
    counts = np.diff(rp)
    for i in range(sc.B):
        assert (counts[i] > 0) == (i in seeing), (i, counts)       # row_ptr is flat across the empty images
    assert sorted(set(out["image"].cpu().numpy().tolist())) == list(seeing)
    assert counts.sum() >= S.MIN_ROWS


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("n", [1, 0])
def test_batch_of_one_point_and_of_none(n, exact, single_image_kernels):
    base = S.empty_images_scene("s3dis_equirectangular", (1, 3))
    sc = S.Scene(f"n{n}", base.camera, base.kw, base.xyz[:n], base.img_xyz, base.per_image,
                 attrs={k: v[:n] for k, v in base.attrs.items()})
    run = Run(sc, exact, with_attrs=True)
    out = run.batch()
    rp = check_layout(out, sc.B)
    refs = [S.oracle_rows(sc, i, exact) for i in range(sc.B)]
    # the point lies within r_max of cameras 1 and 3 only (its box covers a few pixels: one row each in exact mode)
    counts = [len(r["idx"]) for r in refs]
    assert [c > 0 for c in counts] == [False, n > 0, False, n > 0, False] and (not exact or sum(counts) == 2 * n)
    assert np.array_equal(np.diff(rp), counts) and tuple(out["features"].shape) == (sum(counts), 6)
    for i, ref in enumerate(refs):
        check_equals_oracle(run, out, rp[i], rp[i + 1], i, ref, (sc.name, i))
        if n:
            check_equals_single(out, rp[i], rp[i + 1], run.single(i), (sc.name, i))
