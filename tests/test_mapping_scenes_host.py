"""Preconditions of the scenes of tests/mapping_scenes.py, from the C oracle alone (no GPU): each scene really meets the
condition that sends dva_visibility_batch down the branch its GPU test (tests/test_gpu_mapping_dispatch.py) is about."""
import pytest

import mapping_scenes as S


@pytest.mark.parametrize("camera", list(S.CAMERA_MODELS))
def test_camera_model_scene(camera):
    S.check_camera_model_scene(camera)


@pytest.mark.parametrize("img_size", list(S.COUNTER_SIZES), ids=S.size_id)
def test_tile_counter_scene(img_size):
    S.check_tile_counter_scene(img_size, 30_000, 3)


@pytest.mark.parametrize("img_size", [(4096, 1056), (4096, 2080)], ids=S.size_id)
def test_tile_counter_scene_short_images(img_size):
    S.check_tile_counter_scene(img_size, 1500, 5)


def test_second_sweep_scene():
    S.check_second_sweep_scene()


@pytest.mark.parametrize("width", [65536, 65535])
def test_wide_scene(width):
    S.check_wide_scene(width)


@pytest.mark.parametrize("camera", ["s3dis_equirectangular", "scannet"])
@pytest.mark.parametrize("seeing", [(1, 3), (2,)], ids=["seen_by_1_3", "seen_by_2"])
def test_empty_images_scene(camera, seeing):
    S.check_empty_images_scene(camera, seeing)
