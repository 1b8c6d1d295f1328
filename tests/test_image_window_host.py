"""No GPU: the host side of the deferred image windows (WindowedSameSettingImageData, DeferImages, the C ABI of
csrc/image_tail.hip's dva_image_window_u8).

The oracle of the windowed tail, tests/image_window_ref.py::window_np, is held to the eager classes on host tensors;
a deferred setting is driven through the image side of the S3DIS train chain next to the eager one; the deferral begins
and ends where it says.  Every comparison is byte for byte.

The online chains sort, de-duplicate and average mappings with HIP kernels (no CPU fallback in the product), so the
chain test replaces those three primitives by torch / numpy stand-ins (image_window_ref.host_kernels) for BOTH chains:
the mapping side is the base class's code either way, and the test is about the pixels and the roll / crop state.  The
same chains run on the device, kernels and all, in tests/test_gpu_image_window.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import image_window_ref as WR
from deepviewagg_amd import _lib
from deepviewagg_amd.core.data_transform.multimodal import image as T
from deepviewagg_amd.core.multimodal.image import ImageData, SameSettingImageData, WindowedSameSettingImageData


def plain_setting(x, ref_size=None):
    """A host SameSettingImageData around x [B, C, H, W], without mappings; ref_size (W, H) defaults to x's."""
    B, _, H, W = x.shape
    return SameSettingImageData(path=np.array([f"img_{i}" for i in range(B)]), pos=torch.zeros(B, 3),
                                opk=torch.zeros(B, 3), ref_size=ref_size or (W, H), proj_upscale=1, x=x)


# ---- the oracle against the eager classes ---------------------------------------------------------------------------

def window_case(seed):
    """Seeded (src, index, rolls, offsets, size).  The first seeds pin the named cases: 0 no roll, 1 rolls >= W, 2 the
    whole width with a roll, 3 a window on the right and bottom borders; the rest is random (index without repeats,
    as SameSettingImageData.__getitem__ demands)."""
    rng = np.random.default_rng(seed)
    N, H, W = int(rng.integers(1, 6)), int(rng.integers(1, 14)), int(rng.integers(1, 41))
    src = rng.integers(0, 256, size=(N, 3, H, W), dtype=np.uint8)
    B = int(rng.integers(1, N + 1))
    index = rng.permutation(N)[:B]
    Wc, Hc = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
    rolls = rng.integers(-2 * W, 3 * W + 1, size=B)
    offsets = np.stack([rng.integers(0, W - Wc + 1, size=B), rng.integers(0, H - Hc + 1, size=B)], 1)
    if seed == 0:
        rolls[:] = 0
    elif seed == 1:
        rolls = W + rng.integers(0, 2 * W + 1, size=B)
    elif seed == 2:
        Wc, offsets[:, 0], rolls = W, 0, 1 + rng.integers(0, max(W - 1, 1), size=B)
    elif seed == 3:
        offsets[:, 0], offsets[:, 1] = W - Wc, H - Hc
    return src, index, rolls, offsets, (Wc, Hc)


@pytest.mark.parametrize("seed", range(60))
def test_window_np_equals_the_eager_classes(seed):
    src, index, rolls, offsets, size = window_case(seed)
    images = plain_setting(torch.from_numpy(src))[torch.from_numpy(index)]
    images.update_rollings(torch.from_numpy(rolls))
    images.update_cropping(size, torch.from_numpy(offsets))
    want = WR.window_np(src, index, rolls, offsets, size)
    assert np.array_equal(images.x.numpy(), want)
    # the deferred view of the same setting, materialised on the host, holds the same bytes
    lazy = plain_setting(torch.from_numpy(src)).windowed()[torch.from_numpy(index)]
    lazy.update_rollings(torch.from_numpy(rolls))
    lazy.update_cropping(size, torch.from_numpy(offsets))
    assert lazy.is_deferred
    assert np.array_equal(lazy.x.numpy(), want) and not lazy.is_deferred
    assert torch.equal(lazy.crop_offsets, images.crop_offsets) and lazy.crop_size == images.crop_size


def test_the_named_window_cases_are_what_they_say():
    _, _, rolls, _, _ = window_case(0)
    assert not rolls.any()
    src, _, rolls, _, _ = window_case(1)
    assert (rolls >= src.shape[-1]).all()
    src, _, rolls, offsets, size = window_case(2)
    assert size[0] == src.shape[-1] and (rolls % src.shape[-1] != 0).any()
    src, _, _, offsets, size = window_case(3)
    assert (offsets[:, 0] + size[0] == src.shape[-1]).all() and (offsets[:, 1] + size[1] == src.shape[-2]).all()


def test_a_second_roll_adds_to_the_first():
    """update_rollings replaces ``rollings`` but rolls the pixels again: the deferred class accumulates mod W."""
    src = np.random.default_rng(5).integers(0, 256, size=(3, 3, 4, 10), dtype=np.uint8)
    eager, lazy = plain_setting(torch.from_numpy(src)), plain_setting(torch.from_numpy(src)).windowed()
    for rolls in ([3, 0, 9], [8, 5, 4]):
        eager.update_rollings(torch.tensor(rolls))
        lazy.update_rollings(torch.tensor(rolls))
    assert torch.equal(lazy.rollings, eager.rollings) and torch.equal(lazy.rollings, torch.tensor([8, 5, 4]))
    assert torch.equal(lazy.source_roll, torch.tensor([1, 5, 3]))
    assert torch.equal(lazy.x, eager.x)


# ---- the chain ------------------------------------------------------------------------------------------------------

def test_deferred_s3dis_chain_equals_the_eager_chain_on_the_host():
    """SelectMappingFromPointId -> CenterRoll -> PickImagesFromMappingArea -> CropImageGroups ->
    PickImagesFromMemoryCredit on the golden mappings with random uint8 images of 64 x 128."""
    with WR.host_kernels():
        sizes, rolled = set(), False
        for seed in range(4):
            data, images = WR.golden_setting("cpu", seed=seed)
            head = WR.s3dis_head(T)
            _, eager, next_e = WR.run_chain(head, copy.deepcopy(data), copy.deepcopy(images), seed)
            _, lazy, next_l = WR.run_chain([T.DeferImages()] + head, copy.deepcopy(data), copy.deepcopy(images), seed)
            assert isinstance(lazy, ImageData) and len(lazy) >= 1
            assert all(isinstance(im, WindowedSameSettingImageData) and im.is_deferred for im in lazy)
            # nothing but indices moved: every setting still reads the one tensor the chain began with
            assert len({im.source.data_ptr() for im in lazy}) == 1 and lazy[0].source.shape == images.x.shape
            WR.assert_same_settings(eager, lazy)
            assert not any(im.is_deferred for im in lazy)            # the comparison read x
            assert next_e == next_l
            sizes |= {tuple(im.crop_size) for im in eager}
            rolled |= any(bool(im.source_roll.any()) for im in WR.run_chain(
                [T.DeferImages()] + head[:2], copy.deepcopy(data), copy.deepcopy(images), seed)[1:2])
        assert len(sizes) >= 2, sizes                                 # the chain really crops, to several sizes
        assert any(s != (128, 64) for s in sizes)
        assert rolled                                                 # and really rolls


# ---- where the deferral begins and ends -------------------------------------------------------------------------------

def source_of(B=4, H=6, W=16, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(B, 3, H, W), dtype=np.uint8))


def test_reading_x_returns_the_window_and_ends_the_deferral():
    x = source_of()
    lazy = plain_setting(x).windowed()
    assert type(lazy) is WindowedSameSettingImageData and lazy.is_deferred and lazy.source.data_ptr() == x.data_ptr()
    lazy = lazy[[2, 0]]
    lazy.update_cropping((8, 3), torch.tensor([[4, 1], [8, 3]]))
    assert lazy.is_deferred and lazy.img_size == (8, 3)
    got = lazy.x
    assert not lazy.is_deferred and lazy.source is None
    assert torch.equal(got, torch.stack([x[2, :, 1:4, 4:12], x[0, :, 3:6, 8:16]]))
    assert lazy.x is got                                              # an ordinary setting from here on
    sub = lazy[[1]]
    assert torch.equal(sub.x, got[1:]) and not sub.is_deferred


def test_setting_x_ends_the_deferral_and_drops_the_source():
    x = source_of()
    lazy = plain_setting(x).windowed()
    new = torch.rand(4, 5, 3, 8)
    lazy.x = new
    assert not lazy.is_deferred and lazy.source is None and lazy.source_index is None
    assert lazy.x is new and lazy.downscale == 2                      # the base setter's rescale still applies
    lazy = plain_setting(x).windowed()
    lazy.x = None
    assert not lazy.is_deferred and lazy.x is None


def test_getitem_clone_and_to_share_the_source():
    x = source_of()
    lazy = plain_setting(x).windowed()
    ptr = lazy.source.data_ptr()
    assert ptr == x.data_ptr()
    for other in (lazy[[3, 1]], lazy[torch.tensor([True, False, True, False])], lazy.clone(), lazy.to("cpu"),
                  lazy[[0, 1, 2]][[2, 0]]):
        assert other.is_deferred and other.source.data_ptr() == ptr and type(other) is WindowedSameSettingImageData
    assert lazy.is_deferred                                           # and none of them made `lazy` read its pixels
    assert torch.equal(lazy[[3, 1]].source_index, torch.tensor([3, 1]))
    assert torch.equal(lazy[[0, 1, 2]][[2, 0]].source_index, torch.tensor([2, 0]))
    assert torch.equal(lazy[[0, 1, 2]][[2, 0]].x, x[[2, 0]])


def test_settings_that_do_not_qualify_come_back_as_they_are():
    x = source_of()
    half = plain_setting(x[:, :, ::2, ::2].contiguous(), ref_size=(16, 6))
    assert half.downscale == 2
    empty = plain_setting(x)
    empty.x = None
    for images in (plain_setting(x.float()), plain_setting(x[:, :1]), half, empty):
        assert images.windowed() is images and type(images) is SameSettingImageData
    cropped = plain_setting(x).update_cropping((8, 3), torch.zeros(4, 2, dtype=torch.long))
    assert cropped.windowed() is cropped
    rolled = plain_setting(x).update_rollings(torch.tensor([1, 0, 0, 0]))
    assert rolled.windowed() is rolled
    lazy = plain_setting(x).windowed()
    assert lazy.windowed() is lazy
    data = object()
    d, out = T.DeferImages()(data, plain_setting(x.float()))
    assert d is data and type(out) is SameSettingImageData
    d, out = T.DeferImages()(data, ImageData([plain_setting(x), plain_setting(x.float())]))
    assert [type(im) for im in out] == [WindowedSameSettingImageData, SameSettingImageData]


def test_defer_image_windows_rewrites_a_chain():
    cj, fl, tf, nm = T.ColorJitter(0.6, 0.6, 0.7), T.RandomHorizontalFlip(), T.ToFloatImage(), T.Normalize()
    head = WR.s3dis_head(T)
    out = T.defer_image_windows(head + [cj, fl, tf, nm])
    assert type(out[0]) is T.DeferImages and out[1:-1] == head and type(out[-1]) is T.FusedImageTail
    assert (out[-1].color_jitter, out[-1].flip, out[-1].to_float, out[-1].normalize) == (cj, fl, tf, nm)


def test_dropin_resolves_the_new_names():
    import importlib
    from deepviewagg_amd import dropin
    dropin.install()
    mod = importlib.import_module("torch_points3d.core.data_transform.multimodal.image")
    for name in ("DeferImages", "defer_image_windows", "FusedImageTail"):
        assert getattr(mod, name) is getattr(T, name)
    mod = importlib.import_module("torch_points3d.core.multimodal.image")
    assert mod.WindowedSameSettingImageData is WindowedSameSettingImageData


# ---- C ABI ------------------------------------------------------------------------------------------------------------

def call_window(lib, src=1, N=3, H=8, W=16, index=1, rolls=1, offsets=1, B=2, Wc=8, Hc=4, codes=(0,), factors=(1.0,),
                n_ops=None, flip=0, to_float=0, mean=None, std=None, out=1, ws=1, ws_bytes=256):
    """dva_image_window_u8 with fake non-null device pointers (never dereferenced: the call must fail before any launch)."""
    n = len(codes) if n_ops is None else n_ops
    c = (ctypes.c_int32 * len(codes))(*codes) if codes is not None else None
    f = (ctypes.c_double * len(factors))(*factors) if factors is not None else None
    fl = lambda v: None if v is None else (ctypes.c_float * len(v))(*v)
    p = lambda v: ctypes.c_void_p(0x1000 if v else 0)
    return lib.dva_image_window_u8(p(src), N, H, W, p(index), p(rolls), p(offsets), B, Wc, Hc, c, f, n, flip, to_float,
                                   fl(mean), fl(std), p(out), p(ws), ws_bytes, None)


def test_abi_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    assert lib.dva_version() >= 318
    for name in ("src", "index", "rolls", "offsets", "out"):                        # null pointers
        assert call_window(lib, **{name: 0}) == -1, name
    assert call_window(lib, codes=None, n_ops=1) == -1 and call_window(lib, factors=None) == -1
    assert call_window(lib, codes=(1,), ws=0) == -1 and call_window(lib, codes=(1,), ws_bytes=8) == -1
    for name in ("N", "H", "W", "B", "Wc", "Hc"):                                   # negative sizes
        assert call_window(lib, **{name: -1}) == -1, name
    assert call_window(lib, n_ops=-1) == -1
    assert call_window(lib, Wc=17) == -1 and call_window(lib, Hc=9) == -1           # a window larger than the image
    assert call_window(lib, Wc=0) == -1 and call_window(lib, Hc=0) == -1 and call_window(lib, N=0) == -1
    assert call_window(lib, codes=(0, 1, 2, 0), factors=(1.0,) * 4) == -1           # four ops
    assert call_window(lib, codes=(0, 2, 0), factors=(1.0,) * 3) == -1              # a repeated op
    assert call_window(lib, codes=(3,)) == -1 and call_window(lib, codes=(-1,)) == -1
    assert call_window(lib, factors=(-0.5,)) == -1 and call_window(lib, factors=(float("nan"),)) == -1
    assert call_window(lib, to_float=1, mean=[0.5] * 3) == -1
    assert call_window(lib, to_float=1, mean=[0.5] * 3, std=[0.5, 0.0, 0.5]) == -1
    assert call_window(lib, to_float=0, mean=[0.5] * 3, std=[0.5] * 3) == -1
    assert call_window(lib, B=70000) == -2                                          # beyond the grid's second dimension
    assert lib.dva_image_window_workspace_bytes(-1) == -1
    assert lib.dva_image_window_workspace_bytes(3) >= 24
    # an empty batch is a no-op that needs no buffer -- but a window that does not fit is refused all the same
    assert call_window(lib, src=0, index=0, rolls=0, offsets=0, out=0, B=0) == 0
    assert call_window(lib, B=0, Wc=17) == -1


def test_ops_image_window_refuses_host_tensors_and_bad_arguments():
    from deepviewagg_amd import ops
    x = source_of()
    with pytest.raises(_lib.DvaError):
        ops.image_window(x, torch.arange(2))
