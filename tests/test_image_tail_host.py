"""No GPU: the host side of the image tail (ColorJitter / Normalize / ToImageData / FusedImageTail, csrc/image_tail.hip).

The two restatements of the contract in tests/image_tail_ref.py agree byte for byte where they must (H W <= 65793);
ColorJitter.draw() makes torchvision 0.8.2's draws; fuse_image_tail rewrites the chains of the shipped configs; the
C ABI rejects bad arguments before any HIP call; the drop-in names resolve."""
import ctypes

import numpy as np
import pytest
import torch

import image_tail_ref as R
from deepviewagg_amd import _lib
from deepviewagg_amd.core.data_transform.multimodal import image as T

SHAPES = [(3, 5, 23), (2, 16, 64), (1, 1, 1), (2, 256, 256)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatements_agree(shape):
    """numpy contract (integer-sum mean) == torch composition of the torchvision formulas (torch.mean), byte for byte,
    for the 15 op lists on random, all-0 and all-255 images with factors 0.0, 1.0, 1.7 and random ones."""
    assert shape[1] * shape[2] <= 65793
    sets = R.factor_sets(seed=shape[2])
    for kind in ("random", "zeros", "full"):
        x = R.images(shape, kind, seed=shape[1])
        xt = torch.from_numpy(x)
        for names in R.OP_LISTS:
            for tag, factors in sets.items():
                jitter = R.with_factors(names, factors)
                want = R.jitter_torch(xt, jitter).numpy()
                got = R.jitter_np(x, jitter)
                assert np.array_equal(got, want), (shape, kind, jitter)


def test_restatements_agree_on_the_float_tail():
    x = R.images((2, 7, 130), "random", seed=3)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    jitter = [("contrast", 1.25), ("brightness", 0.75)]
    for kw in (dict(to_float=True), dict(to_float=True, mean=mean, std=std),
               dict(flip=True, to_float=True, mean=mean, std=std), dict(jitter=jitter, flip=True)):
        want = R.torch_tail(torch.from_numpy(x), **kw).numpy()
        assert np.array_equal(R.numpy_tail(x, **kw), want), kw
    xf = torch.from_numpy(x).float() / 255
    assert np.array_equal(R.numpy_tail(x, to_float=True, mean=mean, std=std),
                          ((xf - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)).numpy())


# ---- draws --------------------------------------------------------------------------------------------------------

def by_hand(seed, ranges):
    """The draws of torchvision 0.8.2's ColorJitter.forward: ranges = {op id: (lo, hi)} of the present ops."""
    torch.manual_seed(seed)
    out = []
    for i in torch.randperm(4).tolist():
        if i in ranges:
            out.append((R.NAMES[i], torch.tensor(1.0).uniform_(*ranges[i]).item()))
    return out, torch.rand(1)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 11])
def test_color_jitter_draws(seed):
    want, after = by_hand(seed, {0: (1 - 0.6, 1 + 0.6), 1: (1 - 0.6, 1 + 0.6), 2: (max(0.0, 1 - 0.7), 1 + 0.7)})
    torch.manual_seed(seed)
    got = T.ColorJitter(0.6, 0.6, 0.7).draw()
    assert got == want and len(got) == 3
    assert torch.equal(torch.rand(1), after)             # nothing else was drawn


def test_color_jitter_absent_op_draws_nothing_and_pairs_are_used_as_given():
    want, after = by_hand(5, {0: (0.5, 0.75), 2: (0.0, 3.0)})
    torch.manual_seed(5)
    cj = T.ColorJitter(brightness=(0.5, 0.75), contrast=0, saturation=2)     # 1 - 2 clips to 0
    got = cj.draw()
    assert got == want and [n for n, _ in got].count("contrast") == 0
    assert torch.equal(torch.rand(1), after)
    assert all(0.5 <= f <= 0.75 for n, f in got if n == "brightness")
    # a [1, 1] pair is an absent op too
    torch.manual_seed(5)
    assert T.ColorJitter(contrast=(1, 1)).draw() == []
    assert (cj.brightness, cj.contrast, cj.saturation) == ((0.5, 0.75), 0, 2)
    assert repr(cj) == "ColorJitter(brightness=(0.5, 0.75), contrast=0, saturation=2)"


@pytest.mark.parametrize("kw", [dict(brightness=-0.1), dict(contrast=-1), dict(saturation=(-0.5, 1.0)),
                                dict(brightness=(1.2, 0.8))])
def test_color_jitter_rejects_bad_ranges(kw):
    with pytest.raises(ValueError):
        T.ColorJitter(**kw)


def test_normalize_defaults_and_repr():
    n = T.Normalize()
    assert n.mean == [0.485, 0.456, 0.406] and n.std == [0.229, 0.224, 0.225]
    assert repr(n) == "Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])"


# ---- fuse_image_tail ----------------------------------------------------------------------------------------------

def s3dis_head():
    return [T.SelectMappingFromPointId(), T.CenterRoll(), T.PickImagesFromMappingArea(use_bbox=False),
            T.CropImageGroups(padding=8, min_size=64), T.PickImagesFromMemoryCredit(img_size=[1024, 512], n_img=4,
                                                                                   k_coverage=2)]


def test_fuse_s3dis_train_and_eval_lists():
    cj, fl, tf, nm = T.ColorJitter(0.6, 0.6, 0.7), T.RandomHorizontalFlip(), T.ToFloatImage(), T.Normalize()
    head = s3dis_head() + [T.JitterMappingFeatures(sigma=0.02, clip=0.03)]
    fused = T.fuse_image_tail(head + [cj, fl, tf, nm])
    assert fused[:-1] == head and len(fused) == len(head) + 1
    tail = fused[-1]
    assert type(tail) is T.FusedImageTail
    assert (tail.color_jitter, tail.flip, tail.to_float, tail.normalize) == (cj, fl, tf, nm)
    assert tail._PROCESS_IMAGE_DATA
    head = s3dis_head()
    fused = T.fuse_image_tail(head + [tf, nm])
    assert fused[:-1] == head and type(fused[-1]) is T.FusedImageTail
    assert (fused[-1].color_jitter, fused[-1].flip, fused[-1].to_float, fused[-1].normalize) == (None, None, tf, nm)


def test_fuse_leaves_everything_else_alone():
    cj, fl, tf, nm = T.ColorJitter(0.2, 0.2, 0.2), T.RandomHorizontalFlip(), T.ToFloatImage(), T.Normalize()
    src = [cj, fl]
    assert T.fuse_image_tail(src) == [cj, fl] and T.fuse_image_tail(src) is not src
    out = T.fuse_image_tail([tf, cj])
    assert type(out[0]) is T.FusedImageTail and out[1] is cj and len(out) == 2
    assert (out[0].color_jitter, out[0].flip, out[0].to_float, out[0].normalize) == (None, None, tf, None)
    # a transform between two members splits the run: the jitter stays eager, the rest fuses
    mid = T.AddPixelHeightFeature()
    out = T.fuse_image_tail([cj, mid, fl, tf, mid, nm])
    assert out[0] is cj and out[1] is mid and out[3] is mid and out[4] is nm and len(out) == 5
    assert (out[2].color_jitter, out[2].flip, out[2].to_float, out[2].normalize) == (None, fl, tf, None)
    # the order is part of the pattern: a flip before the jitter is no member of the jitter's run
    out = T.fuse_image_tail([fl, cj, tf])
    assert out[0] is fl and (out[1].color_jitter, out[1].flip, out[1].to_float) == (cj, None, tf) and len(out) == 2
    # two runs in one list
    tf2 = T.ToFloatImage()
    out = T.fuse_image_tail([tf, nm, tf2])
    assert [type(o) for o in out] == [T.FusedImageTail] * 2 and out[1].to_float is tf2 and out[0].normalize is nm
    assert T.fuse_image_tail([]) == []


# ---- C ABI ----------------------------------------------------------------------------------------------------------

def call_u8(lib, x=1, B=2, H=4, W=4, codes=(0,), factors=(1.0,), n_ops=None, flip=0, to_float=0, mean=None, std=None,
            out=1, ws=1, ws_bytes=256):
    """dva_image_tail_u8 with fake non-null device pointers (never dereferenced: the call must fail before any launch)."""
    n = len(codes) if n_ops is None else n_ops
    c = (ctypes.c_int32 * len(codes))(*codes) if codes is not None else None
    f = (ctypes.c_double * len(factors))(*factors) if factors is not None else None
    fl = lambda v: None if v is None else (ctypes.c_float * len(v))(*v)
    p = lambda v: ctypes.c_void_p(0x1000 if v else 0)
    return lib.dva_image_tail_u8(p(x), B, H, W, c, f, n, flip, to_float, fl(mean), fl(std), p(out), p(ws), ws_bytes, None)


def test_abi_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    assert lib.dva_version() >= 317
    assert call_u8(lib, x=0) == -1 and call_u8(lib, out=0) == -1                  # null pointers
    assert call_u8(lib, codes=None, n_ops=1) == -1 and call_u8(lib, factors=None) == -1
    assert call_u8(lib, codes=(1,), ws=0) == -1                                   # contrast needs its accumulators
    assert call_u8(lib, codes=(1,), ws_bytes=8) == -1
    assert call_u8(lib, B=-1) == -1 and call_u8(lib, H=-1) == -1 and call_u8(lib, W=-1) == -1
    assert call_u8(lib, n_ops=-1) == -1
    assert call_u8(lib, codes=(0, 1, 2, 0), factors=(1.0,) * 4) == -1             # four ops
    assert call_u8(lib, codes=(0, 2, 0), factors=(1.0,) * 3) == -1                # a repeated op
    assert call_u8(lib, codes=(3,)) == -1 and call_u8(lib, codes=(-1,)) == -1     # unknown op codes (3 would be hue)
    assert call_u8(lib, factors=(-0.5,)) == -1 and call_u8(lib, factors=(float("nan"),)) == -1
    assert call_u8(lib, to_float=1, mean=[0.5] * 3) == -1                         # mean without std
    assert call_u8(lib, to_float=1, mean=[0.5] * 3, std=[0.5, 0.0, 0.5]) == -1    # a zero in std
    assert call_u8(lib, to_float=0, mean=[0.5] * 3, std=[0.5] * 3) == -1          # Normalize without ToFloatImage
    assert lib.dva_image_tail_workspace_bytes(-1) == -1
    assert lib.dva_image_tail_workspace_bytes(3) >= 24
    m = (ctypes.c_float * 2)(0.5, 0.5)
    z = (ctypes.c_float * 2)(0.5, 0.0)
    p = ctypes.c_void_p(0x1000)
    assert lib.dva_image_normalize_f32(None, 1, 2, 16, m, m, p, None) == -1
    assert lib.dva_image_normalize_f32(p, 1, 2, 16, m, m, None, None) == -1
    assert lib.dva_image_normalize_f32(p, 1, 2, 16, None, m, p, None) == -1
    assert lib.dva_image_normalize_f32(p, -1, 2, 16, m, m, p, None) == -1
    assert lib.dva_image_normalize_f32(p, 1, 0, 16, m, m, p, None) == -1
    assert lib.dva_image_normalize_f32(p, 1, 2, -16, m, m, p, None) == -1
    assert lib.dva_image_normalize_f32(p, 1, 2, 16, m, z, p, None) == -1
    big = (ctypes.c_float * 65)(*([1.0] * 65))
    assert lib.dva_image_normalize_f32(p, 1, 65, 16, big, big, p, None) == -2     # more than DVA_IMAGE_MAX_CHANNELS
    # an empty batch or image is a no-op that needs no buffer
    assert call_u8(lib, x=0, out=0, B=0) == 0 and call_u8(lib, x=0, out=0, W=0) == 0
    assert lib.dva_image_normalize_f32(None, 0, 2, 16, m, m, None, None) == 0


def test_ops_image_tail_refuses_host_tensors():
    from deepviewagg_amd import ops
    with pytest.raises(_lib.DvaError):
        ops.image_tail(torch.zeros(1, 3, 2, 2, dtype=torch.uint8), to_float=True)


# ---- drop-in and ToImageData --------------------------------------------------------------------------------------------

def test_dropin_resolves_the_new_names():
    import importlib
    from deepviewagg_amd import dropin
    dropin.install()
    mod = importlib.import_module("torch_points3d.core.data_transform.multimodal.image")
    for name in ("ColorJitter", "Normalize", "ToImageData", "FusedImageTail", "fuse_image_tail"):
        assert getattr(mod, name) is getattr(T, name)


def test_to_image_data_wraps_one_setting():
    from deepviewagg_amd.core.multimodal.image import ImageData, SameSettingImageData
    im = SameSettingImageData(path=np.array(["a", "b"]), pos=torch.zeros(2, 3), opk=torch.zeros(2, 3),
                              ref_size=(8, 4), proj_upscale=1)
    data = object()
    d, out = T.ToImageData()(data, im)
    assert d is data and isinstance(out, ImageData) and len(out) == 1 and out[0] is im
