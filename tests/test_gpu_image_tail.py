"""-m gpu: ops.image_tail and the ColorJitter / Normalize / FusedImageTail transforms (csrc/image_tail.hip) against the
numpy restatement of the contract in tests/image_tail_ref.py.  Every comparison is torch.equal: the contract is bit for
bit.  The float tail is also held to the torch CPU expression ((x.float() / 255) - mean) / std."""
import copy

import numpy as np
import pytest
import torch

import image_tail_ref as R
from conftest import t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# (3, 5, 23): odd width = row tails and unaligned row starts; (2, 7, 130): a tail after full chunks of 4, none of 16
SHAPES = [(3, 5, 23), (2, 16, 64), (1, 1, 1), (2, 7, 130)]


def ops():
    from deepviewagg_amd import ops as o
    return o


def same(got, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("kind", ["random", "zeros", "full"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ops_match_the_contract(shape, kind):
    """The 15 op lists, with factors 0.0 / 1.0 / 1.7 (the clamp on both sides) and random ones; the output is uint8."""
    x = R.images(shape, kind, seed=shape[2])
    xd = t(x, DEV)
    for names in R.OP_LISTS:
        for factors in R.factor_sets(seed=shape[1]).values():
            jitter = R.with_factors(names, factors)
            got = ops().image_tail(xd, jitter=jitter)
            assert got.dtype == torch.uint8
            same(got, R.jitter_np(x, jitter))
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                 # the input is not modified


def test_contrast_mean_is_per_image():
    x = R.images((3, 9, 37), "random", seed=1)
    x[0] //= 4                                                        # three images of different brightness
    x[2] = 255 - x[2] // 3
    jitter = [("brightness", 1.2), ("contrast", 0.5)]
    xd = t(x, DEV)
    batched = ops().image_tail(xd, jitter=jitter)
    same(batched, R.jitter_np(x, jitter))
    for i in range(3):
        assert torch.equal(batched[i:i + 1], ops().image_tail(xd[i:i + 1], jitter=jitter))
    assert len({int(v) for v in R.gray_np(x).reshape(3, -1).sum(1)}) == 3


def test_accumulators_are_cleared_by_every_call():
    x = R.images((2, 16, 64), "random", seed=2)
    xd = t(x, DEV)
    jitter = [("contrast", 1.4)]
    first = ops().image_tail(xd, jitter=jitter)
    second = ops().image_tail(xd, jitter=jitter)
    assert torch.equal(first, second)
    same(second, R.jitter_np(x, jitter))


def test_gray_sum_beyond_32_bits():
    """One all-255 image of 4200 x 4200: S = 255 n = 4.498e9 > 2^32.  Every output byte is the contract's value for one
    such pixel with m = f32(S) / f32(n) on numpy scalars."""
    n = 4200 * 4200
    gray = int(R.gray_np(np.full((1, 3, 1, 1), 255, dtype=np.uint8))[0, 0, 0])
    S = gray * n
    assert S > 2 ** 32
    m = R.contrast_mean_np(S, n)
    want = int(R.blend_np(np.float32(255), m, 0.5))
    xd = torch.full((1, 3, 4200, 4200), 255, dtype=torch.uint8, device=DEV)
    got = ops().image_tail(xd, jitter=[("contrast", 0.5)])
    assert got.dtype == torch.uint8 and got.shape == xd.shape
    lo, hi = int(got.min()), int(got.max())
    assert (lo, hi) == (want, want), (lo, hi, want, float(m))


def test_above_the_exact_float_sum_size():
    """300 x 260 = 78000 pixels > 65793: the integer-sum mean is the definition (no comparison with torch.mean)."""
    x = R.images((1, 300, 260), "random", seed=4)
    for names in (("saturation", "brightness", "contrast"), ("contrast", "saturation", "brightness")):
        jitter = R.with_factors(names, (1.3, 0.6, 1.45))
        same(ops().image_tail(t(x, DEV), jitter=jitter), R.jitter_np(x, jitter))


@pytest.mark.parametrize("shape", [(3, 5, 23), (2, 16, 64), (2, 7, 130)], ids=lambda s: "x".join(map(str, s)))
def test_float_tail(shape):
    x = R.images(shape, "random", seed=5)
    xd, xt = t(x, DEV), torch.from_numpy(x)
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    got = ops().image_tail(xd, to_float=True)
    assert got.dtype == torch.float32
    assert torch.equal(got.cpu(), xt.float() / 255)
    got = ops().image_tail(xd, to_float=True, mean=MEAN, std=STD)
    assert torch.equal(got.cpu(), ((xt.float() / 255) - mean) / std)
    got = ops().image_tail(xd, flip=True, to_float=True, mean=MEAN, std=STD)
    assert torch.equal(got.cpu(), ((torch.flip(xt, [3]).float() / 255) - mean) / std)
    same(got, R.numpy_tail(x, flip=True, to_float=True, mean=MEAN, std=STD))
    # the flip alone, and the whole train tail with a jitter in front
    same(ops().image_tail(xd, flip=True), x[..., ::-1])
    jitter = [("saturation", 1.3), ("contrast", 0.7), ("brightness", 1.1)]
    same(ops().image_tail(xd, jitter=jitter, flip=True, to_float=True, mean=MEAN, std=STD),
         R.numpy_tail(x, jitter=jitter, flip=True, to_float=True, mean=MEAN, std=STD))


def test_normalize_alone_on_five_float_channels():
    """AddPixelHeightFeature / AddPixelWidthFeature add channels before Normalize: any C, with C statistics."""
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 5, 6, 9, generator=g)
    mean, std = [0.485, 0.456, 0.406, 0.5, 0.25], [0.229, 0.224, 0.225, 0.5, 2.0]
    want = (x - torch.tensor(mean).view(1, 5, 1, 1)) / torch.tensor(std).view(1, 5, 1, 1)
    assert torch.equal(ops().image_tail(x.to(DEV), mean=mean, std=std).cpu(), want)
    x = torch.rand(3, 4, 8, 16, generator=g)                          # planes of a multiple of four elements
    want = (x - torch.tensor(mean[:4]).view(1, 4, 1, 1)) / torch.tensor(std[:4]).view(1, 4, 1, 1)
    assert torch.equal(ops().image_tail(x.to(DEV), mean=mean[:4], std=std[:4]).cpu(), want)


def test_non_contiguous_input():
    x = t(R.images((2, 12, 64), "random", seed=7), DEV)
    jitter = [("contrast", 0.8), ("saturation", 1.5)]
    kw = dict(jitter=jitter, flip=True, to_float=True, mean=MEAN, std=STD)
    strided = x[..., ::2]
    assert not strided.is_contiguous()
    assert torch.equal(ops().image_tail(strided, **kw), ops().image_tail(strided.contiguous(), **kw))
    cl = x.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    assert torch.equal(ops().image_tail(cl, **kw), ops().image_tail(x, **kw))
    assert torch.equal(ops().image_tail(cl, jitter=jitter), ops().image_tail(x, jitter=jitter))


def test_empty_batch_and_errors():
    o = ops()
    e = torch.empty(0, 3, 8, 16, dtype=torch.uint8, device=DEV)
    out = o.image_tail(e, jitter=[("contrast", 0.5)])
    assert out.dtype == torch.uint8 and out.shape == e.shape
    out = o.image_tail(e, to_float=True, mean=MEAN, std=STD)
    assert out.dtype == torch.float32 and out.shape == e.shape
    out = o.image_tail(torch.empty(2, 3, 0, 16, dtype=torch.uint8, device=DEV), flip=True, to_float=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 3, 0, 16)
    out = o.image_tail(torch.empty(0, 5, 4, 4, device=DEV), mean=[0.5] * 5, std=[0.5] * 5)
    assert out.dtype == torch.float32 and tuple(out.shape) == (0, 5, 4, 4)
    u8 = torch.zeros(1, 3, 4, 4, dtype=torch.uint8, device=DEV)
    f32 = torch.zeros(1, 3, 4, 4, device=DEV)
    with pytest.raises(TypeError):
        o.image_tail(f32, jitter=[("brightness", 1.0)])                   # jitter on a float image
    with pytest.raises(TypeError):
        o.image_tail(f32.half(), mean=MEAN, std=STD)
    with pytest.raises(TypeError):
        o.image_tail(u8, mean=MEAN, std=STD)                              # Normalize on uint8 without to_float
    with pytest.raises(ValueError):
        o.image_tail(u8, to_float=True, mean=MEAN[:2], std=STD[:2])       # wrong length
    with pytest.raises(ValueError):
        o.image_tail(f32, mean=MEAN, std=STD + [1.0])
    with pytest.raises(ValueError):
        o.image_tail(f32, mean=MEAN, std=[0.2, 0.0, 0.2])                 # a zero in std
    with pytest.raises(ValueError):
        o.image_tail(u8, jitter=[("brightness", 1.0), ("brightness", 0.5)])
    with pytest.raises(ValueError):
        o.image_tail(u8, jitter=[("hue", 0.1)])
    with pytest.raises(ValueError):
        o.image_tail(u8, jitter=[("contrast", -0.1)])
    with pytest.raises(ValueError):
        o.image_tail(torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device=DEV), jitter=[("contrast", 1.0)])


# ---- the transform classes ------------------------------------------------------------------------------------------

class Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def setting(B, H, W, seed, n_points=40):
    """A SameSettingImageData of B uint8 images of W x H with its own small random mapping (built like
    tests/test_gpu_transforms_golden.py::fresh, no golden needed); B = 0 gives a setting without mapping."""
    from deepviewagg_amd.core.multimodal.image import ImageMapping, SameSettingImageData
    gen = torch.Generator().manual_seed(seed)
    m = None
    if B:
        n = 3 * n_points
        pts, imgs = torch.randint(0, n_points, (n,), generator=gen), torch.randint(0, B, (n,), generator=gen)
        pix = torch.stack([torch.randint(0, W, (n,), generator=gen), torch.randint(0, H, (n,), generator=gen)], 1).short()
        m = ImageMapping.from_dense(pts.to(DEV), imgs.to(DEV), pix.to(DEV), torch.rand(n, 2, generator=gen).to(DEV),
                                    num_points=n_points)
    return SameSettingImageData(path=np.array([f"img_{i}" for i in range(B)]), pos=torch.zeros(B, 3, device=DEV),
                                opk=torch.zeros(B, 3, device=DEV), ref_size=(W, H), proj_upscale=1, mappings=m,
                                x=t(R.images((B, H, W), "random", seed=seed), DEV))


def chain(values, p):
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    return [T.ColorJitter(*values), T.RandomHorizontalFlip(p), T.ToFloatImage(), T.Normalize()]


def run(transforms, images, seed):
    torch.manual_seed(seed)
    data = Data(pos=torch.zeros(40, 3, device=DEV))
    for tr in transforms:
        data, images = tr(data, images)
    return images, torch.rand(1)


def settings_of(images):
    from deepviewagg_amd.core.multimodal.image import ImageData
    return list(images) if isinstance(images, ImageData) else [images]


def assert_same_images(a, b):
    a, b = settings_of(a), settings_of(b)
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.x.dtype == torch.float32 and torch.equal(u.x, v.x)
        assert torch.equal(u.mappings.pixels, v.mappings.pixels)


@pytest.mark.parametrize("values", [(0.6, 0.6, 0.7), (0.2, 0.2, 0.2)], ids=["s3dis", "kitti360"])
@pytest.mark.parametrize("p", [0.0, 1.0])
def test_fused_tail_equals_the_eager_chain(values, p):
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    eager = chain(values, p)
    fused = T.fuse_image_tail(eager)
    assert len(fused) == 1 and type(fused[0]) is T.FusedImageTail
    for seed in (0, 1, 2):
        base = setting(3, 10, 52, seed=seed)
        before = base.mappings.pixels.clone()
        a, next_a = run(eager, copy.deepcopy(base), seed)
        b, next_b = run(fused, copy.deepcopy(base), seed)
        assert_same_images(a, b)
        assert torch.equal(next_a, next_b)
        flipped = 52 - 1 - before[:, 0].long()
        assert torch.equal(a.mappings.pixels[:, 0].long(), flipped if p == 1.0 else before[:, 0].long())


def test_fused_tail_draws_transform_major_on_several_settings():
    """Two settings of different sizes: the eager chain draws both jitters, then both flips.  p = 0.5 makes the flips
    depend on the position of their draws in the stream."""
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    from deepviewagg_amd.core.multimodal.image import ImageData
    eager = chain((0.6, 0.6, 0.7), 0.5)
    fused = T.fuse_image_tail(eager)
    flips = set()
    for seed in range(6):
        base = ImageData([setting(2, 8, 48, seed=seed), setting(3, 6, 20, seed=seed + 50)])
        a, next_a = run(eager, copy.deepcopy(base), seed)
        b, next_b = run(fused, copy.deepcopy(base), seed)
        assert isinstance(b, ImageData) and len(b) == 2
        assert_same_images(a, b)
        assert torch.equal(next_a, next_b)
        flips.add(tuple(bool((u.mappings.pixels != v.mappings.pixels).any()) for u, v in zip(a, base)))
    assert len(flips) > 1                                              # both outcomes of a flip were seen


def test_s3dis_train_names_run_end_to_end_fused():
    """The tail of the S3DIS train_transforms, looked up by name as the reference's factory does, fused, on a device
    setting: the eager chain's result."""
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    spec = [("JitterMappingFeatures", dict(sigma=0.02, clip=0.03)),
            ("ColorJitter", dict(brightness=0.6, contrast=0.6, saturation=0.7)), ("RandomHorizontalFlip", {}),
            ("ToFloatImage", {}), ("Normalize", {})]
    eager = [getattr(T, name)(**params) for name, params in spec]
    fused = T.fuse_image_tail(eager)
    assert [type(f).__name__ for f in fused] == ["JitterMappingFeatures", "FusedImageTail"]
    base = setting(4, 16, 64, seed=9)
    a, next_a = run(eager, copy.deepcopy(base), 9)
    b, next_b = run(fused, copy.deepcopy(base), 9)
    assert_same_images(a, b)
    assert torch.equal(a.mappings.features, b.mappings.features) and torch.equal(next_a, next_b)
    # the eval tail
    eager = [T.ToFloatImage(), T.Normalize()]
    a, _ = run(eager, copy.deepcopy(base), 0)
    b, _ = run(T.fuse_image_tail(eager), copy.deepcopy(base), 0)
    assert_same_images(a, b)
    assert torch.equal(a.x.cpu(), ((base.x.cpu().float() / 255) - torch.tensor(MEAN).view(1, 3, 1, 1))
                       / torch.tensor(STD).view(1, 3, 1, 1))


def test_empty_batch_still_consumes_the_draws():
    """B = 0: nothing is launched, the result is an empty tensor, and the jitter's draws are made all the same."""
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    cj = T.ColorJitter(0.6, 0.6, 0.7)
    base = setting(0, 8, 16, seed=3)
    a, next_a = run([cj], copy.deepcopy(base), 4)
    assert tuple(a.x.shape) == (0, 3, 8, 16) and a.x.dtype == torch.uint8
    torch.manual_seed(4)
    cj.draw()
    assert torch.equal(torch.rand(1), next_a)                          # exactly the jitter's draws were made
    eager = [cj, T.ToFloatImage(), T.Normalize()]
    a, next_a = run(eager, copy.deepcopy(base), 4)
    b, next_b = run(T.fuse_image_tail(eager), copy.deepcopy(base), 4)
    assert tuple(a.x.shape) == (0, 3, 8, 16) and a.x.dtype == torch.float32
    assert tuple(b.x.shape) == (0, 3, 8, 16) and b.x.dtype == torch.float32
    assert torch.equal(next_a, next_b)
