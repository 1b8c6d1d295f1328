"""-m gpu: ops.image_window (csrc/image_tail.hip, dva_image_window_u8) against the numpy oracle
tests/image_window_ref.py::window_np composed with tests/image_tail_ref.py::numpy_tail, and the deferred online chains
(DeferImages / defer_image_windows) against the eager ones.  No tolerance anywhere: fp32 outputs are compared on their
raw bytes."""
import copy
import itertools

import numpy as np
import pytest
import torch

import image_tail_ref as R
import image_window_ref as WR
from conftest import t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# [4, 3, 9, 37]: every source alignment and planes that do not share it; [5, 3, 12, 40]: rows alternate between 16-byte
# and 8-byte alignment; [3, 3, 64, 128]: every row 16-byte aligned, the alignment of a chunk is the window's alone
SOURCES = [(5, 12, 40), (4, 9, 37), (3, 64, 128)]
JITTERS = [(), (("saturation", 1.3), ("contrast", 0.7), ("brightness", 1.1)),
           (("contrast", 1.45), ("brightness", 0.6), ("saturation", 0.4))]
# every subset of {jitter (two orders), flip, to_float, normalize} that ops.image_tail accepts (Normalize needs to_float)
TAILS = [dict(jitter=j, flip=f, to_float=tf, **(dict(mean=MEAN, std=STD) if nm else {}))
         for j, f, (tf, nm) in itertools.product(JITTERS, (False, True), ((False, False), (True, False), (True, True)))]


def ops():
    from deepviewagg_amd import ops as o
    return o


def same(got, want):
    want = torch.from_numpy(np.array(want, order="C", copy=True))     # (a flipped width-1 array keeps a negative stride)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert torch.equal(got.cpu().contiguous().view(torch.uint8), want.view(torch.uint8))


def source(shape, seed):
    N, H, W = shape
    return np.random.default_rng(seed).integers(0, 256, size=(N, 3, H, W), dtype=np.uint8)


def windows(shape, Wc, rng):
    """(index, rolls, offsets, Hc) for one call on a source of ``shape``: eight output images whose windows begin at
    the source columns ``starts`` -- 16-byte aligned, dword aligned, odd, and with the wrap column W inside a chunk
    (W - 5, W - 2) or exactly on a chunk boundary (W - 16, W - 4) -- split at random into offset and roll (some rolls
    beyond W or negative); the index is permuted and repeats entries."""
    N, H, W = shape
    starts = np.array([0, 4, 1, W - 5, W - 16, W - 4, W - 2, 7]) % W
    index = np.array([3, 0, N - 1, 0, 1, 2, 3, 1]) % N
    Hc = int(rng.integers(1, H + 1))
    ox = rng.integers(0, W - Wc + 1, size=8)
    rolls = (ox - starts) % W + W * rng.integers(-1, 3, size=8)
    offsets = np.stack([ox, rng.integers(0, H - Hc + 1, size=8)], 1)
    assert ((offsets[:, 0] - rolls) % W == starts).all()
    return index, rolls, offsets, Hc


def load_classes(shape, Wc, index, rolls, offsets, Hc, vec, flip):
    """Which source cases the chunks of one call meet, restated from the kernel's header: for a full chunk that does
    not pass the wrap column, the alignment of its plane-0 source address (the base of a torch allocation is 512-byte
    aligned); for the others, where the wrap column falls."""
    N, H, W = shape
    seen = set()
    for b in range(len(index)):
        x0 = (offsets[b, 0] - rolls[b]) % W
        for y in range(Hc):
            row = ((index[b] * 3) * H + offsets[b, 1] + y) * W
            for c0 in range(0, Wc, vec):
                n = min(vec, Wc - c0)
                s = (x0 + (Wc - c0 - n if flip else c0)) % W
                if n < vec or (Hc * Wc) % vec or ((b * 3 * Hc + y) * Wc + c0) % vec:
                    seen.add("partial")                                   # not full, or no aligned destination
                elif s + vec > W:
                    seen.add("wrap_inside")
                else:
                    a = row + s
                    seen.add("aligned16" if a % 16 == 0 else "dword" if a % 4 == 0 else "odd")
                    if s + vec == W and c0 + vec < Wc:
                        seen.add("wrap_boundary")
    return seen


@pytest.mark.parametrize("shape", SOURCES, ids=lambda s: "x".join(map(str, s)))
def test_window_matches_the_oracle(shape):
    """Widths 1, 3, 4, 16, 17, 32 and W times the 18 tails; the eight windows of a call cover the source cases."""
    N, H, W = shape
    src = source(shape, seed=W)
    srcd = t(src, DEV)
    rng = np.random.default_rng(H)
    seen = {4: set(), 16: set()}
    for Wc in (1, 3, 4, 16, 17, 32, W):
        index, rolls, offsets, Hc = windows(shape, Wc, rng)
        win = WR.window_np(src, index, rolls, offsets, (Wc, Hc))
        args = (srcd, t(index, DEV), t(rolls, DEV), t(offsets, DEV), (Wc, Hc))
        for kw in TAILS:
            got = ops().image_window(*args, **kw)
            same(got, R.numpy_tail(win, **kw))
            seen[4 if kw["to_float"] else 16] |= load_classes(shape, Wc, index, rolls, offsets, Hc,
                                                             4 if kw["to_float"] else 16, kw["flip"])
    assert torch.equal(srcd.cpu(), torch.from_numpy(src))                 # the source is not modified
    for vec in (4, 16):
        assert seen[vec] >= {"aligned16", "dword", "odd", "wrap_inside", "wrap_boundary", "partial"}, (vec, seen[vec])


def test_defaults_are_the_whole_image_unrolled():
    src = source((4, 9, 37), seed=1)
    srcd = t(src, DEV)
    index = torch.tensor([2, 0, 3], device=DEV)
    same(ops().image_window(srcd, index), src[[2, 0, 3]])
    same(ops().image_window(srcd, index, to_float=True, mean=MEAN, std=STD),
         R.numpy_tail(src[[2, 0, 3]], to_float=True, mean=MEAN, std=STD))
    rolls = torch.tensor([5, 0, 36], device=DEV)
    same(ops().image_window(srcd, index, rollings=rolls), WR.window_np(src, [2, 0, 3], [5, 0, 36], np.zeros((3, 2)), (37, 9)))
    off = torch.tensor([[3, 1], [0, 0], [29, 4]], device=DEV)
    same(ops().image_window(srcd, index, offsets=off, size=(8, 5)),
         WR.window_np(src, [2, 0, 3], [0, 0, 0], off.cpu().numpy(), (8, 5)))


def test_contrast_mean_is_taken_over_the_window_alone():
    """255 everywhere but in the windows, whose pixels are <= 16: a mean taken over the image, the source rows or the
    unrolled columns would lift every output byte above 16."""
    N, H, W, Wc, Hc = 3, 64, 128, 32, 16
    rng = np.random.default_rng(3)
    src = np.full((N, 3, H, W), 255, dtype=np.uint8)
    index, rolls = np.array([2, 0, 1, 0]), np.array([0, 100, 135, -7])
    offsets = np.array([[96, 48], [10, 0], [50, 20], [0, 7]])
    for b, i in enumerate(index):
        cols = (offsets[b, 0] + np.arange(Wc) - rolls[b]) % W
        src[i][:, offsets[b, 1]:offsets[b, 1] + Hc, cols] = rng.integers(0, 17, size=(3, Hc, Wc), dtype=np.uint8)
    win = WR.window_np(src, index, rolls, offsets, (Wc, Hc))
    assert win.max() <= 16
    args = (t(src, DEV), t(index, DEV), t(rolls, DEV), t(offsets, DEV), (Wc, Hc))
    for jitter in ([("contrast", 0.5)], [("brightness", 1.0), ("contrast", 0.25)]):
        for kw in (dict(), dict(flip=True, to_float=True)):
            want = R.numpy_tail(win, jitter=jitter, **kw)
            got = ops().image_window(*args, jitter=jitter, **kw)
            same(got, want)
            assert float(got.max()) <= (16 / 255 if kw else 16)
    # and the mean is per output image, also for two windows of one source image
    batched = ops().image_window(*args, jitter=[("contrast", 0.5)])
    for b in range(4):
        one = tuple(a[b:b + 1] for a in args[1:4])
        assert torch.equal(batched[b:b + 1], ops().image_window(args[0], *one, (Wc, Hc), jitter=[("contrast", 0.5)]))


def test_the_same_call_twice_gives_the_same_bytes():
    shape = (3, 64, 128)
    src = t(source(shape, seed=8), DEV)
    index, rolls, offsets, Hc = windows(shape, 32, np.random.default_rng(8))
    args = (src, t(index, DEV), t(rolls, DEV), t(offsets, DEV), (32, Hc))
    kw = dict(jitter=JITTERS[1], flip=True, to_float=True, mean=MEAN, std=STD)
    first = ops().image_window(*args, **kw)
    second = ops().image_window(*args, **kw)
    assert torch.equal(first.view(torch.uint8), second.view(torch.uint8))


def test_out_of_range_windows_are_clamped_not_read():
    """index and offsets are device data: values out of range are the caller's error, their pixels unspecified, but
    every read stays inside the source (the call returns and the source is intact)."""
    src = source((2, 9, 37), seed=2)
    srcd = t(src, DEV)
    index = torch.tensor([-5, 7, 1], device=DEV)
    offsets = torch.tensor([[0, -3], [2 ** 40, 100], [-9, 8]], device=DEV)
    rolls = torch.tensor([2 ** 50, -2 ** 50, 3], device=DEV)
    out = ops().image_window(srcd, index, rolls, offsets, (16, 4), jitter=[("contrast", 0.5)], to_float=True)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (3, 3, 4, 16) and bool(torch.isfinite(out).all())
    assert torch.equal(srcd.cpu(), torch.from_numpy(src))


def test_empty_batch_and_errors():
    o = ops()
    src = t(source((2, 8, 16), seed=0), DEV)
    none = torch.empty(0, dtype=torch.long, device=DEV)
    out = o.image_window(src, none, size=(4, 2), jitter=[("contrast", 0.5)])
    assert out.dtype == torch.uint8 and tuple(out.shape) == (0, 3, 2, 4)
    out = o.image_window(src, none, to_float=True, mean=MEAN, std=STD)
    assert out.dtype == torch.float32 and tuple(out.shape) == (0, 3, 8, 16)
    out = o.image_window(src[:0], none, size=(4, 2))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (0, 3, 2, 4)
    one = torch.zeros(1, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError):
        o.image_window(src[:0], one)                                       # an image of an empty source
    with pytest.raises(ValueError):
        o.image_window(src, one, size=(17, 8))
    with pytest.raises(ValueError):
        o.image_window(src, one, size=(16, 9))
    with pytest.raises(ValueError):
        o.image_window(src, one, size=(0, 4))
    with pytest.raises(ValueError):
        o.image_window(src[:, :2], one)
    with pytest.raises(TypeError):
        o.image_window(src.float(), one)
    with pytest.raises(TypeError):
        o.image_window(src, one.int())
    with pytest.raises(TypeError):
        o.image_window(src, one, rollings=torch.zeros(2, dtype=torch.long, device=DEV))
    with pytest.raises(TypeError):
        o.image_window(src, one, offsets=torch.zeros(1, 3, dtype=torch.long, device=DEV))
    with pytest.raises(TypeError):
        o.image_window(src, one, mean=MEAN, std=STD)                       # Normalize without to_float
    with pytest.raises(ValueError):
        o.image_window(src, one, jitter=[("hue", 0.1)])
    with pytest.raises(ValueError):
        o.image_window(src, one, jitter=[("contrast", 1.0), ("contrast", 0.5)])


# ---- the deferred chains ----------------------------------------------------------------------------------------------

def tail(T, p):
    return [T.JitterMappingFeatures(sigma=0.02, clip=0.03), T.ColorJitter(0.6, 0.6, 0.7), T.RandomHorizontalFlip(p),
            T.ToFloatImage(), T.Normalize()]


@pytest.mark.parametrize("roll", [True, False], ids=["s3dis", "kitti360"])
def test_deferred_chain_equals_the_eager_chain(roll):
    """The S3DIS train chain, and the KITTI-360 one (no CenterRoll), both ending in the tail: defer_image_windows(chain)
    against fuse_image_tail(chain) from equal generator states."""
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    from deepviewagg_amd.core.multimodal.image import WindowedSameSettingImageData
    sizes, flips = set(), set()
    for seed in range(4):
        data, images = WR.golden_setting(DEV, seed=seed)
        chain = WR.s3dis_head(T, roll=roll) + tail(T, 0.5)
        eager, deferred = T.fuse_image_tail(chain), T.defer_image_windows(chain)
        assert type(deferred[0]) is T.DeferImages and type(deferred[-1]) is T.FusedImageTail
        # up to the tail the deferred chain has moved no pixel
        _, head, _ = WR.run_chain(deferred[:-2], copy.deepcopy(data), copy.deepcopy(images), seed)
        assert all(type(im) is WindowedSameSettingImageData and im.is_deferred for im in head)
        _, a, next_a = WR.run_chain(eager, copy.deepcopy(data), copy.deepcopy(images), seed)
        _, b, next_b = WR.run_chain(deferred, copy.deepcopy(data), copy.deepcopy(images), seed)
        assert all(im.x.dtype == torch.float32 and not im.is_deferred for im in b)
        WR.assert_same_settings(a, b)
        assert next_a == next_b
        sizes |= {tuple(im.crop_size) for im in a}
    assert len(sizes) >= 2 and any(s != (128, 64) for s in sizes), sizes


def test_a_reader_of_x_in_the_chain_gets_the_eager_bytes():
    """AddPixelHeightFeature knows nothing of the deferral: it reads x (the uint8 window) and sets a float x."""
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    data, images = WR.golden_setting(DEV, seed=1)
    chain = WR.s3dis_head(T) + [T.ToFloatImage(), T.AddPixelHeightFeature()]
    _, a, next_a = WR.run_chain(chain, copy.deepcopy(data), copy.deepcopy(images), 1)
    _, b, next_b = WR.run_chain([T.DeferImages()] + chain, copy.deepcopy(data), copy.deepcopy(images), 1)
    assert all(im.x.shape[1] == 4 for im in b)
    WR.assert_same_settings(a, b)
    assert next_a == next_b
