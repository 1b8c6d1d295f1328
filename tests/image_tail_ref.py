"""Two restatements of the image tail's contract (ColorJitter ops, flip, ToFloatImage, Normalize), no test by itself.

``numpy_tail``   the contract as ``ops.image_tail`` documents it: separately rounded float32 steps on numpy arrays, the
                 contrast mean taken from the exact integer sum of the gray image.
``torch_tail``   the torch composition of torchvision 0.8.2's formulas (``functional_tensor._blend``,
                 ``rgb_to_grayscale``, ``adjust_brightness`` / ``_contrast`` / ``_saturation``, ``Normalize``), written
                 out here because torchvision is no dependency: the contrast mean is ``torch.mean`` over
                 ``dim=(-3, -2, -1)``.  It runs on whatever device its input lives on.

For ``H * W * 255 < 2^24`` (``H * W <= 65793``) the float32 sum behind ``torch.mean`` is exact in any order and the
two agree by construction; beyond it ``torch.mean`` depends on torch's summation order and the integer sum is the
project's definition."""
import itertools

import numpy as np
import torch

NAMES = ("brightness", "contrast", "saturation")
# every non-empty subset of the three ops in every order: 3 + 6 + 6 = 15 lists of names
OP_LISTS = [p for k in (1, 2, 3) for p in itertools.permutations(NAMES, k)]
F32 = np.float32


def gray_np(img):
    """uint8 [..., 3, H, W] -> float32 [..., H, W] holding u8((0.2989 r + 0.587 g) + 0.114 b)."""
    r, g, b = (img[..., c, :, :].astype(F32) for c in range(3))
    return np.trunc((F32(0.2989) * r + F32(0.587) * g) + F32(0.114) * b)


def blend_np(p, q, f):
    """u8(clamp(f32(f) p + f32(1.0 - f) q, 0, 255)) on float32 arrays holding integers; 1.0 - f in double."""
    v = F32(f) * p + F32(1.0 - float(f)) * q
    return np.trunc(np.clip(v, F32(0), F32(255)))


def contrast_mean_np(gray_sum, n):
    """m = f32(S) / f32(n) from the integer sum S of the gray image and its pixel count n."""
    return F32(int(gray_sum)) / F32(int(n))


def jitter_np(x, jitter):
    """x uint8 [B, 3, H, W] (numpy) -> uint8 [B, 3, H, W] after the (name, factor) ops in order."""
    img = x.astype(F32)
    n = x.shape[-2] * x.shape[-1]
    for name, f in jitter:
        if name == "brightness":
            img = blend_np(img, np.zeros_like(img), f)
        elif name == "saturation":
            img = blend_np(img, gray_np(img)[:, None], f)
        elif name == "contrast":
            sums = gray_np(img).astype(np.int64).reshape(img.shape[0], -1).sum(axis=1)
            m = np.array([contrast_mean_np(s, n) for s in sums], dtype=F32).reshape(-1, 1, 1, 1)
            img = blend_np(img, m, f)
        else:
            raise ValueError(name)
    return img.astype(np.uint8)


def numpy_tail(x, jitter=(), flip=False, to_float=False, mean=None, std=None):
    """The contract on a numpy array: x uint8 [B, 3, H, W] (or float32 [B, C, H, W] with mean / std alone)."""
    if x.dtype == np.uint8:
        out = jitter_np(x, jitter)
        if flip:
            out = out[..., ::-1]
        if to_float:
            out = out.astype(F32) / F32(255)
    else:
        assert not jitter and not flip and not to_float and x.dtype == F32
        out = x
    if mean is not None:
        m = np.asarray(mean, dtype=F32).reshape(1, -1, 1, 1)
        s = np.asarray(std, dtype=F32).reshape(1, -1, 1, 1)
        out = (out - m) / s
    return np.ascontiguousarray(out)


# ---- the torch composition of torchvision 0.8.2's formulas ------------------------------------------------------

def _blend(img1, img2, ratio):
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255.0).to(img1.dtype)


def _gray(img):
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)


def jitter_torch(img, jitter):
    for name, f in jitter:
        if name == "brightness":
            img = _blend(img, torch.zeros_like(img), f)
        elif name == "saturation":
            img = _blend(img, _gray(img), f)
        elif name == "contrast":
            mean = torch.mean(_gray(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True)
            img = _blend(img, mean, f)
        else:
            raise ValueError(name)
    return img


def torch_tail(x, jitter=(), flip=False, to_float=False, mean=None, std=None):
    """The same chain as eager torch ops on x's device: x uint8 [B, 3, H, W] tensor."""
    out = jitter_torch(x, jitter)
    if flip:
        out = torch.flip(out, [3])
    if to_float:
        out = out.float() / 255
    if mean is not None:
        m = torch.as_tensor(mean, dtype=torch.float32, device=x.device).view(1, -1, 1, 1)
        s = torch.as_tensor(std, dtype=torch.float32, device=x.device).view(1, -1, 1, 1)
        out = (out - m) / s
    return out


def images(shape, kind, seed=0):
    """uint8 [B, 3, H, W] numpy test image: 'random', 'zeros' or 'full' (all 255)."""
    B, H, W = shape
    if kind == "zeros":
        return np.zeros((B, 3, H, W), dtype=np.uint8)
    if kind == "full":
        return np.full((B, 3, H, W), 255, dtype=np.uint8)
    return np.random.default_rng(seed).integers(0, 256, size=(B, 3, H, W), dtype=np.uint8)


def factor_sets(seed=0):
    """Factors per (brightness, contrast, saturation): the clamp on both sides (0.0, 1.7), the identity and random."""
    rng = np.random.default_rng(seed)
    rand = [float(F32(v)) for v in rng.uniform(0.3, 1.7, size=3)]
    return {"zero": (0.0, 0.0, 0.0), "one": (1.0, 1.0, 1.0), "high": (1.7, 1.7, 1.7), "random": tuple(rand)}


def with_factors(names, factors):
    """[(name, factor)] for an op list, the factor of each op taken from a (brightness, contrast, saturation) triple."""
    return [(n, factors[NAMES.index(n)]) for n in names]
