"""The contract of the image loading ops, restated in numpy (no PIL, no torch, no package import).

``PIL.Image.resize(size)`` on an RGB image is Pillow's 8-bit BICUBIC resample: per axis a table of fixed-point
coefficients computed in C double (every operation rounded on its own), then int32 multiply-adds over uint8 pixels,
horizontal pass first into a uint8 intermediate, then the vertical pass.  ``read_images`` of the reference
(core/multimodal/image.py:1059-1099) composes it with a roll along the width and a crop or a second resize from a box;
``NonStaticMask`` (core/data_transform/multimodal/image.py:139-154) compares the views it read.

Written with scalar loops over Python floats (C doubles) where the product's table builder is vectorised, so that the
two are independent statements of the same arithmetic.  ``resample_pass`` restates one launch of
``dva_image_resample_u8`` (include/dva.h) so that the product's pass plans can be run on the host.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(in_size, in0, in1, out_size):
    """(ksize, bounds int [out, 2] = (xmin, xmax), k int [out, ksize]) of one axis."""
    in0, in1 = float(in0), float(in1)
    scale = filterscale = (in1 - in0) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    kk = np.zeros((out_size, ksize), dtype=np.int64)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = int(center - support + 0.5)              # int() truncates toward zero, as the C cast
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def _clip8(s):
    assert np.abs(s).max(initial=0) < 2 ** 31, "the int32 accumulator of the contract overflowed"
    return np.clip(s >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_axis(img, axis, in0, in1, out_size):
    """One pass over ``img`` uint8 [H, W, 3] along ``axis`` (0: rows / vertical, 1: columns / horizontal)."""
    _, bounds, kk = coefficients(img.shape[axis], in0, in1, out_size)
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for xx in range(out_size):
        xmin, xmax = bounds[xx]
        s = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for x in range(xmax):
            s = s + src[xmin + x] * kk[xx, x]
        out[xx] = _clip8(s)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize(img, size, box=None):
    """``PIL.Image.fromarray(img).resize(size, box=box)`` for uint8 [H, W, 3]; ``size = (W, H)``."""
    H, W = img.shape[:2]
    Wo, Ho = int(size[0]), int(size[1])
    x0, y0, x1, y1 = (0, 0, W, H) if box is None else box
    assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
    if (Wo, Ho) == (W, H) and (x0, y0, x1, y1) == (0, 0, W, H):
        return img.copy()
    out = img
    if Wo != W or x0 != 0 or x1 != W:
        out = resample_axis(out, 1, x0, x1, Wo)
    if Ho != H or y0 != 0 or y1 != H:
        out = resample_axis(out, 0, y0, y1, Ho)
    return out


def roll(img, delta):
    """The reference's ``pil_roll``: ``new[x] = old[(x + delta) % W]``."""
    W = img.shape[1]
    delta = int(delta) % W
    return img[:, (np.arange(W) + delta) % W]


def read_images(sources, size, rollings=None, crop_size=None, crop_offsets=None, downscale=None):
    """uint8 [B, 3, H, W] of the reference's ``read_images`` over decoded ``sources`` (uint8 [H, W, 3] each)."""
    n = len(sources)
    size = (int(size[0]), int(size[1]))
    rollings = np.zeros(n, dtype=np.int64) if rollings is None else np.asarray(rollings)
    if crop_size is None:
        crop_size, crop_offsets = size, np.zeros((n, 2), dtype=np.int64)
    w, h = int(crop_size[0]), int(crop_size[1])
    out = []
    for img, delta, (left, top) in zip(sources, rollings, np.asarray(crop_offsets)):
        img = roll(resize(img, size), delta)
        left, top = int(left), int(top)
        if downscale is None:
            img = img[top:top + h, left:left + w]
        else:
            end_size = tuple(int(v / downscale) for v in (w, h))
            img = resize(img, end_size, box=(left, top, left + w, top + h))
        out.append(img)
    return np.stack(out).transpose(0, 3, 1, 2)


def nonstatic_mask(images):
    """bool [W, H] of uint8 [n, 3, H, W]: the pixels where some view i >= 1 differs from view 0 in all three channels."""
    mask = np.zeros(images.shape[2:], dtype=bool)
    for other in images[1:]:
        mask |= (images[0] != other).all(axis=0)
    return mask.T


def resample_pass(src, axis, coeffs, bounds, table_index, shifts, periods, out_hw):
    """One launch of ``dva_image_resample_u8`` as include/dva.h states it, on uint8 ``src`` [B, h, w, 3]: ``axis`` 0
    runs along x, 1 along y; returns uint8 [B, ho, wo, 3]."""
    B, h, w, _ = src.shape
    ho, wo = out_hw
    out_period, src_period, other_period = periods
    out = np.empty((B, ho, wo, 3), dtype=np.uint8)
    n_axis, n_other = (wo, ho) if axis == 0 else (ho, wo)
    for b in range(B):
        kk, bb = coeffs[table_index[b]], bounds[table_index[b]]
        s_out, s_src, s_oth = (int(v) for v in shifts[b])
        o = np.arange(n_other) + s_oth
        o = o % other_period if other_period else o
        lines = src[b][o] if axis == 0 else src[b][:, o].transpose(1, 0, 2)      # [other, axis, 3]
        lines = lines.astype(np.int64)
        for i in range(n_axis):
            r = i + s_out
            r = r % out_period if out_period else r
            xmin, xmax = bb[r]
            s = np.full((n_other, 3), 1 << (PRECISION_BITS - 1), dtype=np.int64)
            for x in range(xmax):
                a = xmin + x + s_src
                a = a % src_period if src_period else a
                s = s + lines[:, a] * int(kk[r, x])
            if axis == 0:
                out[b, :, i] = _clip8(s)
            else:
                out[b, i] = _clip8(s)
    return out
