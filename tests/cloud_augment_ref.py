"""numpy restatement of the arithmetic of ``ops.cloud_augment`` (csrc/cloud_augment.hip, include/dva.h): float32
throughout, every operation rounded on its own, correctly rounded division and square root (numpy's float32 ufuncs).
The CENTER mean is taken from ``math.fsum``: the correctly rounded float64 sum, divided in float64, rounded to float32.

Steps are the tuples ``ops.cloud_augment`` takes.  ``apply(..., consts=rows)`` uses the given rows (the device's) where
it would compute a maximum or a mean; ``stages`` then holds what the restatement itself finds at each reducing step,
which is what the rows are checked against."""
import math

import numpy as np

F32 = np.float32

# the step lists of the shipped chains, with fixed drawn values: the S3DIS / KITTI-360 run (noise, rotate, scale,
# symmetry) and the ScanNet run (rotation with norm, symmetry, scale)
_c, _s = math.cos(math.pi * 37.5 / 180.0), math.sin(math.pi * 37.5 / 180.0)
ROT_Z_T = np.array([[_c, _s, 0], [-_s, _c, 0], [0, 0, 1]], dtype=F32).T.copy()     # RandomRotate passes A^T
ROT_3 = np.array([[0.8137977, -0.44096962, 0.37852232], [0.46984631, 0.88256412, 0.01802831],
                  [-0.34202014, 0.16317591, 0.92541658]], dtype=F32)
SCALE = np.array([0.93, 1.07, 1.012], dtype=F32)
S3DIS_RUN = [("noise",), ("linear", ROT_Z_T, False), ("scale", SCALE), ("flip", (True, False, False))]
SCANNET_RUN = [("linear", ROT_3, True), ("flip", (True, True, False)), ("scale", SCALE)]


def f32_ulp(x):
    """Spacing of float32 at |x| (of the smallest normal below it)."""
    x = abs(float(x))
    return float(np.spacing(F32(max(x, float(np.finfo(F32).tiny)))))


def fsum_mean(col):
    """float32 of (the exact sum of the float32 column, rounded to float64, divided by N in float64); and that float64."""
    mean = math.fsum(col.astype(np.float64).tolist()) / col.shape[0]
    return F32(mean), mean


def _linear(p, M):
    M = np.asarray(M, dtype=F32)
    a, b, c = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    return np.stack([(a * M[i, 0] + b * M[i, 1]) + c * M[i, 2] for i in range(3)], axis=1).astype(F32)


def apply(pos, steps, norm=None, noise=None, consts=None):
    """-> (pos_out, norm_out, consts float32 [R, 3], stages): ``stages[r]`` is ``("max", maxima)`` of the flagged
    columns (0 elsewhere) or ``("mean", float32 means, float64 means)`` as the restatement finds them at reducing step r."""
    p = np.ascontiguousarray(pos, dtype=F32).copy()
    v = None if norm is None else np.ascontiguousarray(norm, dtype=F32).copy()
    rows, stages = [], []
    for step in steps:
        name = step[0]
        if name == "noise":
            p = p + np.asarray(noise, dtype=F32)
        elif name == "linear":
            p = _linear(p, step[1])
            if step[2]:
                v = _linear(v, step[1])
        elif name == "scale":
            s = np.asarray(step[1], dtype=F32)
            p = p * s
            if v is not None:
                v = v / s
                length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
                v = v / np.maximum(length, F32(1e-12))[:, None]
        elif name == "flip":
            mask = np.asarray(step[1], dtype=bool)
            own = np.where(mask, p.max(axis=0), F32(0)).astype(F32)
            stages.append(("max", own))
            m = own if consts is None else np.asarray(consts[len(rows)], dtype=F32)
            rows.append(m)
            p = np.where(mask[None, :], m[None, :] - p, p).astype(F32)
        elif name == "center":
            means = [fsum_mean(p[:, c]) for c in range(3)]
            own = np.array([m[0] for m in means], dtype=F32)
            stages.append(("mean", own, np.array([m[1] for m in means], dtype=np.float64)))
            m = own if consts is None else np.asarray(consts[len(rows)], dtype=F32)
            rows.append(m)
            p = p - m[None, :]
        else:
            raise ValueError(name)
        assert p.dtype == F32 and (v is None or v.dtype == F32)
    return p, v, np.array(rows, dtype=F32).reshape(len(rows), 3), stages


def linear_bound(p, M, k=6):
    """``k * 2^-24 * sum_j |p_j| |M_ij|`` per output element: each of two float32 evaluations of the three-term sum
    (any order, fused or not) lies within 3 * 2^-24 of that magnitude from the exact value, so they lie within 6 of
    each other."""
    return k * 2.0 ** -24 * (np.abs(np.asarray(p, dtype=np.float64)) @ np.abs(np.asarray(M, dtype=np.float64)).T)


def cloud(n, seed, offset=None, scale=(4.0, 3.0, 2.5)):
    """float32 [n, 3] with positive and negative coordinates; ``offset`` moves it to world coordinates."""
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3)) - 0.5) * np.asarray(scale)
    if offset is not None:
        p = p + np.asarray(offset, dtype=np.float64)
    return p.astype(F32)


def normals(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def noise(n, seed, sigma=0.01, clip=0.05):
    rng = np.random.default_rng(seed)
    return np.clip(sigma * rng.standard_normal((n, 3)), -clip, clip).astype(F32)
