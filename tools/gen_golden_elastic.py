#!/usr/bin/env python
"""Write tests/golden/elastic_*.npz by running the REFERENCE's own ElasticDistortion
(torch_points3d/core/data_transform/grid_transform.py:194-256) over the real scipy.

TEST INFRASTRUCTURE: needs the reference source tree (argument 1, default ../reference next to this repository) and
scipy; nothing in the package, the tests, smoke() or bench.py runs it; the tests read the committed .npz files.

The reference's grid_transform.py is loaded as in tools/gen_golden_grid_sampling.py.  While its class runs under
recorded seeds of ``random`` (the 0.95 gate) and ``numpy.random`` (the noise), ``np.random.randn`` and
``scipy.interpolate.RegularGridInterpolator`` are wrapped to record, per level, the drawn noise, the knot axes, the
smoothed field (the interpolator's ``values``) and the float64 interpolant.  Nothing the reference computes is changed.

For every level the tool asserts that the restatement the device code implements equals the reference BIT FOR BIT --
``noise_dim`` and the axes from the six bounds with the reference's numpy expressions, the smoothing as float64 sums
of three neighbours times ``w = float64(float32(1) / 3)`` in ascending order from 0.0 stored as float32 after every
pass, the interpolant with the cell of ``numpy.searchsorted(side="right") - 1`` clipped to [0, d - 2] and the corners
in ``itertools.product`` order, ``out = float32(float64(pos) + value * magnitude)`` -- so that a change of scipy or
numpy shows up here and not as a GPU failure.  It also asserts that the static method under the numpy seed alone gives
the class's first level.

Files (keys: pos, seed_random, seed_numpy, granularity, magnitude, applied, levels, repr and per level l
l{l}_noise_dim, l{l}_ax0, l{l}_ax1, l{l}_ax2, l{l}_noise, l{l}_field, l{l}_out_pos; the transform's output is the
last level's out_pos, asserted here, or pos when the gate skipped it):
  elastic_room     16 k room points, both default levels
  elastic_street   a street at KITTI-360 world offsets (float32 spacing 2.4e-4 in y), levels 0.5 / 2.0
  elastic_planar   a planar cloud: extent 0 and noise_dim 3 on z in the first level
  elastic_single   one point: noise_dim (3, 3, 3) in both levels
  elastic_lattice  a 1/4 lattice at granularity 0.25: in the first level every point sits on a knot of every axis and
                   the largest coordinates on the last cell's lower knot, the upper bound of the cell index
  elastic_gate     seeds for which the 0.95 gate skips the transform: levels = 0, the output is pos, no noise is drawn

Usage:  python tools/gen_golden_elastic.py [REFERENCE_ROOT]
"""
import itertools
import os
import random
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import scipy.interpolate  # noqa: E402
import scipy.ndimage  # noqa: E402
import torch  # noqa: E402

import gen_golden_grid_sampling as GG  # noqa: E402  (also puts oracle/shims on sys.path)

MAX_KIB = 600


# ---------------------------------------------------------------------------------------------------------------
# the restatement (what csrc/elastic.hip and ops.elastic_distortion compute)
# ---------------------------------------------------------------------------------------------------------------
def bounds_restated(pos, granularity):
    """noise_dim and the axes from the six bounds alone, with the reference's numpy expressions."""
    coords_min = pos.min(0)
    extent = pos.max(0) - coords_min                    # fp32(x - min) is monotone in x
    noise_dim = (extent // granularity).astype(int) + 3
    ax = [
        np.linspace(d_min, d_max, d)
        for d_min, d_max, d in zip(coords_min - granularity, coords_min + granularity * (noise_dim - 2), noise_dim)
    ]
    return noise_dim, ax


def smooth_restated(noise):
    w = np.float64(np.float32(1) / np.float32(3))
    v = noise
    for _ in range(2):
        for axis in range(3):
            d = v.shape[axis]
            pad = [(0, 0)] * 4
            pad[axis] = (1, 1)
            x = np.pad(v.astype(np.float64), pad)
            taps = [np.take(x, np.arange(o, o + d), axis=axis) for o in range(3)]
            acc = 0.0 + taps[0] * w
            acc = acc + taps[1] * w
            acc = acc + taps[2] * w
            v = acc.astype(np.float32)
    return v


def interp_restated(ax, field, pos):
    x = pos.astype(np.float64)
    inside = np.ones(x.shape[0], dtype=bool)
    cells, lo, hi = [], [], []
    for k in range(3):
        a, d = ax[k], ax[k].shape[0]
        i = np.clip(np.searchsorted(a, x[:, k], side="right") - 1, 0, d - 2)
        y = (x[:, k] - a[i]) / (a[i + 1] - a[i])
        inside &= ~(x[:, k] < a[0]) & ~(x[:, k] > a[-1])
        cells.append(i)
        lo.append(1 - y)
        hi.append(y)
    value = np.zeros((x.shape[0], 3))
    for c in itertools.product((0, 1), repeat=3):       # axis 0 slowest, lower corner first
        weight = np.ones(x.shape[0])
        for k in range(3):
            weight = weight * (hi[k] if c[k] else lo[k])
        value = value + field[cells[0] + c[0], cells[1] + c[1], cells[2] + c[2]].astype(np.float64) * weight[:, None]
    value[~inside] = 0.0
    return value, cells, hi


def level_restated(pos, granularity, magnitude, noise):
    noise_dim, ax = bounds_restated(pos, granularity)
    field = smooth_restated(noise)
    value, cells, y = interp_restated(ax, field, pos)
    out = (pos.astype(np.float64) + value * magnitude).astype(np.float32)
    return noise_dim, ax, field, value, out, cells, y


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# running the reference with its numpy / scipy calls recorded
# ---------------------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.noise, self.axes, self.field, self.value = [], [], [], []

    def __enter__(self):
        rec = self
        self._randn, self._rgi = np.random.randn, scipy.interpolate.RegularGridInterpolator

        def randn(*shape):
            out = rec._randn(*shape)
            rec.noise.append(out.astype(np.float32))
            return out

        class Interpolator(self._rgi):
            def __init__(self, points, values, **kw):
                rec.axes.append([np.array(p) for p in points])
                rec.field.append(np.array(values))
                super().__init__(points, values, **kw)

            def __call__(self, xi, *a, **kw):
                out = super().__call__(xi, *a, **kw)
                rec.value.append(np.array(out))
                return out

        np.random.randn = randn
        scipy.interpolate.RegularGridInterpolator = Interpolator
        return self

    def __exit__(self, *exc):
        np.random.randn = self._randn
        scipy.interpolate.RegularGridInterpolator = self._rgi


def applied_seed(start, want):
    """The first seed >= start of ``random`` whose first draw passes (want) or fails the reference's 0.95 gate."""
    for s in range(start, start + 10000):
        random.seed(s)
        if (random.random() < 0.95) == want:
            return s
    raise AssertionError("no seed found")


def gen_scene(G, Data, name, pos, granularity, magnitude, seed_random, seed_numpy, applied=True, check=None):
    pos = pos.contiguous()
    assert pos.dtype == torch.float32
    seed_random = applied_seed(seed_random, applied)
    transform = G.ElasticDistortion(granularity=granularity, magnitude=magnitude)
    random.seed(seed_random)
    np.random.seed(seed_numpy)
    data = Data(pos=pos.clone(), y=torch.arange(pos.shape[0]))
    with Recorder() as rec, warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)       # scipy.ndimage.filters, the reference's spelling
        out = transform(data)
    assert out is data and torch.equal(out.y, torch.arange(pos.shape[0]))
    levels = len(rec.noise)
    assert levels == (len(granularity) if applied else 0) and len(rec.field) == len(rec.value) == levels
    arrays = dict(pos=pos, seed_random=np.int64(seed_random), seed_numpy=np.int64(seed_numpy),
                  granularity=np.asarray(granularity, dtype=np.float64),
                  magnitude=np.asarray(magnitude, dtype=np.float64), applied=np.bool_(applied),
                  levels=np.int64(levels), repr=np.array(repr(transform)))
    cur = pos.numpy()
    for l in range(levels):
        g, m = granularity[l], magnitude[l]
        noise_dim, ax, field, value, nxt, cells, y = level_restated(cur, g, m, rec.noise[l])
        assert tuple(noise_dim) + (3,) == rec.noise[l].shape, (name, l)
        assert rec.field[l].dtype == np.float32 and same_bits(field, rec.field[l]), (name, l, "smoothing")
        for k in range(3):
            assert ax[k].dtype == np.float64 and same_bits(ax[k], rec.axes[l][k]), (name, l, "axis", k)
        assert same_bits(value, rec.value[l]), (name, l, "interpolant")
        if check is not None:
            check(l, cur, ax, cells, y)
        if l == 0:          # the static method alone, under the numpy seed alone
            np.random.seed(seed_numpy)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", DeprecationWarning)
                first = G.ElasticDistortion.elastic_distortion(pos.clone(), g, m)
            assert first.dtype == torch.float32 and same_bits(first.numpy(), nxt), (name, "static method")
        arrays[f"l{l}_noise_dim"] = noise_dim.astype(np.int64)
        for k in range(3):
            arrays[f"l{l}_ax{k}"] = ax[k]
        arrays[f"l{l}_noise"] = rec.noise[l]
        arrays[f"l{l}_field"] = field
        arrays[f"l{l}_out_pos"] = nxt
        cur = nxt
        print(f"    {name}: level {l}  noise_dim {tuple(int(d) for d in noise_dim)}  "
              f"max |shift| {float(np.abs(value * m).max()):.3f}")
    assert out.pos.dtype == torch.float32 and same_bits(out.pos.numpy(), cur), (name, "output")
    if not applied:
        assert torch.equal(out.pos, pos)
    save(name, arrays)


def save(name, arrays):
    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
              for k, v in arrays.items()}
    path = os.path.join(GG.OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    kib = os.path.getsize(path) / 1024
    assert kib < MAX_KIB, (name, kib)
    print(f"  {name}.npz  {kib:.1f} KiB")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    G, Data = GG.load_reference_grid_transform(ref_root)
    gen = torch.Generator().manual_seed(1917)
    default = dict(granularity=[0.2, 0.8], magnitude=[0.4, 1.6])

    gen_scene(G, Data, "elastic_room", GG.room_scene(gen, n=16000), seed_random=101, seed_numpy=201, **default)

    gen_scene(G, Data, "elastic_street", GG.street_scene(gen, n=9000), granularity=[0.5, 2.0], magnitude=[0.4, 1.6],
              seed_random=102, seed_numpy=202)

    planar = torch.rand(5000, 3, generator=gen) * torch.tensor([3.0, 2.0, 0.0]) + torch.tensor([0.5, -1.0, 0.75])

    def check_planar(l, cur, ax, cells, y):
        if l == 0:
            assert ax[2].shape[0] == 3 and float(cur[:, 2].max()) == float(cur[:, 2].min())

    gen_scene(G, Data, "elastic_planar", planar, seed_random=103, seed_numpy=203, check=check_planar, **default)

    def check_single(l, cur, ax, cells, y):
        assert [a.shape[0] for a in ax] == [3, 3, 3]

    gen_scene(G, Data, "elastic_single", torch.tensor([[1.25, -0.375, 2.0625]]), seed_random=104, seed_numpy=204,
              check=check_single, **default)

    q = torch.arange(0, 9, dtype=torch.float32) / 4
    lattice = torch.stack(torch.meshgrid(q, q[:7], q[:5], indexing="ij"), -1).reshape(-1, 3) - torch.tensor(
        [1.0, 0.5, 2.0])
    lattice = lattice[torch.randperm(lattice.shape[0], generator=gen)]

    def check_lattice(l, cur, ax, cells, y):
        if l == 0:
            for k in range(3):
                d = ax[k].shape[0]
                assert (y[k] == 0).all(), k                               # every point on a knot
                assert (ax[k][cells[k]] == cur[:, k]).all(), k
                assert int(cells[k].max()) == d - 2 and int(cells[k].min()) == 1, k

    gen_scene(G, Data, "elastic_lattice", lattice, granularity=[0.25, 0.5], magnitude=[0.4, 1.6], seed_random=105,
              seed_numpy=205, check=check_lattice)

    small = torch.rand(1000, 3, generator=gen) * torch.tensor([4.0, 3.0, 2.5])
    gen_scene(G, Data, "elastic_gate", small, seed_random=106, seed_numpy=206, applied=False, **default)


if __name__ == "__main__":
    main()
