"""ElasticDistortion on the device against the reference's own class (fixtures tests/golden/elastic_*.npz, written by
tools/gen_golden_elastic.py from torch_points3d/core/data_transform/grid_transform.py:194-256 over the real scipy).
Every comparison is exact: same dtype, shape, device and bits."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from deepviewagg_amd import ops
from deepviewagg_amd.core.data_transform import grid_transform as G

pytestmark = pytest.mark.gpu

FIXTURES = ("elastic_room", "elastic_street", "elastic_planar", "elastic_single", "elastic_lattice")
DEV = "cuda:0"


def same(got, want, device=DEV):
    """torch.equal plus dtype, shape and device; ``want`` is a numpy array or a CPU tensor."""
    want = want if torch.is_tensor(want) else torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    assert got.device == torch.device(device), got.device
    return torch.equal(got.cpu(), want)


def levels_of(g):
    """(input pos, granularity, magnitude, noise, field, axes, output pos) of every level, as numpy arrays."""
    cur = g["pos"]
    for l in range(int(g["levels"])):
        yield (cur, float(g["granularity"][l]), float(g["magnitude"][l]), g[f"l{l}_noise"], g[f"l{l}_field"],
               [g[f"l{l}_ax{k}"] for k in range(3)], g[f"l{l}_out_pos"])
        cur = g[f"l{l}_out_pos"]


@pytest.mark.parametrize("name", FIXTURES)
def test_smooth_equals_scipy(name):
    for _, _, _, noise, field, _, _ in levels_of(load_golden(name)):
        keep = noise.copy()
        assert same(ops.elastic_smooth(noise), field)                                    # numpy in
        dev_noise = torch.from_numpy(noise).to(DEV)
        assert same(ops.elastic_smooth(dev_noise), field)                                # device tensor in
        assert np.array_equal(noise, keep) and torch.equal(dev_noise.cpu(), torch.from_numpy(keep))


@pytest.mark.parametrize("name", FIXTURES)
def test_displace_equals_the_interpolator(name):
    for pos, _, m, _, field, axes, out in levels_of(load_golden(name)):
        got = ops.elastic_displace(torch.from_numpy(pos).to(DEV), torch.from_numpy(field).to(DEV), axes, m)
        assert same(got, out)
        got = ops.elastic_displace(torch.from_numpy(pos), field, [torch.from_numpy(a) for a in axes], m)   # CPU in
        assert same(got, out)


@pytest.mark.parametrize("name", FIXTURES)
def test_one_level_equals_the_static_method(name):
    """Device bounds, host noise_dim and axes, smoothing and interpolation, with the reference's noise."""
    for pos, g, m, noise, _, _, out in levels_of(load_golden(name)):
        assert same(ops.elastic_distortion(torch.from_numpy(pos).to(DEV), g, m, noise=noise), out)
        assert same(ops.elastic_distortion(torch.from_numpy(pos), g, m, noise=torch.from_numpy(noise)), out)


def test_bounds_are_exact():
    gen = torch.Generator().manual_seed(3)
    for n in (1, 63, 64, 65, 1000, 65536, 65537, 300001):
        pos = (torch.randn(n, 3, generator=gen) * torch.tensor([1.0, 1e3, 1e-3])).contiguous()
        want = torch.cat([pos.min(0).values, pos.max(0).values])
        assert same(ops.minmax3(pos.to(DEV)), want), n


def test_static_method_draws_the_reference_noise():
    g = load_golden("elastic_room")
    pos, gr, m = torch.from_numpy(g["pos"]), float(g["granularity"][0]), float(g["magnitude"][0])
    for device in ("cpu", DEV):
        np.random.seed(int(g["seed_numpy"]))
        out = G.ElasticDistortion.elastic_distortion(pos.to(device), gr, m)
        assert same(out, g["l0_out_pos"], device)


@pytest.mark.parametrize("device", ["cpu", DEV])
@pytest.mark.parametrize("name", FIXTURES)
def test_class_equals_the_reference_under_its_seeds(name, device):
    g = load_golden(name)
    pos = torch.from_numpy(g["pos"]).to(device)
    n = pos.shape[0]
    y, meta = torch.arange(n, device=device), torch.tensor([3.0, 1.0, 4.0])
    data = SimpleNamespace(pos=pos, y=y, meta=meta, name="scene")
    keep = pos.clone()
    random.seed(int(g["seed_random"]))
    np.random.seed(int(g["seed_numpy"]))
    out = G.ElasticDistortion(granularity=g["granularity"].tolist(), magnitude=g["magnitude"].tolist())(data)
    assert out is data
    assert same(out.pos, g[f"l{int(g['levels']) - 1}_out_pos"], device)
    assert out.y is y and out.meta is meta and out.name == "scene" and sorted(vars(out)) == ["meta", "name", "pos", "y"]
    assert torch.equal(pos, keep)                                   # the input tensor itself is not written
    # the streams are where the reference leaves them: one draw of `random`, the noise of every level of numpy
    random.seed(int(g["seed_random"]))
    random.random()
    state = random.getstate()
    np.random.seed(int(g["seed_numpy"]))
    for l in range(int(g["levels"])):
        np.random.randn(*g[f"l{l}_noise"].shape)
    want_next = np.random.rand()
    random.seed(int(g["seed_random"]))
    np.random.seed(int(g["seed_numpy"]))
    G.ElasticDistortion(granularity=g["granularity"].tolist(), magnitude=g["magnitude"].tolist())(
        SimpleNamespace(pos=pos))
    assert random.getstate() == state and np.random.rand() == want_next


def test_class_takes_a_dict():
    g = load_golden("elastic_lattice")
    random.seed(int(g["seed_random"]))
    np.random.seed(int(g["seed_numpy"]))
    data = {"pos": torch.from_numpy(g["pos"]).to(DEV)}
    out = G.ElasticDistortion(granularity=g["granularity"].tolist(), magnitude=g["magnitude"].tolist())(data)
    assert out is data and same(out["pos"], g["l1_out_pos"])


@pytest.mark.parametrize("device", ["cpu", DEV])
def test_gate_skipping_seed_leaves_pos_and_draws_no_noise(device):
    g = load_golden("elastic_gate")
    pos = torch.from_numpy(g["pos"]).to(device)
    data = SimpleNamespace(pos=pos, y=torch.arange(pos.shape[0]))
    random.seed(int(g["seed_random"]))
    np.random.seed(int(g["seed_numpy"]))
    before = np.random.get_state()
    out = G.ElasticDistortion()(data)
    after = np.random.get_state()
    assert out is data and out.pos is pos and same(out.pos, g["pos"], device)
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_wrong_noise_shape_and_empty_cloud_raise():
    g = load_golden("elastic_room")
    pos = torch.from_numpy(g["pos"]).to(DEV)
    with pytest.raises(ValueError, match="noise of shape"):
        ops.elastic_distortion(pos, 0.2, 0.4, noise=g["l1_noise"])
    with pytest.raises(ValueError, match="noise of shape"):
        ops.elastic_distortion(pos, 0.2, 0.4, noise=g["l0_noise"][..., :2])
    with pytest.raises(ValueError, match="zero-size array"):
        ops.elastic_distortion(torch.zeros(0, 3, device=DEV), 0.2, 0.4)
    with pytest.raises(ValueError, match="zero-size array"):
        G.ElasticDistortion.elastic_distortion(torch.zeros(0, 3), 0.2, 0.4)
    with pytest.raises(ValueError, match="ascending"):
        ops.elastic_displace(pos, g["l0_field"], [g["l0_ax0"][::-1].copy(), g["l0_ax1"], g["l0_ax2"]], 0.4)
    with pytest.raises(ValueError, match="knots"):
        ops.elastic_displace(pos, g["l0_field"], [g["l0_ax0"][:-1], g["l0_ax1"], g["l0_ax2"]], 0.4)
    assert tuple(ops.elastic_displace(pos[:0], g["l0_field"], [g[f"l0_ax{k}"] for k in range(3)], 0.4).shape) == (0, 3)


# ---------------------------------------------------------------------------------------------------------------
# steps 3 to 5 in float64 torch on the host: one torch operation per rounding, so nothing is fused
# ---------------------------------------------------------------------------------------------------------------
def smooth_f64(noise):
    w = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(3.0, dtype=torch.float32)
    w = w.double()
    v = noise
    for _ in range(2):
        for axis in range(3):
            d = v.shape[axis]
            x = v.double()
            zero = torch.zeros_like(x.narrow(axis, 0, 1))
            x = torch.cat([zero, x, zero], dim=axis)
            acc = 0.0 + x.narrow(axis, 0, d) * w
            acc = acc + x.narrow(axis, 1, d) * w
            acc = acc + x.narrow(axis, 2, d) * w
            v = acc.float()
    return v


def displace_f64(pos, field, axes, magnitude):
    x = pos.double()
    inside = torch.ones(x.shape[0], dtype=torch.bool)
    cells, lo, hi = [], [], []
    for k in range(3):
        a, xk = axes[k], x[:, k].contiguous()
        d = a.shape[0]
        i = (torch.searchsorted(a, xk, right=True) - 1).clamp(0, d - 2)        # the largest i with a[i] <= x, clipped
        y = (xk - a[i]) / (a[i + 1] - a[i])
        inside &= ~(xk < a[0]) & ~(xk > a[-1])
        cells.append(i)
        lo.append(1 - y)
        hi.append(y)
    value = torch.zeros(x.shape[0], 3, dtype=torch.float64)
    f = field.double()
    for c0 in (0, 1):                                                          # axis 0 slowest, lower corner first
        for c1 in (0, 1):
            for c2 in (0, 1):
                weight = (hi[0] if c0 else lo[0]) * (hi[1] if c1 else lo[1])
                weight = weight * (hi[2] if c2 else lo[2])
                value = value + f[cells[0] + c0, cells[1] + c1, cells[2] + c2] * weight[:, None]
    value[~inside] = 0.0
    return (x + value * magnitude).float(), inside


def big_case():
    gen = torch.Generator().manual_seed(2021)
    dims, n, step = (60, 50, 20), 1 << 21, 0.2
    noise = torch.randn(*dims, 3, generator=gen)
    start = (-3.1, 1153.25, 115.875)
    axes = [torch.from_numpy(np.linspace(s, s + step * (d - 1), d)) for s, d in zip(start, dims)]
    # uniform over the axes and 2 % beyond them on every side; the first points on knots (as float32) and the ends
    lo = torch.tensor([float(a[0]) for a in axes], dtype=torch.float64)
    hi = torch.tensor([float(a[-1]) for a in axes], dtype=torch.float64)
    u = torch.rand(n, 3, generator=gen, dtype=torch.float64) * 1.04 - 0.02
    pos = (lo + u * (hi - lo)).float()
    m = min(dims)
    pos[:m] = torch.stack([axes[k][:m] for k in range(3)], 1).float()
    pos[m] = torch.stack([a[-1] for a in axes]).float()
    pos[m + 1] = torch.stack([a[0] for a in axes]).float()
    return noise, axes, pos.contiguous()


def test_two_million_points_against_float64_torch():
    noise, axes, pos = big_case()
    field = smooth_f64(noise)
    assert same(ops.elastic_smooth(noise), field)
    want, inside = displace_f64(pos, field, axes, 1.6)
    n_out = int((~inside).sum())
    assert 0.05 * pos.shape[0] < n_out < 0.2 * pos.shape[0]             # both branches are well covered
    assert torch.equal(want[~inside], pos[~inside]) and not torch.equal(want[inside], pos[inside])
    got = ops.elastic_displace(pos.to(DEV), field.to(DEV), axes, 1.6)
    assert same(got, want)


def test_long_axes_take_the_global_memory_path():
    """More knots than the LDS stage holds (4096 over the three axes): same result as the float64 restatement."""
    gen = torch.Generator().manual_seed(5)
    dims = (4200, 3, 2)
    field = smooth_f64(torch.randn(*dims, 3, generator=gen))
    axes = [torch.from_numpy(np.linspace(-2.0, -2.0 + 0.05 * (d - 1), d)) for d in dims]
    lo = torch.tensor([float(a[0]) for a in axes], dtype=torch.float64)
    hi = torch.tensor([float(a[-1]) for a in axes], dtype=torch.float64)
    pos = (lo + (torch.rand(100000, 3, generator=gen, dtype=torch.float64) * 1.02 - 0.01) * (hi - lo)).float()
    want, inside = displace_f64(pos, field, axes, 0.4)
    assert 0 < int((~inside).sum()) < pos.shape[0]
    assert same(ops.elastic_displace(pos.to(DEV), field, axes, 0.4), want)


def test_identical_calls_give_identical_bytes():
    g = load_golden("elastic_street")
    pos = torch.from_numpy(g["pos"]).to(DEV)
    a = ops.elastic_distortion(pos, 0.5, 0.4, noise=g["l0_noise"])
    b = ops.elastic_distortion(pos, 0.5, 0.4, noise=g["l0_noise"])
    assert a.data_ptr() != b.data_ptr() and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    noise, axes, big = big_case()
    field = ops.elastic_smooth(noise)
    assert ops.elastic_smooth(noise).cpu().numpy().tobytes() == field.cpu().numpy().tobytes()
    big = big.to(DEV)
    a, b = ops.elastic_displace(big, field, axes, 1.6), ops.elastic_displace(big, field, axes, 1.6)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_chain_stays_on_the_device(monkeypatch):
    """GridSampling3D -> ElasticDistortion -> GridSampling3D on device input: ElasticDistortion copies nothing of
    the size of pos to the host, and the chain gives the coords of the same chain fed the fixture's recorded noise
    through ops.  The first sampling keeps one of the identical points of every 1 cm voxel of the room, so the bounds
    of both levels, and with them the shapes of the noise, are the fixture's."""
    g = load_golden("elastic_room")
    pos = torch.from_numpy(g["pos"])
    n = pos.shape[0]

    def first(seed):
        torch.manual_seed(seed)
        data = SimpleNamespace(pos=pos.to(DEV), y=torch.arange(n, device=DEV))
        return G.GridSampling3D(0.01, mode="last")(data)

    last = G.GridSampling3D(0.05, quantize_coords=True, mode="last")

    moved = []
    data = first(7)
    m = data.pos.shape[0]
    assert 0.5 * n < m < n and data.pos.is_cuda
    real_to, real_cpu = torch.Tensor.to, torch.Tensor.cpu

    def is_host(args, kwargs):
        target = kwargs.get("device", args[0] if args else None)
        return isinstance(target, (str, torch.device)) and torch.device(target).type == "cpu"

    def to(self, *args, **kwargs):
        if self.is_cuda and is_host(args, kwargs):
            moved.append(self.numel())
        return real_to(self, *args, **kwargs)

    def cpu(self, *args, **kwargs):
        if self.is_cuda:
            moved.append(self.numel())
        return real_cpu(self, *args, **kwargs)

    random.seed(int(g["seed_random"]))
    np.random.seed(int(g["seed_numpy"]))
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "to", to)
        mp.setattr(torch.Tensor, "cpu", cpu)
        data = G.ElasticDistortion()(data)
    assert data.pos.is_cuda and tuple(data.pos.shape) == (m, 3)
    assert moved and max(moved) <= 6, moved                             # the six bounds of every level, nothing else
    a = last(data)

    data = first(7)
    p = data.pos
    for l in range(2):
        p = ops.elastic_distortion(p, float(g["granularity"][l]), float(g["magnitude"][l]), noise=g[f"l{l}_noise"])
    data.pos = p
    b = last(data)
    for k in ("pos", "y", "coords"):
        got, want = getattr(a, k), getattr(b, k)
        assert got.is_cuda and got.dtype == want.dtype and torch.equal(got, want), k
    assert a.coords.dtype == torch.int32 and a.coords.shape[0] == a.pos.shape[0] > 1000
