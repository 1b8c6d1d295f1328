"""GPU: ``ops.cloud_augment`` (csrc/cloud_augment.hip) against its numpy restatement (tests/cloud_augment_ref.py), the
classes of core/data_transform/augment.py on a device cloud against the reference's fixture, ``FusedCloudAugment``
against the eager chain, and the S3DIS chain end to end on the device.

Sizes: one lane's chunk is 4 points and a block 256 lanes, so 1, 2, 63 ... 257 run the scalar tail, the vector path and
both in one block; 1000 is the largest single-block size class and 70001 launches 69 blocks per reduction, whose partial
rows the next launch combines."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cloud_augment_ref as R
import test_cloud_augment_host as H
from deepviewagg_amd import ops
from deepviewagg_amd.core.data_transform import augment as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 70001]
WORLD = (102345.25, -98761.5, 115.875)            # KITTI-360 world scale

LISTS = {
    "noise": [("noise",)],
    "linear": [("linear", R.ROT_Z_T, False)],
    "linear_norm": [("linear", R.ROT_3, True)],
    "scale": [("scale", R.SCALE)],
    "scale_plain": [("scale", R.SCALE)],
    "flip_x": [("flip", (True, False, False))],
    "center": [("center",)],
    "s3dis": R.S3DIS_RUN,
    "scannet": R.SCANNET_RUN,
    "center_flip_center": [("center",), ("flip", (False, True, True)), ("center",)],
    "flip_xyz": [("flip", (True, True, True))],
}
WITH_NORM = ("linear_norm", "scale", "scannet")

_CLOUDS = {}


def inputs(n, kind):
    """(pos, norm, noise) numpy arrays of a size and kind, made once."""
    if (n, kind) not in _CLOUDS:
        pos = R.cloud(n, seed=n, offset=WORLD if kind == "world" else None)
        _CLOUDS[(n, kind)] = (pos, R.normals(n, seed=n + 1), R.noise(n, seed=n + 2))
    return _CLOUDS[(n, kind)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_and_check(pos_t, steps, norm_t=None, noise_t=None):
    """One call against the restatement, under the rules of the module docstring of cloud_augment_ref."""
    keep = [None if x is None else x.clone() for x in (pos_t, norm_t, noise_t)]
    out, norm_out, consts = ops.cloud_augment(pos_t, steps, norm=norm_t, noise=noise_t)
    again = ops.cloud_augment(pos_t, steps, norm=norm_t, noise=noise_t)
    torch.cuda.synchronize()
    for x, k in zip((pos_t, norm_t, noise_t), keep):                       # the inputs are not written
        assert x is None or torch.equal(x, k)
    for a, b in zip((out, norm_out, consts), again):                       # the same call gives the same bytes
        assert (a is None and b is None) or np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    n_reduce = sum(s[0] in ("flip", "center") for s in steps)
    assert consts.shape == (n_reduce, 3) and consts.dtype == torch.float32 and consts.is_cuda
    assert out.data_ptr() != pos_t.data_ptr() and out.is_contiguous()
    rows = consts.cpu().numpy()
    want, want_norm, _, stages = R.apply(pos_t.cpu().numpy(), steps, norm=None if norm_t is None else norm_t.cpu().numpy(),
                                         noise=None if noise_t is None else noise_t.cpu().numpy(), consts=rows)
    for r, stage in enumerate(stages):
        if stage[0] == "max":                                              # the exact column maxima, 0 elsewhere
            assert np.array_equal(bits(rows[r]), bits(stage[1])), (r, rows[r], stage[1])
        else:
            for c in range(3):
                mean = float(stage[2][c])
                print(f"center row {r} axis {c}: device {rows[r, c]!r} fsum {stage[1][c]!r} exact {mean!r}")
                assert abs(float(rows[r, c]) - mean) <= (0.5 + 2.0 ** -20) * R.f32_ulp(mean), (r, c)
                assert abs(float(rows[r, c]) - float(stage[1][c])) <= R.f32_ulp(mean), (r, c)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    touched = norm_t is not None and any((s[0] == "linear" and s[2]) or s[0] == "scale" for s in steps)
    if touched:
        assert np.array_equal(bits(norm_out.cpu().numpy()), bits(want_norm))
    else:
        assert norm_out is norm_t
    return out, norm_out, consts


@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("n", SIZES)
def test_op_matches_the_restatement(n, name):
    pos, norm, noise = inputs(n, "room")
    steps = LISTS[name]
    run_and_check(dev(pos), steps, dev(norm) if name in WITH_NORM else None,
                  dev(noise) if any(s[0] == "noise" for s in steps) else None)


@pytest.mark.parametrize("name", ["s3dis", "center_flip_center", "center", "flip_xyz"])
@pytest.mark.parametrize("n", [257, 70001])
def test_op_at_world_scale(n, name):
    pos, _, noise = inputs(n, "world")
    assert np.abs(pos[:, :2]).min() > 9e4
    run_and_check(dev(pos), LISTS[name], None, dev(noise) if name == "s3dis" else None)


@pytest.mark.parametrize("n", [65, 1000])
def test_op_takes_non_contiguous_and_unaligned_views(n):
    pos, norm, noise = inputs(n, "room")
    wide = torch.zeros(n, 5, device=DEV)
    wide[:, 1:4] = dev(pos)
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    run_and_check(view, LISTS["s3dis"] + [("center",)], None, dev(noise))
    # a contiguous slice whose first row is not 16-byte aligned: the point-by-point path on every chunk
    shifted = dev(np.concatenate([pos[:1], pos]))[1:]
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 != 0
    run_and_check(shifted, LISTS["scannet"], dev(norm), None)


def test_op_empty_cloud_launches_nothing():
    timer, ops.TIMER = ops.TIMER, ops.KernelTimer()
    try:
        empty = torch.zeros(0, 3, device=DEV)
        out, norm_out, consts = ops.cloud_augment(empty, LISTS["scannet"] + [("center",)], norm=empty.clone())
        assert out.shape == (0, 3) and norm_out.shape == (0, 3) and consts.shape == (2, 3)
        data = SimpleNamespace(pos=empty)
        torch.manual_seed(1)
        data = A.FusedCloudAugment([A.RandomNoise(), A.RandomSymmetry([True, True, True]), A.Center()])(data)
        assert data.pos.shape == (0, 3) and data.pos.is_cuda
        after = torch.rand(1)
        torch.manual_seed(1)
        torch.randn(0, 3), [torch.rand(1) for _ in range(3)]
        assert torch.equal(torch.rand(1), after)                            # the draws were consumed
        assert ops.TIMER.records == []
    finally:
        ops.TIMER = timer


# ---- the classes on a device cloud ------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", H.CASES)
def test_classes_on_device_match_the_reference(tag):
    transform, data = H.make(tag)
    cpu = {k: v.clone() for k, v in data.items()}
    H.seed_all(H.G[f"{tag}_seed"])
    out = transform({k: v.to(DEV) for k, v in data.items()})
    H.check_state(tag)                                                      # the state the CPU run (the reference) leaves
    for k, v in out.items():
        assert v.is_cuda, (tag, k)
    H.check_against_golden(tag, out, cpu.get("pos"), cpu.get("norm"))


def s3dis_members():
    return [A.RandomNoise(0.01, 0.05), A.RandomRotate(180, axis=2), A.RandomScaleAnisotropic([0.9, 1.1]),
            A.RandomSymmetry([True, False, False])]


def scannet_members():
    return [A.Random3AxisRotation(rot_x=2, rot_y=2, rot_z=180), A.RandomSymmetry([True, True, False]),
            A.RandomScaleAnisotropic([0.9, 1.1])]


def cloud_attrs(n, seed):
    pos, norm, _ = inputs(n, "room")
    return dict(pos=dev(pos), norm=dev(norm), y=torch.arange(n, device=DEV) + seed, tag="cloud")


def container(kind, attrs):
    return SimpleNamespace(**attrs) if kind == "namespace" else dict(attrs)


def attr(data, key):
    return data[key] if isinstance(data, dict) else getattr(data, key)


@pytest.mark.parametrize("kind", ["namespace", "dict", "list"])
@pytest.mark.parametrize("members", [s3dis_members, scannet_members], ids=["s3dis", "scannet"])
def test_fused_equals_the_eager_chain(members, kind):
    def build():
        if kind == "list":
            return [container("namespace", cloud_attrs(1000, 0)), container("dict", cloud_attrs(257, 1))]
        return container(kind, cloud_attrs(1000, 0))
    for seed in (0, 1, 2):                                                  # symmetry drawn and not drawn
        H.seed_all(seed)
        eager = build()
        for transform in members():
            eager = transform(eager)
        state = (random.random(), torch.rand(1))
        H.seed_all(seed)
        src = build()
        held = [(attr(d, "y"), attr(d, "tag")) for d in (src if kind == "list" else [src])]
        (fused,) = A.fuse_cloud_augment(members())
        timer, ops.TIMER = ops.TIMER, ops.KernelTimer()
        try:
            got = fused(src)
            calls = len(ops.TIMER.records)
        finally:
            ops.TIMER = timer
        assert (random.random(), torch.rand(1)) == state
        pairs = list(zip(got, eager)) if kind == "list" else [(got, eager)]
        assert calls == len(pairs)                                          # one op call per cloud
        for (g, e), (y, tag) in zip(pairs, held):
            assert np.array_equal(bits(attr(g, "pos").cpu().numpy()), bits(attr(e, "pos").cpu().numpy()))
            assert np.array_equal(bits(attr(g, "norm").cpu().numpy()), bits(attr(e, "norm").cpu().numpy()))
            assert attr(g, "y") is y and attr(g, "tag") is tag


def test_composition_lies_within_the_bounds_of_the_device_route(monkeypatch):
    """CLOUD_AUGMENT_ON_DEVICE = False runs the torch composition on the device tensors.  Noise, scale on pos and flip
    are the device route's results bit for bit; a rotation lies within 6 * 2^-24 * sum_j |p_j| |M_ij|; Center within the
    error of torch's float32 mean -- any summation order of N float32 terms is within (N - 1) * 2^-24 * sum |x| of the
    exact sum -- plus the roundings of the two means and of the subtractions (one ulp of the largest coordinate)."""
    n = 300
    pos = inputs(1000, "world")[0][:n]
    norm = inputs(1000, "room")[1][:n]

    def both(make_transform, seed, with_norm=False):
        outs = []
        for on_device in (True, False):
            monkeypatch.setattr(A, "CLOUD_AUGMENT_ON_DEVICE", on_device)
            H.seed_all(seed)
            data = dict(pos=dev(pos))
            if with_norm:
                data["norm"] = dev(norm)
            outs.append(make_transform()(data))
        return outs

    for make_transform in (lambda: A.RandomNoise(0.01, 0.05), lambda: A.RandomScaleAnisotropic([0.9, 1.1]),
                           lambda: A.RandomSymmetry([True, True, True])):
        for seed in (0, 1):
            d, c = both(make_transform, seed)
            assert np.array_equal(bits(d["pos"].cpu().numpy()), bits(c["pos"].cpu().numpy()))
    for make_transform, with_norm in ((lambda: A.RandomRotate(180, axis=2), False),
                                      (lambda: A.Random3AxisRotation(rot_x=2, rot_y=2, rot_z=180), True)):
        H.seed_all(4)
        step = make_transform().draw(dict(pos=pos, norm=norm) if with_norm else dict(pos=pos))[0]
        d, c = both(make_transform, 4, with_norm)
        for key, src in (("pos", pos), ("norm", norm))[:2 if with_norm else 1]:
            diff = np.abs(d[key].cpu().numpy().astype(np.float64) - c[key].cpu().numpy().astype(np.float64))
            assert (diff <= R.linear_bound(src, step[1].numpy())).all(), key
    d, c = both(A.Center, 0)
    diff = np.abs(d["pos"].cpu().numpy().astype(np.float64) - c["pos"].cpu().numpy().astype(np.float64))
    p64 = np.abs(pos.astype(np.float64))
    bound = (n - 1) * 2.0 ** -24 * p64.sum(axis=0) / n + np.array([R.f32_ulp(m) for m in p64.max(axis=0)])
    print("center: composition - device", diff.max(axis=0), "bound", bound)
    assert (diff <= bound[None, :]).all()


# ---- end to end ---------------------------------------------------------------------------------------------------

def test_s3dis_chain_end_to_end_on_the_device():
    from deepviewagg_amd.core.data_transform import grid_transform as GT
    from deepviewagg_amd.core.data_transform import transforms as T
    rng = np.random.default_rng(7)
    n = 36000
    room = (rng.random((n, 3)) * np.array([4.0, 3.0, 2.5])).astype(np.float32)
    data = SimpleNamespace(pos=dev(room), rgb=dev(rng.random((n, 3)).astype(np.float32)),
                           y=dev(rng.integers(0, 13, n)), mapping_index=torch.arange(n, device=DEV))
    H.seed_all(9)
    np.random.seed(9)
    data = T.SphereSampling(1.0, np.array([2.0, 1.5, 1.25]))(data)
    sampled = data.pos.shape[0]
    assert 4000 < sampled < 6500
    head = A.fuse_cloud_augment([A.RandomNoise(0.001, 0.05), A.RandomRotate(180, axis=2),
                                 A.RandomScaleAnisotropic([0.8, 1.2]), A.RandomSymmetry([True, False, False]),
                                 A.XYZFeature(add_z=True), A.AddFeatsByKeys([True, True], ["rgb", "pos_z"]), A.Center()])
    assert [type(h) for h in head] == [A.FusedCloudAugment, A.XYZFeature, A.AddFeatsByKeys, A.FusedCloudAugment]
    tail = [GT.GridSampling3D(0.05, quantize_coords=True, mode="last"), A.ShiftVoxels()]
    for transform in head:
        data = transform(data)
    per_point = ("pos", "rgb", "y", "mapping_index", "pos_z", "x")
    assert all(getattr(data, k).is_cuda and getattr(data, k).shape[0] == data.pos.shape[0] for k in per_point)
    assert data.x.shape[1] == 4 and abs(float(data.pos.mean())) < 1e-5
    host = SimpleNamespace(**{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in vars(data).items()})
    state, py_state = torch.get_rng_state(), random.getstate()
    for transform in tail:
        data = transform(data)
    torch.set_rng_state(state)
    random.setstate(py_state)
    for transform in tail:
        host = transform(host)
    for k in per_point + ("coords",):                  # grid_size is the reference's CPU scalar tensor on either route
        assert getattr(data, k).is_cuda, k
    assert data.coords.dtype == torch.int32 and 0 < data.coords.shape[0] < sampled
    assert not host.coords.is_cuda
    assert torch.equal(data.coords.cpu(), host.coords)
    assert torch.equal(data.mapping_index.cpu(), host.mapping_index)
    assert torch.equal(data.x.cpu(), host.x)
