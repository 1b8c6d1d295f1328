#!/usr/bin/env python
"""Write tests/golden/cloud_augment.npz by running the REFERENCE's own RandomNoise, RandomScaleAnisotropic,
RandomSymmetry, ShiftVoxels (torch_points3d/core/data_transform/transforms.py:463-563, :699-723) and
Random3AxisRotation (features.py:30-81, over utils/geometry.py:5-22) on small seeded clouds.

TEST INFRASTRUCTURE: needs the reference source tree (argument 1, default ../reference next to this repository);
nothing in the package, the tests, smoke() or bench.py runs it; the tests read the committed .npz file.

The reference's geometry.py, features.py and transforms.py are loaded as single files, in that order.  Every other
module they import at the top (torch_geometric, torch_scatter, torch_points_kernels, pykeops, numba, sklearn, tqdm,
joblib and the rest of torch_points3d) is a stand-in whose every attribute is an inert placeholder: the five classes
touch torch, numpy and ``random`` alone.  ``torch_points3d.utils.is_iterable`` is the reference's one-liner.

Per case the file holds the inputs, the seed (``random.seed(s)`` and ``torch.manual_seed(s)`` in front of the call),
the reference's outputs, the matrix of a rotation, and the next ``random.random()`` and ``torch.rand(1)`` after the
call, which pin the state the call leaves both generators in.  ``repr_*`` are the reference's repr strings.

Usage:  python tools/gen_golden_cloud_augment.py [REFERENCE_ROOT]
"""
import importlib.abc
import importlib.machinery
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "cloud_augment.npz")

STAND_INS = ("torch_points3d", "torch_geometric", "torch_scatter", "torch_points_kernels", "pykeops", "numba",
             "sklearn", "tqdm", "joblib", "omegaconf")
KITTI_OFFSET = torch.tensor([1153.25, 3907.5, 115.875], dtype=torch.float64)


class Unused:
    """Base class, decorator (with or without arguments) or callable that is never really used."""

    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, *args, **kwargs):
        return args[0] if args and callable(args[0]) else None


class StandIn(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return Unused


class StandInFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in STAND_INS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        return StandIn(spec.name)

    def exec_module(self, module):
        pass


def load_reference(ref_root):
    sys.meta_path.insert(0, StandInFinder())
    import torch_points3d.utils
    torch_points3d.utils.is_iterable = lambda e: isinstance(e, (list, tuple))

    def load(name, *parts):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, "torch_points3d", *parts))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    load("torch_points3d.utils.geometry", "utils", "geometry.py")
    features = load("torch_points3d.core.data_transform.features", "core", "data_transform", "features.py")
    transforms = load("torch_points3d.core.data_transform.transforms", "core", "data_transform", "transforms.py")
    assert transforms.Random3AxisRotation is features.Random3AxisRotation
    return transforms, features


class Data:
    def __init__(self, **kwargs):
        self.__dict__.update(kwargs)


def seed_all(seed):
    random.seed(seed)
    torch.manual_seed(seed)


def next_draws():
    return np.float64(random.random()), torch.rand(1).numpy()


def room(gen, n):
    return (torch.rand(n, 3, generator=gen) * torch.tensor([4.0, 3.0, 2.5]) - torch.tensor([2.0, 1.5, 0.0])).contiguous()


def street(gen, n):
    xyz = torch.rand(n, 3, generator=gen, dtype=torch.float64) * torch.tensor([12.0, 6.0, 3.0], dtype=torch.float64)
    return (xyz + KITTI_OFFSET).float().contiguous()


def unit_normals(gen, n):
    v = torch.randn(n, 3, generator=gen)
    return (v / v.norm(dim=1, keepdim=True)).contiguous()


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    T, F = load_reference(ref_root)
    gen = torch.Generator().manual_seed(2024)
    pos = room(gen, 300)
    far = street(gen, 200)
    norm = unit_normals(gen, 300)
    coords = torch.randint(-400, 400, (300, 3), generator=gen).int()
    arrays = {"pos": pos, "far": far, "norm": norm, "coords": coords}
    cases = []

    def record(tag, seed, transform, data, outputs, **extra):
        seed_all(seed)
        out = transform(data)
        r, t = next_draws()
        arrays[f"{tag}_seed"] = np.int64(seed)
        arrays[f"{tag}_next_random"], arrays[f"{tag}_next_rand"] = r, t
        for key in outputs:
            arrays[f"{tag}_{key}"] = getattr(out, key).clone()
        for key, value in extra.items():
            arrays[f"{tag}_{key}"] = value
        arrays[f"repr_{tag}"] = np.array(repr(transform))
        cases.append(tag)
        print(f"    {tag}: seed {seed}, {repr(transform)}")

    # RandomNoise: the S3DIS values, and a sigma large enough for the clamp to bite, at world offsets
    record("noise", 11, T.RandomNoise(sigma=0.01, clip=0.05), Data(pos=pos.clone()), ["pos"],
           sigma=np.float64(0.01), clip=np.float64(0.05))
    record("noise_far", 12, T.RandomNoise(sigma=0.04, clip=0.05), Data(pos=far.clone()), ["pos"],
           sigma=np.float64(0.04), clip=np.float64(0.05))
    # RandomScaleAnisotropic without and with norm
    record("scale", 21, T.RandomScaleAnisotropic(scales=[0.9, 1.1]), Data(pos=pos.clone()), ["pos"],
           scales=np.array([0.9, 1.1]))
    record("scale_norm", 22, T.RandomScaleAnisotropic(scales=[0.8, 1.2]), Data(pos=pos.clone(), norm=norm.clone()),
           ["pos", "norm"], scales=np.array([0.8, 1.2]))
    # RandomSymmetry: seeds that draw (x, y), x alone, y alone and nothing between them
    seen = set()
    for seed in range(100, 200):
        seed_all(seed)
        drawn = tuple(bool(torch.rand(1) < 0.5) for _ in range(2))
        if drawn in seen:
            continue
        seen.add(drawn)
        record(f"sym_{len(seen)}", seed, T.RandomSymmetry(axis=[True, True, False]), Data(pos=pos.clone()), ["pos"],
               axis=np.array([True, True, False]), drawn=np.array(drawn + (False,)))
        if len(seen) == 4:
            break
    assert len(seen) == 4
    record("sym_far", 31, T.RandomSymmetry(axis=[True, True, True]), Data(pos=far.clone()), ["pos"],
           axis=np.array([True, True, True]))
    # Random3AxisRotation: the ScanNet values with norm, and z alone (one draw of random.random) without
    for tag, seed, kw, data in (
            ("rot", 41, dict(rot_x=2, rot_y=2, rot_z=180), Data(pos=pos.clone(), norm=norm.clone())),
            ("rot_z", 42, dict(rot_z=180), Data(pos=far.clone()))):
        transform = F.Random3AxisRotation(apply_rotation=True, **kw)
        seed_all(seed)
        matrix = transform.generate_random_rotation_matrix()
        record(tag, seed, transform, data, ["pos", "norm"] if tag == "rot" else ["pos"], M=matrix,
               angles=np.array([kw.get("rot_x", 0), kw.get("rot_y", 0), kw.get("rot_z", 0)], dtype=np.float64))
    record("rot_off", 43, F.Random3AxisRotation(apply_rotation=False), Data(pos=pos.clone()), ["pos"])
    # ShiftVoxels
    record("shift", 51, T.ShiftVoxels(), Data(coords=coords.clone()), ["coords"])
    record("shift_off", 52, T.ShiftVoxels(apply_shift=False), Data(coords=coords.clone()), ["coords"])

    arrays["cases"] = np.array(cases)
    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    np.savez_compressed(OUT, **arrays)
    kib = os.path.getsize(OUT) / 1024
    assert kib < 100, kib
    print(f"  cloud_augment.npz  {kib:.1f} KiB")


if __name__ == "__main__":
    main()
