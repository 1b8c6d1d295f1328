#!/usr/bin/env python
"""Write tests/golden/pca_*.npz by running the REFERENCE's own PCAComputePointwise and EigenFeatures
(torch_points3d/core/data_transform/features.py:307-329, :360-485, :488-587).

TEST INFRASTRUCTURE: needs the reference source tree (argument 1, default ../reference next to this repository);
nothing in the package, the tests, smoke() or bench.py runs it; the tests read the committed .npz files.

The reference's features.py is loaded as a single file: the packages its header imports and this image lacks are
placeholders (torch_geometric.nn*, torch_points3d.{datasets,utils,core.spatial_ops}*; none of them is called by
the two transforms), oracle/shims provides pykeops (argKmin: brute force in fp32, ties to the lower index) and
torch_geometric.data.Data.  ``torch.symeig`` no longer exists in torch: it is restated as
``torch.linalg.eigh(A, UPLO='U')`` (symeig's default ``upper=True``).  K-NN through the KeOps branch
(use_faiss=False), PCA in fp32 on the CPU as the reference runs it.

Scenes (each file: inputs, the reference's neighbours, eigenvalues, eigenvectors, EigenFeatures outputs without and
with temperature=5):
  pca_s3dis     self search, planar room faces with noise, n = 3000, k = 50
  pca_kitti     use_full_pos: 1000 queries (a jittered subsample plus points outside the full cloud's box) in a
                6000-point street-like full cloud, k = 50
  pca_voxel     self search on voxel centres (masses of tied distances), k = 26
  pca_degen     self search, k = 16: 40 copies of one point, a collinear line, a coplanar patch, far apart

Usage:  python tools/gen_golden_pointwise_pca.py [REFERENCE_ROOT]
"""
import importlib.util
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shims"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def load_reference_features(ref_root):
    def placeholder(name, attrs=(), is_pkg=False):
        m = types.ModuleType(name)
        if is_pkg:
            m.__path__ = []
        for a in attrs:
            setattr(m, a, type(a, (), {}))
        sys.modules[name] = m
        return m

    placeholder("torch_geometric.nn", ["fps", "radius", "knn", "voxel_grid"], is_pkg=True)
    placeholder("torch_geometric.nn.pool", [], is_pkg=True)
    placeholder("torch_geometric.nn.pool.consecutive", ["consecutive_cluster"])
    placeholder("torch_geometric.nn.pool.pool", ["pool_pos", "pool_batch"])
    for pkg in ("torch_points3d", "torch_points3d.core", "torch_points3d.core.data_transform",
                "torch_points3d.datasets", "torch_points3d.core.spatial_ops"):
        placeholder(pkg, [], is_pkg=True)
    placeholder("torch_points3d.datasets.multiscale_data", ["MultiScaleData"])
    placeholder("torch_points3d.utils", ["is_iterable"], is_pkg=True)
    placeholder("torch_points3d.utils.transform_utils", ["SamplingStrategy"])
    placeholder("torch_points3d.utils.config", ["is_list"])
    placeholder("torch_points3d.utils.geometry", ["euler_angles_to_rotation_matrix"])
    placeholder("torch_points3d.core.spatial_ops.neighbour_finder",
                ["RadiusNeighbourFinder", "FAISSGPUKNNNeighbourFinder"])
    name = "torch_points3d.core.data_transform.features"
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ref_root, "torch_points3d", "core", "data_transform", "features.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def s3dis_scene(gen):
    """Points on the six faces of a 6 x 4 x 3 room, 5 mm noise."""
    n = 3000
    size = torch.tensor([6.0, 4.0, 3.0])
    xyz = torch.rand(n, 3, generator=gen) * size
    axis = torch.randint(0, 3, (n,), generator=gen)
    side = torch.randint(0, 2, (n,), generator=gen).float()
    xyz[torch.arange(n), axis] = side * size[axis]
    return xyz + torch.randn(n, 3, generator=gen) * 5e-3


def kitti_scene(gen):
    """Full cloud: a road plane, two facades and poles; queries: a jittered subsample and points beyond the box."""
    parts = []
    road = torch.rand(3000, 3, generator=gen) * torch.tensor([40.0, 12.0, 0.0]) - torch.tensor([20.0, 6.0, 0.0])
    parts.append(road + torch.randn(3000, 3, generator=gen) * 0.02)
    for y in (-6.0, 6.0):
        f = torch.rand(1200, 3, generator=gen) * torch.tensor([40.0, 0.0, 8.0]) - torch.tensor([20.0, -y, 0.0])
        parts.append(f + torch.randn(1200, 3, generator=gen) * 0.03)
    t = torch.rand(600, generator=gen) * 5
    poles = torch.stack([torch.randint(-3, 4, (600,), generator=gen).float() * 5, torch.full((600,), 4.5), t], 1)
    parts.append(poles + torch.randn(600, 3, generator=gen) * 0.01)
    full = torch.cat(parts)
    sub = full[torch.randperm(full.shape[0], generator=gen)[:960]] + torch.randn(960, 3, generator=gen) * 0.05
    outside = torch.rand(40, 3, generator=gen) * torch.tensor([60.0, 30.0, 20.0]) - torch.tensor([30.0, 15.0, 5.0])
    outside[:20, 0] = 25.0 + torch.rand(20, generator=gen) * 5            # beyond the full cloud's box in x
    outside[20:, 2] = 9.0 + torch.rand(20, generator=gen) * 5             # and in z
    return torch.cat([sub, outside]), full


def voxel_scene(gen):
    c = torch.unique(torch.randint(0, 16, (5000, 3), generator=gen), dim=0)
    c = c[torch.randperm(c.shape[0], generator=gen)[:2000]]
    return (c.float() + 0.5) * 0.05


def degen_scene(gen):
    dup = torch.tensor([[1.25, -2.5, 0.75]]).repeat(40, 1)
    s = torch.arange(60, dtype=torch.float32)
    line = torch.stack([10.0 + 0.1 * s, 0.05 * s, 0.0 * s], 1)              # collinear, exact coordinates
    g = torch.stack(torch.meshgrid(torch.arange(10.0), torch.arange(10.0), indexing="ij"), -1).reshape(-1, 2)
    patch = torch.cat([g * 0.1, torch.full((100, 1), 3.0)], 1) + torch.tensor([0.0, 20.0, 0.0])   # z = const
    return torch.cat([dup, line, patch])


def run(F, Data, name, pos, k, full_pos=None):
    data = Data(pos=pos.clone())
    if full_pos is not None:
        data.full_pos = full_pos.clone()
    data = F.PCAComputePointwise(num_neighbors=k, use_full_pos=full_pos is not None, use_faiss=False)(data)
    # the reference's neighbours: the same KeOps expression its _process evaluates (features.py:423-436)
    search = full_pos if full_pos is not None else pos
    from pykeops.torch import LazyTensor
    d = ((LazyTensor(pos[:, None, :]) - LazyTensor(search[None, :, :])) ** 2).sum(dim=2)
    neighbors = d.argKmin(k, dim=1)
    out = dict(pos=pos, k=np.int64(k), neighbors=neighbors.int(), eigenvalues=data.eigenvalues,
               eigenvectors=data.eigenvectors)
    if full_pos is not None:
        out["full_pos"] = full_pos
    plain = F.EigenFeatures()(Data(eigenvalues=data.eigenvalues.clone(), eigenvectors=data.eigenvectors.clone()))
    hot = F.EigenFeatures(temperature=5)(Data(eigenvalues=data.eigenvalues.clone(),
                                              eigenvectors=data.eigenvectors.clone()))
    for tag, dd in (("", plain), ("_t5", hot)):
        for f in ("norm", "linearity", "planarity", "scattering"):
            out[f + tag] = getattr(dd, f)
    arrays = {key: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
              for key, v in out.items()}
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    F = load_reference_features(ref_root)
    torch.symeig = lambda A, eigenvectors=True: torch.linalg.eigh(A, UPLO='U')
    from torch_geometric.data import Data
    gen = torch.Generator().manual_seed(360)
    run(F, Data, "pca_s3dis", s3dis_scene(gen), 50)
    query, full = kitti_scene(gen)
    run(F, Data, "pca_kitti", query, 50, full_pos=full)
    run(F, Data, "pca_voxel", voxel_scene(gen), 26)
    run(F, Data, "pca_degen", degen_scene(gen), 16)


if __name__ == "__main__":
    main()
