#!/usr/bin/env python
"""Time GridSampling3D on the device at the sizes of the shipped data configs (HIP events, no profiler):

  last  2^20 street-like points, mode 'last' + quantize_coords, x [N, 4], y, mapping_index, size 0.05
        (the per-sample call of every multimodal config: produces data.coords, carries mapping_index)
  mean  2^24 room-like points, mode 'mean', rgb [N, 3], y, setattr_full_pos, size 0.02
        (the pre-collate call on a fused S3DIS area: produces data.full_pos)

For each: the whole transform on device-resident data (median / min over --reps timed calls after --warmup untimed
ones; mode 'last' includes the CPU randperm it draws), the CPU torch.randperm(N) alone, and the device stages
ops.grid_cluster / grid_mean / grid_majority.  As context, a host-CPU restatement of the same step in torch (round,
unique, index_add / bincount), timed once with the host clock.  One JSON line on stdout; --out writes it.

Usage:  python tools/grid_sampling_bench.py [--reps 5] [--warmup 2] [--out FILE]
"""
import argparse
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import measure  # noqa: E402


def street(n, gen):
    """A 100 m street piece: road, two facades, poles; 2 cm noise, at KITTI-360 world offsets."""
    part = torch.randint(0, 8, (n,), generator=gen)
    u = torch.rand(n, 3, generator=gen)
    xyz = u * torch.tensor([100.0, 16.0, 0.0])
    for p, y in ((5, 0.0), (6, 16.0)):
        m = part == p
        xyz[m] = u[m] * torch.tensor([100.0, 0.0, 12.0]) + torch.tensor([0.0, y, 0.0])
    m = part == 7
    xyz[m] = torch.stack([torch.randint(0, 20, (int(m.sum()),), generator=gen).float() * 5,
                          torch.full((int(m.sum()),), 15.0), u[m, 2] * 6], 1)
    return xyz + torch.randn(n, 3, generator=gen) * 0.02 + torch.tensor([1100.0, 3900.0, 115.0])


def room(n, gen):
    """Faces of a 30 x 20 x 4 m area, 5 mm noise (a fused S3DIS area is a few such rooms)."""
    size = torch.tensor([30.0, 20.0, 4.0])
    axis = torch.randint(0, 3, (n,), generator=gen)
    side = torch.randint(0, 2, (n,), generator=gen).float()
    xyz = torch.rand(n, 3, generator=gen) * size
    xyz[torch.arange(n), axis] = side * size[axis]
    return xyz + torch.randn(n, 3, generator=gen) * 5e-3


def timed(fn, reps, warmup):
    t = measure.summarise(measure.repeated(fn, reps, measure.event_window, warmup), 3)
    return {"median_ms": t["median"], "min_ms": t["min"], "reps": reps}


def host_restatement(pos, size, attrs, labels, mode):
    """The same step on the host CPU in torch: quantise, unique, then per-voxel gather / means / majority."""
    coords = torch.round(pos / size).long()
    _, cluster = torch.unique(coords, dim=0, return_inverse=True)
    m = int(cluster.max()) + 1
    if mode == "last":
        perm = torch.randperm(pos.shape[0])
        rep = torch.full((m,), -1, dtype=torch.long).scatter_reduce(0, cluster[perm], torch.arange(pos.shape[0]),
                                                                    "amax")
        _ = [a[perm][rep] for a in attrs + [labels]]
    else:
        count = torch.bincount(cluster, minlength=m).float()
        _ = [torch.zeros((m,) + a.shape[1:]).index_add_(0, cluster, a) / count.view(-1, *([1] * (a.dim() - 1)))
             for a in attrs]
        lab = labels - labels.min()
        nl = int(lab.max()) + 1
        _ = torch.bincount(cluster * nl + lab, minlength=m * nl).view(m, nl).argmax(1)


def run_case(name, n, size, mode, reps, warmup, gen):
    from deepviewagg_amd import ops
    from deepviewagg_amd.core.data_transform.grid_transform import GridSampling3D
    dev = torch.device("cuda", 0)
    if name == "last":
        pos = street(n, gen)
        attrs = {"x": torch.rand(n, 4, generator=gen), "y": torch.randint(-1, 20, (n,), generator=gen),
                 "mapping_index": torch.arange(n)}
        tr = GridSampling3D(size, quantize_coords=True, mode="last")
    else:
        pos = room(n, gen)
        attrs = {"rgb": torch.rand(n, 3, generator=gen), "y": torch.randint(-1, 13, (n,), generator=gen)}
        tr = GridSampling3D(size, mode="mean", setattr_full_pos=True)
    pos_d = pos.to(dev)
    attrs_d = {k: v.to(dev) for k, v in attrs.items()}

    def transform():
        return tr(SimpleNamespace(pos=pos_d, **attrs_d))

    out = transform()
    res = {"n": n, "size": size, "mode": mode, "n_voxels": int(out.pos.shape[0]),
           "transform": timed(transform, reps, warmup)}
    ms = measure.repeated(lambda: torch.randperm(n), reps, measure.host_window, warmup=0)
    res["cpu_randperm_ms"] = measure.summarise(ms, 3)["median"]
    rank = torch.randperm(n).to(dev) if mode == "last" else None
    res["grid_cluster"] = timed(lambda: ops.grid_cluster(pos_d, size, rank=rank), reps, warmup)
    cl = ops.grid_cluster(pos_d, size, rank=rank)
    counts = (cl.offsets[1:] - cl.offsets[:-1]).cpu()
    res["points_per_voxel"] = {"median": int(counts.median()), "max": int(counts.max())}
    if mode == "mean":
        res["grid_mean_rgb"] = timed(lambda: ops.grid_mean(attrs_d["rgb"], cl), reps, warmup)
        res["grid_mean_pos"] = timed(lambda: ops.grid_mean(pos_d, cl), reps, warmup)
        res["grid_majority_y"] = timed(lambda: ops.grid_majority(attrs_d["y"], cl), reps, warmup)
    else:
        res["index_select_x"] = timed(lambda: attrs_d["x"].index_select(0, cl.rep), reps, warmup)
    floats = [v for v in attrs.values() if v.is_floating_point()]
    if mode == "last":
        floats = floats + [attrs["mapping_index"]]
    host = lambda: host_restatement(pos, size, floats + ([pos] if mode == "mean" else []), attrs["y"], mode)
    res["host_cpu_restatement_ms"] = round(measure.host_window(host), 1)
    res["host_cpu_threads"] = torch.get_num_threads()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    gen = torch.Generator().manual_seed(0)
    result = measure.header("grid_sampling_bench")
    result["last"] = run_case("last", 1 << 20, 0.05, "last", args.reps, args.warmup, gen)
    result["mean"] = run_case("mean", 1 << 24, 0.02, "mean", args.reps, args.warmup, gen)
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
