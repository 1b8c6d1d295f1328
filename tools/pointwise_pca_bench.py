#!/usr/bin/env python
"""Time PCAComputePointwise's two device stages at the sizes of the shipped data configs (HIP events, no profiler):

  self     10^6 points of a room-like surface cloud, K-NN of every point among them, k = 50
           (S3DIS / ScanNet: PCAComputePointwise(num_neighbors=50) on data.pos)
  full_pos 10^6 queries in a 5 x 10^6-point street-like full cloud, k = 50
           (KITTI-360 with use_full_pos: the voxel-subsampled points searched in data.full_pos)

For each: ops.knn_query (grid build + search, every level) and ops.pointwise_pca, median / min over --reps timed calls
after --warmup untimed ones; the self case also times ops.knn (the self search of NeighborhoodBasedMappingFeatures).
As context, the reference's own path on the same neighbours: batch_pca (features.py:307-329) per chunk of 10^6
points on the CPU in fp32, with torch.linalg.eigh in place of the removed torch.symeig, timed once with the host
clock; its largest eigenvalue difference to the device result is reported.  One JSON line on stdout; --out writes it.

Usage:  python tools/pointwise_pca_bench.py [--reps 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import measure  # noqa: E402


def room(n, gen):
    """Points on the six faces of a 20 x 12 x 4 m room with 40 furniture boxes, 5 mm noise."""
    size = torch.tensor([20.0, 12.0, 4.0])
    axis = torch.randint(0, 3, (n,), generator=gen)
    side = torch.randint(0, 2, (n,), generator=gen).float()
    box = torch.randint(0, 41, (n,), generator=gen)           # 0: the room, 1..40: a box of 1 x 1 x 1 m
    origin = torch.rand(41, 3, generator=gen) * (size - 1.0)
    origin[:, 2] = 0.0
    scale = torch.where(box[:, None] == 0, size, torch.ones(3))
    xyz = torch.rand(n, 3, generator=gen) * scale
    xyz[torch.arange(n), axis] = side * scale[torch.arange(n), axis]
    xyz = xyz + torch.where(box[:, None] == 0, torch.zeros(3), origin[box])
    return xyz + torch.randn(n, 3, generator=gen) * 5e-3


def street(n, gen):
    """A 200 m street: road plane, two facades, poles and cars; 2 cm noise."""
    part = torch.randint(0, 10, (n,), generator=gen)
    u = torch.rand(n, 3, generator=gen)
    xyz = torch.empty(n, 3)
    road = part < 5
    xyz[road] = u[road] * torch.tensor([200.0, 16.0, 0.0]) - torch.tensor([100.0, 8.0, 0.0])
    for p, y in ((5, -8.0), (6, 8.0), (7, -8.0)):
        m = part == p
        xyz[m] = u[m] * torch.tensor([200.0, 0.0, 12.0]) - torch.tensor([100.0, -y, 0.0])
    m = part == 8                                              # poles: 40 vertical segments of 6 m
    pole = torch.randint(0, 40, (n,), generator=gen)[m]
    xyz[m] = torch.stack([pole.float() * 5 - 100, torch.full_like(u[m, 0], 6.5), u[m, 2] * 6], 1)
    m = part == 9                                              # cars: 60 boxes of 4 x 2 x 1.5 m
    car = torch.randint(0, 60, (n,), generator=gen)[m]
    xyz[m] = u[m] * torch.tensor([4.0, 2.0, 1.5]) + torch.stack(
        [car.float() * 3.3 - 100, torch.where(car % 2 == 0, -5.0, 3.0), torch.zeros_like(u[m, 0])], 1)
    return xyz + torch.randn(n, 3, generator=gen) * 0.02


def timed(fn, reps, warmup):
    t = measure.summarise(measure.repeated(fn, reps, measure.event_window, warmup), 3)
    return {"median_ms": t["median"], "min_ms": t["min"], "reps": reps}


def reference_cpu(search, nbr, chunk=1_000_000):
    """features.py:455-470 on the CPU: batch_pca per chunk, fp32, eigh for symeig."""
    evals = []
    for i in range(0, nbr.shape[0], chunk):
        x = search[nbr[i:i + chunk].long()]
        c = x - x.mean(dim=1).unsqueeze(1)
        w, _ = torch.linalg.eigh(c.transpose(1, 2).bmm(c) / c.shape[1], UPLO='U')
        evals.append(w.clamp(min=0))
    return torch.cat(evals)


def case(name, query, search, k, reps, warmup, with_self_knn):
    from deepviewagg_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    q, s = query.to(dev), search.to(dev)
    out = {"n_query": query.shape[0], "n_search": search.shape[0], "k": k}
    out["knn_query"] = timed(lambda: ops.knn_query(q, s, k), reps, warmup)
    if with_self_knn:
        out["knn_self"] = timed(lambda: ops.knn(s, k), reps, warmup)
    nbr, _ = ops.knn_query(q, s, k)
    out["pointwise_pca"] = timed(lambda: ops.pointwise_pca(s, nbr), reps, warmup)
    evals, _ = ops.pointwise_pca(s, nbr)
    nbr_cpu, ref = nbr.cpu(), []
    cpu_ms = measure.host_window(lambda: ref.append(reference_cpu(search, nbr_cpu)))
    ref = ref[0]
    lmax = ref[:, 2:].clamp(min=1e-30)
    out["reference_cpu_batch_pca"] = {"ms": round(cpu_ms, 1), "threads": torch.get_num_threads(),
                                      "max_eigenvalue_diff_over_lmax": float(((evals.cpu() - ref).abs() / lmax).max())}
    print(f"{name}: {json.dumps(out)}", file=sys.stderr)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "pointwise_pca_bench measures the HIP device"
    gen = torch.Generator().manual_seed(0)
    res = measure.header("pointwise_pca_bench")
    cloud = room(1_000_000, gen)
    res["self"] = case("self", cloud, cloud, 50, args.reps, args.warmup, True)
    full = street(5_000_000, gen)
    sub = full[torch.randperm(full.shape[0], generator=gen)[:1_000_000]]
    sub = sub + torch.randn(sub.shape, generator=gen) * 0.02
    res["full_pos"] = case("full_pos", sub, full, 50, args.reps, args.warmup, False)
    measure.emit(res, args.out)


if __name__ == "__main__":
    main()
