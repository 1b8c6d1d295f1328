#!/usr/bin/env python
"""Time ops.radius_query on the device (HIP events, no profiler) at the sizes of an evaluation tiling:

  2^20 and 2^24 area-like points (a 60 x 40 x 8 m block at KITTI-360 world offsets, uniform) x 4, 256 and 2048 centres,
  spheres (dims = 3, radius 2 m) and cylinders (dims = 2, radius 2 m); the centres are points of the cloud.

For each case: the whole call on a device-resident cloud (median / min over --reps timed calls after --warmup untimed
ones; it includes the one host read that sizes ``idx`` and the allocations), the number of members, and the rate of
(point, centre) pairs tested.  As context, the host time of the reference's way on the same inputs: scikit-learn's
``KDTree(leaf_size=50)`` build and ``query_radius`` one centre at a time, for at most --host-centres centres, when
scikit-learn is importable; otherwise a numpy float64 brute force over at most 16 centres.  The record says which,
and how many centres were timed.  Timed once with the host clock.  One JSON line on stdout; --out writes it.

Usage:  python tools/radius_sampling_bench.py [--reps 5] [--warmup 2] [--host-centres 256] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import measure  # noqa: E402

RADIUS = 2.0


def area(n, gen):
    xyz = torch.rand(n, 3, generator=gen) * torch.tensor([60.0, 40.0, 8.0])
    return (xyz + torch.tensor([1153.25, 3907.5, 115.875])).contiguous()


def timed(fn, reps, warmup):
    t = measure.summarise(measure.repeated(fn, reps, measure.event_window, warmup), 3)
    return {"median_ms": t["median"], "min_ms": t["min"], "reps": reps}


def host_times(pos, centres_by_b, dims, host_centres):
    """Host time of the same queries: {"method", "build_ms", "query_ms": {B: ms}, "centres_timed": {B: count}}."""
    p = pos.numpy()[:, :dims]
    res = {"query_ms": {}, "centres_timed": {}}
    try:
        from sklearn.neighbors import KDTree
    except ImportError:
        KDTree = None
    if KDTree is not None:
        res["method"] = "sklearn KDTree(leaf_size=50).query_radius, one centre at a time"
        built = []
        res["build_ms"] = round(measure.host_window(lambda: built.append(KDTree(p, leaf_size=50))), 1)
        tree = built[0]
    else:
        res["method"] = "numpy float64 brute force, one centre at a time"
        p64 = p.astype(np.float64)
        host_centres = min(host_centres, 16)
    for B, centres in centres_by_b.items():
        c = centres.numpy()[:host_centres]

        def queries():
            for row in c:
                if KDTree is not None:
                    tree.query_radius(row[np.newaxis], r=RADIUS)
                else:
                    d = ((p64 - row) ** 2).sum(1)
                    np.nonzero(d <= RADIUS * RADIUS)
        res["query_ms"][str(B)] = round(measure.host_window(queries), 1)
        res["centres_timed"][str(B)] = int(c.shape[0])
    return res


def run_cloud(n, centre_counts, reps, warmup, host_centres, gen):
    from deepviewagg_amd import ops
    dev = torch.device("cuda", 0)
    pos = area(n, gen)
    pos_d = pos.to(dev)
    out = {"n": n, "radius": RADIUS}
    for dims, name in ((3, "sphere"), (2, "cylinder")):
        centres_by_b = {}
        cases = {}
        for B in centre_counts:
            centres = pos[torch.randint(0, n, (B,), generator=gen), :dims].double()
            centres_by_b[B] = centres
            ptr, idx = ops.radius_query(pos_d, centres, RADIUS, dims=dims)
            members = int(ptr[-1])
            del idx
            t = timed(lambda: ops.radius_query(pos_d, centres, RADIUS, dims=dims), reps, warmup)
            t.update(centres=B, members=members,
                     giga_pairs_per_s=round(2 * n * B / (t["median_ms"] * 1e-3) / 1e9, 1))   # count + fill passes
            cases[str(B)] = t
        out[name] = {"device": cases, "host": host_times(pos, centres_by_b, dims, host_centres)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-centres", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    gen = torch.Generator().manual_seed(0)
    result = measure.header("radius_sampling_bench", host_cpu_threads=torch.get_num_threads(),
                            clouds=[run_cloud(n, (4, 256, 2048), args.reps, args.warmup, args.host_centres, gen)
                                    for n in (1 << 20, 1 << 24)])
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
