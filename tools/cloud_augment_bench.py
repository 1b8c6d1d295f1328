#!/usr/bin/env python
"""Time the positional 3D augmentations of the shipped train chains on a device-resident cloud, at N = 10^5, 3 * 10^5
and 2^20 points:

  s3dis    RandomNoise(0.001) -> RandomRotate(180, axis=2) -> RandomScaleAnisotropic([0.8, 1.2]) ->
           RandomSymmetry([True, False, False])                           (pos alone; S3DIS and KITTI-360)
  scannet  Random3AxisRotation(rot_x=2, rot_y=2, rot_z=180) -> RandomSymmetry([True, True, False]) ->
           RandomScaleAnisotropic([0.9, 1.1])                             (pos and norm)

five ways each:

  fused       FusedCloudAugment: the members' draws, then one ops.cloud_augment (csrc/cloud_augment.hip)
  eager       the chain of this package's classes, one ops.cloud_augment per class
  torch       the plain torch composition of the reference's lines on the device (CLOUD_AUGMENT_ON_DEVICE = False)
  host_trip   what a user had to do before: copy pos (and norm) to the host, run the composition there, copy back
  draws_only  the members' draw() alone, the noise tensor uploaded: the host work every variant above contains

One process; every variant of a size is warmed up, then the variants alternate inside every repetition; a window is
``inner`` back-to-back applications between two device events, ``inner`` chosen so that a window lasts about --window
seconds; the figure is the median over --reps windows, per application, with the minimum and maximum.  The draws are
live (every application draws anew from the default generators), so a symmetry is applied in about half of them.
Before timing, fused and eager are checked equal bit for bit from the same generator state.

``launches`` are device kernel launches per application with every symmetry drawn: for fused and eager by construction
(one apply kernel per op call and one reduction launch per flip step; the upload of the noise tensor is a copy, not a
launch), for the torch composition counted with torch.profiler where it is available (null otherwise).
One JSON line on stdout; --out writes it (profiles/cloud_augment_bench.json).

Usage:  python tools/cloud_augment_bench.py [--reps 7] [--window 0.2] [--out FILE]
"""
import argparse
import os
import random
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import measure  # noqa: E402

SIZES = (100_000, 300_000, 1 << 20)


def chains():
    from deepviewagg_amd.core.data_transform import augment as A
    return {
        "s3dis": ([A.RandomNoise(0.001, 0.05), A.RandomRotate(180, axis=2), A.RandomScaleAnisotropic([0.8, 1.2]),
                   A.RandomSymmetry([True, False, False])], False),
        "scannet": ([A.Random3AxisRotation(rot_x=2, rot_y=2, rot_z=180), A.RandomSymmetry([True, True, False]),
                     A.RandomScaleAnisotropic([0.9, 1.1])], True),
    }


def seed_with_every_symmetry(members, data):
    """A seed under which every RandomSymmetry of the chain draws all of its axes."""
    from deepviewagg_amd.core.data_transform import augment as A
    for seed in range(1000):
        random.seed(seed)
        torch.manual_seed(seed)
        ok = True
        for m in members:
            steps = m.draw(data)
            if type(m) is A.RandomSymmetry:
                ok = ok and bool(steps) and list(steps[0][1]) == [bool(a) for a in m.axis]
        if ok:
            return seed
    raise RuntimeError("no seed draws every symmetry")


def profiled_kernels(fn, seed):
    try:
        from torch.profiler import ProfilerActivity, profile
        random.seed(seed)
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
        return len(kernels) if kernels else None
    except Exception:
        return None


def run_case(name, n, reps, seconds, gen):
    from deepviewagg_amd.core.data_transform import augment as A
    dev = torch.device("cuda", 0)
    members, with_norm = chains()[name]
    pos = ((torch.rand(n, 3, generator=gen) - 0.5) * torch.tensor([4.0, 3.0, 2.5])).to(dev)
    norm = None
    if with_norm:
        v = torch.randn(n, 3, generator=gen)
        norm = (v / v.norm(dim=1, keepdim=True)).to(dev)
    (fused,) = A.fuse_cloud_augment(members)

    def cloud(device=None):
        d = SimpleNamespace(pos=pos if device is None else pos.to(device))
        if norm is not None:
            d.norm = norm if device is None else norm.to(device)
        return d

    def through(transforms, on_device=True):
        def fn():
            A.CLOUD_AUGMENT_ON_DEVICE = on_device
            try:
                d = cloud()
                for tr in transforms:
                    d = tr(d)
            finally:
                A.CLOUD_AUGMENT_ON_DEVICE = True
            return d
        return fn

    def host_trip():
        d = cloud("cpu")
        for tr in members:
            d = tr(d)
        d.pos = d.pos.to(dev)
        if norm is not None:
            d.norm = d.norm.to(dev)
        return d

    def draws_only():
        d = cloud()
        for tr in members:
            for step in tr.draw(d):
                if step[0] == "noise":
                    step[1].to(dev)

    variants = {"fused": through([fused]), "eager": through(members), "torch": through(members, on_device=False),
                "host_trip": host_trip, "draws_only": draws_only}
    outs = {}
    for kind in ("fused", "eager", "torch"):
        random.seed(1)
        torch.manual_seed(1)
        outs[kind] = variants[kind]()
    assert torch.equal(outs["fused"].pos, outs["eager"].pos), f"{name} {n}: fused and eager differ"
    checks = {"fused_equals_eager": True,
              "torch_max_abs_diff_pos": float((outs["torch"].pos - outs["fused"].pos).abs().max())}
    if norm is not None:
        assert torch.equal(outs["fused"].norm, outs["eager"].norm), f"{name} {n}: fused and eager norms differ"
        checks["torch_max_abs_diff_norm"] = float((outs["torch"].norm - outs["fused"].norm).abs().max())
    del outs
    seed = seed_with_every_symmetry(members, cloud())
    reducing = sum(type(m) in (A.RandomSymmetry, A.Center) for m in members)
    launches = {"fused": 1 + reducing, "eager": len(members) + reducing,
                "torch": profiled_kernels(variants["torch"], seed)}
    ms, inner = measure.alternate(variants, reps, measure.event_window, warmup=3, seconds=seconds, probe_inner=3)
    rows = {}
    for key in variants:
        t = measure.summarise(ms[key], 4)
        rows[key] = {"ms": t["median"], "min_ms": t["min"], "max_ms": t["max"],
                     "applications_per_window": inner[key]}
        if key in launches:
            rows[key]["launches"] = launches[key]
    for other in ("eager", "torch", "host_trip"):
        rows["fused"][f"speedup_vs_{other}"] = round(rows[other]["ms"] / rows["fused"]["ms"], 2)
    return {"chain": name, "n": n, "with_norm": with_norm, "bytes_per_point_fused_pass": 24 * (2 if with_norm else 1),
            "checks": checks, "variants": rows}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    gen = torch.Generator().manual_seed(0)
    result = measure.header(
        "cloud_augment_bench", reps=args.reps, window_s=args.window, host_cpu_threads=torch.get_num_threads(),
        cases=[run_case(name, n, args.reps, args.window, gen) for n in SIZES for name in ("s3dis", "scannet")])
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
