#!/usr/bin/env python
"""Time ElasticDistortion on the device at the sizes of a training sample and of a whole area:

  1.5 x 10^5 points of an 8 x 6 x 3 m room (a ScanNet scene after the first grid sampling) and 2^22 points of a
  30 x 20 x 5 m floor, both default levels (granularity 0.2 / 0.8, magnitude 0.4 / 1.6), pos resident on the device.

For each cloud: the whole transform as the data pipeline calls it (host clock around a synchronised call: median /
min over --reps calls after --warmup untimed ones), and its parts, each timed on its own over both levels --
``noise_draw_ms`` (``np.random.randn(...).astype(float32)`` on the host), ``upload_ms`` (the noise to the device),
``bounds_ms`` (the bounds kernel and the synchronising read of its six floats), ``smooth_ms`` and ``displace_ms``
(HIP events around the kernels alone, inputs resident).  ``host_share`` = (noise draw + upload + bounds) / whole.
Where scipy is importable the same levels are also timed on the host with the scipy calls the reference makes (six
``ndimage.convolve`` and one ``RegularGridInterpolator`` per level), once, with the host clock.
One JSON line on stdout; --out writes it (profiles/elastic_distortion_bench.json).

Usage:  python tools/elastic_distortion_bench.py [--reps 7] [--warmup 2] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import measure  # noqa: E402

GRANULARITY, MAGNITUDE = [0.2, 0.8], [0.4, 1.6]
CLOUDS = (("scannet_scene", 150000, (8.0, 6.0, 3.0)), ("area_2^22", 1 << 22, (30.0, 20.0, 5.0)))


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3), round(min(ms), 3)


def events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 3)


def host_level(pos, granularity, magnitude):
    """One level with scipy on the host: the calls the reference makes, restated."""
    from scipy import ndimage
    from scipy.interpolate import RegularGridInterpolator
    third = np.float32(1) / np.float32(3)
    lo = pos.min(0)
    dim = ((pos - lo).max(0) // granularity).astype(int) + 3
    noise = np.random.randn(*dim, 3).astype(np.float32)
    for _ in range(2):
        for axis in range(3):
            shape = [1, 1, 1, 1]
            shape[axis] = 3
            noise = ndimage.convolve(noise, np.full(shape, third, dtype=np.float32), mode="constant", cval=0)
    ax = [np.linspace(a, b, d) for a, b, d in zip(lo - granularity, lo + granularity * (dim - 2), dim)]
    interp = RegularGridInterpolator(ax, noise, bounds_error=False, fill_value=0)
    return (pos + interp(pos) * magnitude).astype(np.float32)


def run_cloud(name, n, extent, reps, warmup, gen):
    from deepviewagg_amd import ops
    from deepviewagg_amd.core.data_transform.grid_transform import ElasticDistortion
    dev = torch.device("cuda", 0)
    pos = (torch.rand(n, 3, generator=gen) * torch.tensor(extent)).contiguous()
    pos_d = pos.to(dev)
    transform = ElasticDistortion(apply_distorsion=True, granularity=GRANULARITY, magnitude=MAGNITUDE)

    def whole():
        # the 0.95 gate would skip one call in twenty: time the loop over the levels itself
        out = pos_d
        for g, m in zip(transform._granularity, transform._magnitude):
            out = transform.elastic_distortion(out, g, m)
        return out

    total, total_min = wall(whole, reps, warmup)
    # the parts, level by level on the inputs of that level
    parts = {"noise_draw_ms": 0.0, "upload_ms": 0.0, "bounds_ms": 0.0, "smooth_ms": 0.0, "displace_ms": 0.0}
    dims = []
    cur = pos_d
    for g, m in zip(GRANULARITY, MAGNITUDE):
        b = ops.minmax3(cur).cpu().numpy()
        dim = ((b[3:] - b[:3]) // g).astype(int) + 3
        dims.append([int(d) for d in dim])
        ax = [np.linspace(a, c, d) for a, c, d in zip(b[:3] - g, b[:3] + g * (dim - 2), dim)]
        parts["noise_draw_ms"] += wall(lambda: np.random.randn(*dim, 3).astype(np.float32), reps, 1)[0]
        noise = np.random.randn(*dim, 3).astype(np.float32)
        parts["upload_ms"] += wall(lambda: torch.from_numpy(noise).to(dev), reps, 1)[0]
        parts["bounds_ms"] += wall(lambda: ops.minmax3(cur).cpu(), reps, warmup)[0]
        noise_d = torch.from_numpy(noise).to(dev)
        parts["smooth_ms"] += events(lambda: ops.elastic_smooth(noise_d), reps, warmup)
        field = ops.elastic_smooth(noise_d)
        axes_d = [torch.from_numpy(a) for a in ax]
        parts["displace_ms"] += events(lambda: ops.elastic_displace(cur, field, axes_d, m), reps, warmup)
        cur = ops.elastic_displace(cur, field, ax, m)
    parts = {k: round(v, 3) for k, v in parts.items()}
    host_ms = parts["noise_draw_ms"] + parts["upload_ms"] + parts["bounds_ms"]
    out = {"cloud": name, "n": n, "extent_m": list(extent), "noise_dims": dims,
           "device": {"whole_ms": total, "whole_min_ms": total_min, "reps": reps, **parts,
                      "host_share": round(host_ms / total, 3)}}
    try:
        import scipy  # noqa: F401
    except ImportError:
        out["host"] = None
        return out
    p = pos.numpy()
    t0 = time.perf_counter()
    for g, m in zip(GRANULARITY, MAGNITUDE):
        p = host_level(p, g, m)
    out["host"] = {"method": "scipy.ndimage.convolve x 6 + RegularGridInterpolator per level, timed once",
                   "whole_ms": round((time.perf_counter() - t0) * 1e3, 1)}
    out["speedup"] = round(out["host"]["whole_ms"] / total, 1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    gen = torch.Generator().manual_seed(0)
    np.random.seed(0)
    result = measure.header(
        "elastic_distortion_bench", host_cpu_threads=torch.get_num_threads(), granularity=GRANULARITY,
        magnitude=MAGNITUDE, clouds=[run_cloud(name, n, extent, args.reps, args.warmup, gen) for name, n, extent in CLOUDS])
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
