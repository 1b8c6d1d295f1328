"""What a strided sparse convolution needs before it can run -- output coordinates, both kernel maps, the parent index --
by the composition (``Conv3d._build_composition`` + ``ops.voxel_parent_index``: torch operators, two host reads, three
hash tables) against the device level (``Conv3d._build_level`` over ``ops.voxel_level``: one sort), on the same device in
the same process, the two alternating.

    python tools/voxel_level_bench.py [--reps 7] [--seconds 0.1] [--voxels 300000 1048576] [--out profiles/voxel_level_bench.json]

Voxels: the surface cloud of tools/sparse_conv_bench.py at 3 * 10^5 and 2^20 voxels.  Rows:

* ``level_1_2`` / ``level_2_4`` / ``level_4_8``: one kernel_size 2 / stride 2 level on a tensor with cold caches; the
  coarser tensors are the output voxels of the level before.  The device route of ``level_1_2`` reads the coordinate
  bounds (one per input tensor); the coarser levels find them in the cache, as they do in a model.
* ``encoder_first_forward``: the first forward of four ``ResNetDown`` stages (eval, no grad) on a tensor with cold caches,
  ``snn.LEVEL_ON_DEVICE`` off against on: the four levels among everything else a first forward does.

Per row and route: host-clock time per call between two synchronisations (the work ends on the host: median, range and
the runs of ``--reps`` windows of ``--seconds``), and of one call the torch operator calls, the calls into the HIP
library, the host synchronisations and the peak of device memory above what was resident.  ``launches``: of one call of
the device route, per C entry the device time between two events, its algorithmic bytes and their fraction of the HBM
specification (8 TB/s).  ``device_wins`` / ``device_loses``: the two ranges of window times do not overlap and the device
median is the smaller / the larger."""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import measure                                                              # noqa: E402
from deepviewagg_amd import ops                                             # noqa: E402
from deepviewagg_amd.modules.SparseConv3d import ResNetDown, nn as snn      # noqa: E402

DEV = "cuda:0"
HBM_SPEC_BYTES_PER_MS = 8.0e9
WIDTHS = (16, 32, 64, 96, 128)


def surface_coords(n):
    """tools/sparse_conv_bench.py's cloud: unique voxels on the faces of a box, sorted by a coarse block key."""
    rng = np.random.default_rng(0)
    extent = int(np.sqrt(n / 4.5))
    p = rng.integers(0, extent, size=(int(n * 1.6), 3))
    face = rng.integers(0, 3, p.shape[0])
    p[np.arange(p.shape[0]), face] = rng.integers(0, 2, p.shape[0]) * (extent - 1)
    c = np.unique(p, axis=0)[:n]
    coords = torch.from_numpy(np.concatenate([c, np.zeros((c.shape[0], 1), dtype=np.int64)], 1).astype(np.int32)).to(DEV)
    key = ((coords[:, 2] // 8).long() * 4096 + (coords[:, 1] // 8).long()) * 4096 + (coords[:, 0] // 8).long()
    return coords[torch.argsort(key)].contiguous()


@contextlib.contextmanager
def level_on_device(on):
    found, snn.LEVEL_ON_DEVICE = snn.LEVEL_ON_DEVICE, on
    try:
        yield
    finally:
        snn.LEVEL_ON_DEVICE = found


def level_routes(coords, in_stride, bounds):
    """{route: callable} of one kernel_size 2 / stride 2 level on ``coords`` at ``in_stride``, each on cold caches."""
    key, out_stride = (in_stride, 2, 2, 1), 2 * in_stride
    feats = torch.empty(coords.shape[0], 0, device=DEV)

    def composition():
        x = snn.SparseVoxelTensor(feats, coords, in_stride)
        snn.Conv3d._build_composition(x, key, out_stride)
        return x, ops.voxel_parent_index(x.C, x.coord_maps[out_stride], out_stride)

    def device():
        x = snn.SparseVoxelTensor(feats, coords, in_stride)
        if in_stride > 1:
            x.coord_maps.bounds = (1, *bounds)          # read at the input tensor, as in a model
        assert snn.Conv3d._build_level(x, key, out_stride)
        return x, x.coord_maps.parents[(in_stride, out_stride)]
    return {"composition": composition, "device": device}


def encoder_routes(coords):
    torch.manual_seed(17)
    stages = torch.nn.ModuleList(ResNetDown(down_conv_nn=[WIDTHS[i], WIDTHS[i + 1]], N=1)
                                 for i in range(4)).eval().to(DEV)
    feats = torch.randn(coords.shape[0], WIDTHS[0], generator=torch.Generator().manual_seed(17)).to(DEV)

    def forward(on):
        x = snn.SparseVoxelTensor(feats, coords)        # cold caches
        with torch.no_grad(), level_on_device(on):
            for stage in stages:
                x = stage(x)
        return x, None
    return {"composition": lambda: forward(False), "device": lambda: forward(True)}


def same(a, b):
    """The two routes leave the same caches and parents (bit for bit), and the same features where there are any."""
    (xa, pa), (xb, pb) = a, b
    ok = set(xa.coord_maps) == set(xb.coord_maps) and set(xa.kernel_maps) == set(xb.kernel_maps)
    ok = ok and all(torch.equal(xa.coord_maps[s], xb.coord_maps[s]) for s in xa.coord_maps)
    ok = ok and all(torch.equal(m, w) for k in xa.kernel_maps for m, w in zip(xa.kernel_maps[k], xb.kernel_maps[k]))
    if pa is not None:
        ok = ok and torch.equal(pa, pb)
    return bool(ok and xa.F.shape == xb.F.shape)


def timed_launches(fn):
    """Per C entry of one call of ``fn``: device ms between two events, algorithmic bytes, fraction of the HBM spec."""
    found, ops.TIMER = ops.TIMER, ops.KernelTimer(only=("voxel_bounds", "voxel_level", "voxel_level_maps"))
    try:
        fn()
        agg = ops.TIMER.summary()
    finally:
        ops.TIMER = found
    return {name: {"launches": a["launches"], "ms": round(a["ms"], 4), "bytes": a["bytes"],
                   "hbm_fraction": round(a["bytes"] / max(a["ms"], 1e-6) / HBM_SPEC_BYTES_PER_MS, 4)}
            for name, a in agg.items()}


def run_row(name, routes, voxels, n_in, reps, seconds):
    equal = same(routes["composition"](), routes["device"]())
    ms, inner = measure.alternate(routes, reps, measure.host_window, warmup=2, seconds=seconds)
    row = {"row": name, "voxels": voxels, "rows_in": n_in, "same_results": equal, "inner": inner}
    for route, fn in routes.items():
        row[route] = {"ms": measure.summarise(ms[route], 4), "runs": [round(t, 4) for t in ms[route]],
                      **measure.profile_once(fn)}
    row["launches"] = timed_launches(routes["device"])
    c, d = row["composition"]["ms"], row["device"]["ms"]
    apart = not measure.ranges_overlap((c["min"], c["max"]), (d["min"], d["max"]))
    row["speedup"] = round(c["median"] / d["median"], 3)
    row["device_wins"] = bool(apart and d["median"] < c["median"])
    row["device_loses"] = bool(apart and d["median"] > c["median"])
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.1, help="length of one timed window")
    ap.add_argument("--voxels", type=int, nargs="+", default=[300000, 1 << 20])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_level_bench.json"))
    args = ap.parse_args(argv)
    rows = []
    for n in args.voxels:
        coords = surface_coords(n)
        bounds = ops.voxel_bounds(coords)
        level, in_stride = coords, 1
        for _ in range(3):
            rows.append(run_row(f"level_{in_stride}_{2 * in_stride}", level_routes(level, in_stride, bounds),
                                int(coords.shape[0]), int(level.shape[0]), args.reps, args.seconds))
            level, in_stride = snn.downsample_coords(level, 2 * in_stride), 2 * in_stride
        rows.append(run_row("encoder_first_forward", encoder_routes(coords), int(coords.shape[0]), int(coords.shape[0]),
                            args.reps, args.seconds))
        for r in rows[-4:]:
            print(f"{r['voxels']} {r['row']}: composition {r['composition']['ms']['median']} ms, device "
                  f"{r['device']['ms']['median']} ms, same {r['same_results']}", file=sys.stderr)
        torch.cuda.empty_cache()
    measure.emit(measure.header("voxel_level_bench", reps=args.reps, window_seconds=args.seconds,
                                hbm_spec_tb_per_s=8.0, rows=rows), args.out)


if __name__ == "__main__":
    main()
