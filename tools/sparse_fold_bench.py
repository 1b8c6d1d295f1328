"""Sparse-convolution stages at inference: the folded copy (``fold_for_inference``: BatchNorm, ReLU and the residual
sum in the epilogue of the convolution, weights packed once) against the unfolded modules in eval mode, on the same
device in the same process, the two alternating.

    python tools/sparse_fold_bench.py [--reps 7] [--seconds 0.2] [--voxels 300000 1048576] [--out profiles/sparse_fold_bench.json]

Voxels: the surface cloud of tools/sparse_conv_bench.py (the faces of a room-sized box, in the order a voxelised scan
arrives), at 3 * 10^5 and 2^20 voxels, fp32 and bf16 features (bf16: both routes under autocast(bfloat16)).  Arms per
shape: ``ResBlock`` 64 -> 64, ``ResBlock`` 64 -> 128 (with the 1x1x1 shortcut), and a ``ResNetDown(64 -> 128, N=2)`` ->
``ResNetUp(128 + 64 -> 64, N=1)`` pair.  Both routes run under ``torch.no_grad()`` with their kernel maps cached on the
input tensor (one untimed call builds them) and, for the folded route, the packed weights cached on the modules.

Per arm and route: device-event time per call over windows of ``--seconds`` (median and spread of ``--reps`` windows),
and of one call the calls into the HIP library, the torch operator calls on device tensors, the host synchronisations
and the peak of device memory above what was resident, and ``kernels``, the device kernels the torch profiler counts
in one call (None where it has no tracer).  ``folded_wins``: the two ranges of window times do not overlap
and the folded median is the smaller.  ``max_diff_over_scale``: the largest difference of the two outputs over the
largest unfolded value (the folded route rounds W * g once, the unfolded one the convolution and the BatchNorm apart).
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import measure                                                                          # noqa: E402
from deepviewagg_amd.modules.SparseConv3d import (ResBlock, ResNetDown, ResNetUp,       # noqa: E402
                                                  fold_for_inference, nn as snn)

DEV = "cuda:0"
C = 64


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


def randomise_norms(module, gen):
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.3)
    return module


class Pair(torch.nn.Module):
    """An encoder stage and the decoder stage that takes its input as the skip."""

    def __init__(self):
        super().__init__()
        self.down = ResNetDown(down_conv_nn=[C, 2 * C], N=2)
        self.up = ResNetUp(up_conv_nn=[2 * C, C, C], N=1)

    def forward(self, x):
        return self.up(self.down(x), x)


def arms():
    return {"resblock_64_64": lambda: ResBlock(C, C, snn.Conv3d),
            "resblock_64_128_shortcut": lambda: ResBlock(C, 2 * C, snn.Conv3d),
            "resnet_down_up_pair": Pair}


def run_row(arm, make, coords, dtype, reps, seconds):
    gen = torch.Generator().manual_seed(17)
    torch.manual_seed(17)
    plain = randomise_norms(make(), gen).eval().to(DEV)
    folded = fold_for_inference(plain)
    feats = torch.randn(coords.shape[0], C, generator=gen).to(DEV).to(dtype)
    x = snn.SparseVoxelTensor(feats, coords)
    amp = torch.autocast("cuda", dtype=torch.bfloat16) if dtype == torch.bfloat16 else contextlib.nullcontext()

    def call(module):
        with torch.no_grad(), amp:
            return module(x)

    routes = {"folded": lambda: call(folded), "unfolded": lambda: call(plain)}
    out_f, out_u = routes["folded"]().F.float(), routes["unfolded"]().F.float()     # builds the maps and the packs
    diff = float((out_f - out_u).abs().max() / out_u.abs().max())
    del out_f, out_u
    ms, inner = measure.alternate(routes, reps, measure.event_window, warmup=1, seconds=seconds)
    row = {"arm": arm, "voxels": int(coords.shape[0]), "dtype": str(dtype).split(".")[-1],
           "max_diff_over_scale": diff, "inner": inner}
    for name, fn in routes.items():
        s = measure.summarise(ms[name], 4)
        row[name] = {"ms": s, "runs": [round(t, 4) for t in ms[name]], **measure.profile_once(fn),
                     "kernels": measure.profiler_kernel_count(fn)}
    f, u = row["folded"]["ms"], row["unfolded"]["ms"]
    row["speedup"] = round(u["median"] / f["median"], 3)
    row["folded_wins"] = bool(f["median"] < u["median"]
                              and not measure.ranges_overlap((f["min"], f["max"]), (u["min"], u["max"])))
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.2, help="length of one timed window")
    ap.add_argument("--voxels", type=int, nargs="+", default=[300000, 1 << 20])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_fold_bench.json"))
    args = ap.parse_args(argv)
    rows = []
    for n in args.voxels:
        coords = surface_coords(n)
        for dtype in (torch.float32, torch.bfloat16):
            for arm, make in arms().items():
                rows.append(run_row(arm, make, coords, dtype, args.reps, args.seconds))
                r = rows[-1]
                print(f"{r['voxels']} {r['dtype']} {arm}: folded {r['folded']['ms']['median']} ms, unfolded "
                      f"{r['unfolded']['ms']['median']} ms", file=sys.stderr)
                torch.cuda.empty_cache()
    measure.emit(measure.header("sparse_fold_bench", reps=args.reps, window_seconds=args.seconds, channels=C,
                                rows=rows), args.out)


if __name__ == "__main__":
    main()
