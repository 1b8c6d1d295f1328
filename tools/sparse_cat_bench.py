"""Convolving a channel concatenation of voxel features: the lazy route (``snn.cat(..., lazy=True)`` / ``snn.LAZY_CAT``:
the parts go to the convolution kernel as they are, ``ops.sparse_conv`` on a list) against the materialised route of the
default (the concatenated tensor is written, then cast and padded by the convolution), on the same device in the same
process, the two alternating.

    python tools/sparse_cat_bench.py [--reps 7] [--seconds 0.2] [--voxels 300000 1048576] [--out profiles/sparse_cat_bench.json]

Voxels: the surface cloud of tools/sparse_conv_bench.py at 3 * 10^5 and 2^20 voxels, fp32 and autocast(bfloat16).  Under
autocast the wide part of the fusion (the pooled image features) is bf16, as the pooling leaves it, and the 3D features are
fp32.  Arms:

* ``fusion_4_512_128_fwd`` / ``_fwd_bwd``: the fusion layer of Res16UNet34-L4-early, parts (4, 512) -> 128, K = 27; the
  materialised route is ``BimodalFusion('concatenation')`` followed by ``Conv3d``;
* ``decoder_join_resblock``: parts (128, 64) into ``ResBlock`` 192 -> 96 with its ``downsample``, training mode, forward
  and backward;
* ``decoder_join_folded``: the same block folded for inference (``fold_for_inference``), no grad;
* ``resnet_down_up_pair``: the ``ResNetDown -> ResNetUp`` pair of tools/sparse_fold_bench.py, eval mode, no grad.

Per arm and route: device-event time per call over windows of ``--seconds`` (median and spread of ``--reps`` windows), and
of one call the calls into the HIP library, the torch operator calls, the host synchronisations, the peak of device memory
above what was resident and ``kernels``, the device kernels the torch profiler counts.  ``lazy_wins`` / ``lazy_loses``: the
two ranges of window times do not overlap and the lazy median is the smaller / the larger.
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
from deepviewagg_amd.modules.multimodal.fusion import BimodalFusion                    # noqa: E402
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


@contextlib.contextmanager
def lazy_cat(on):
    found = snn.LAZY_CAT
    snn.LAZY_CAT = on
    try:
        yield
    finally:
        snn.LAZY_CAT = found


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
    """An encoder stage and the decoder stage that takes its input as the skip (``ResNetUp`` calls ``snn.cat``)."""

    def __init__(self):
        super().__init__()
        self.down = ResNetDown(down_conv_nn=[C, 2 * C], N=2)
        self.up = ResNetUp(up_conv_nn=[2 * C, C, C], N=1)

    def forward(self, x):
        return self.up(self.down(x), x)


def _feats(n, widths, dtypes, gen, grad):
    return [torch.randn(n, w, generator=gen).to(DEV).to(dt).requires_grad_(grad) for w, dt in zip(widths, dtypes)]


def fusion_arm(backward):
    """(4, 512) -> 128: the 3D features stay fp32, the pooled features come in the compute dtype."""
    def make(coords, dtype, gen):
        n = coords.shape[0]
        conv = snn.Conv3d(516, 128, kernel_size=3).to(DEV)
        fusion = BimodalFusion("concatenation")
        x3d, xmod = _feats(n, (4, 512), (torch.float32, dtype), gen, backward)
        base = snn.SparseVoxelTensor(x3d, coords)
        g = torch.randn(n, 128, generator=gen).to(DEV).to(dtype)

        def route(lazy):
            with torch.set_grad_enabled(backward):
                if lazy:
                    x = snn.LazyCatTensor((x3d, xmod), base.C, base.s, base.coord_maps, base.kernel_maps)
                else:
                    x = base.like(fusion(x3d, xmod))
                out = conv(x).F
                if backward:
                    out.backward(g)
                    for t in (x3d, xmod, conv.kernel):
                        t.grad = None
            return out.detach()
        return route
    return make


def resblock_arm(folded):
    """(128, 64) -> ResBlock 192 -> 96 with its downsample: training forward + backward, or folded for inference."""
    def make(coords, dtype, gen):
        n = coords.shape[0]
        block = randomise_norms(ResBlock(192, 96, snn.Conv3d), gen).to(DEV)
        block = fold_for_inference(block.eval()) if folded else block.train()
        a, b = _feats(n, (128, 64), (dtype, dtype), gen, not folded)
        ta = snn.SparseVoxelTensor(a, coords)
        tb = ta.like(b)
        g = torch.randn(n, 96, generator=gen).to(DEV).to(dtype)

        def route(lazy):
            with torch.set_grad_enabled(not folded):
                out = block(snn.cat(ta, tb, lazy=lazy)).F
                if not folded:
                    out.backward(g)
                    for t in [a, b] + list(block.parameters()):
                        t.grad = None
            return out.detach()
        return route
    return make


def pair_arm(coords, dtype, gen):
    pair = randomise_norms(Pair(), gen).eval().to(DEV)
    x = snn.SparseVoxelTensor(torch.randn(coords.shape[0], C, generator=gen).to(DEV).to(dtype), coords)

    def route(lazy):
        with torch.no_grad(), lazy_cat(lazy):
            return pair(x).F
    return route


def arms():
    return {"fusion_4_512_128_fwd": fusion_arm(False), "fusion_4_512_128_fwd_bwd": fusion_arm(True),
            "decoder_join_resblock": resblock_arm(False), "decoder_join_folded": resblock_arm(True),
            "resnet_down_up_pair": pair_arm}


def run_row(arm, make, coords, dtype, reps, seconds):
    gen = torch.Generator().manual_seed(17)
    torch.manual_seed(17)
    route = make(coords, dtype, gen)
    amp = torch.autocast("cuda", dtype=torch.bfloat16) if dtype == torch.bfloat16 else contextlib.nullcontext()

    def call(lazy):
        with amp:
            return route(lazy)

    routes = {"lazy": lambda: call(True), "materialised": lambda: call(False)}
    out_l, out_m = routes["lazy"]().float(), routes["materialised"]().float()          # builds the maps and the packs
    diff = float((out_l - out_m).abs().max() / out_m.abs().max())
    del out_l, out_m
    ms, inner = measure.alternate(routes, reps, measure.event_window, warmup=1, seconds=seconds)
    row = {"arm": arm, "voxels": int(coords.shape[0]), "dtype": str(dtype).split(".")[-1],
           "max_diff_over_scale": diff, "inner": inner}
    for name, fn in routes.items():
        s = measure.summarise(ms[name], 4)
        row[name] = {"ms": s, "runs": [round(t, 4) for t in ms[name]], **measure.profile_once(fn),
                     "kernels": measure.profiler_kernel_count(fn)}
    lz, mt = row["lazy"]["ms"], row["materialised"]["ms"]
    apart = not measure.ranges_overlap((lz["min"], lz["max"]), (mt["min"], mt["max"]))
    row["speedup"] = round(mt["median"] / lz["median"], 3)
    row["lazy_wins"] = bool(apart and lz["median"] < mt["median"])
    row["lazy_loses"] = bool(apart and lz["median"] > mt["median"])
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.2, help="length of one timed window")
    ap.add_argument("--voxels", type=int, nargs="+", default=[300000, 1 << 20])
    ap.add_argument("--arms", nargs="+", default=None, help="a subset of the arms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_cat_bench.json"))
    args = ap.parse_args(argv)
    rows = []
    for n in args.voxels:
        coords = surface_coords(n)
        for dtype in (torch.float32, torch.bfloat16):
            for arm, make in arms().items():
                if args.arms and arm not in args.arms:
                    continue
                rows.append(run_row(arm, make, coords, dtype, args.reps, args.seconds))
                r = rows[-1]
                print(f"{r['voxels']} {r['dtype']} {arm}: lazy {r['lazy']['ms']['median']} ms, materialised "
                      f"{r['materialised']['ms']['median']} ms", file=sys.stderr)
                torch.cuda.empty_cache()
    measure.emit(measure.header("sparse_cat_bench", reps=args.reps, window_seconds=args.seconds, rows=rows), args.out)


if __name__ == "__main__":
    main()
