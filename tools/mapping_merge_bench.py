"""Mapping merge after a strided 3D stage: the device op (ops.merge_mapping behind ImageMapping.select_points(mode=
'merge')) against the kept torch composition, on the same device in the same process.

    python tools/mapping_merge_bench.py [--reps 5] [--out profiles/mapping_merge_bench.json]

Two shapes: the headline scene (2^20 points, 32 exact views each, parents = stride-2 floor of integer voxel
coordinates) and a reference-sized batch (3 * 10^5 points, the view-count law of bench.py's workload S2: k = min(32,
1 + Geom(0.2)), 10 % of the points unseen).  The two routes alternate; each is timed `reps` times after one warm-up,
wall clock around the whole call (the host readbacks are part of what a training step pays).  Reported: the medians,
the spread (max - min) of the repetitions, the HIP-event times of the two entries, and the achieved bytes/s of the
device op on the algorithmic count  read N*8 + V*16 + P*4 + V*F*4, write (M+1)*8 + V'*16 + P'*4 + V'*F*4.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import measure                                                           # noqa: E402
from deepviewagg_amd import ops                                          # noqa: E402
from deepviewagg_amd.core.multimodal.csr import CSRData                  # noqa: E402
from deepviewagg_amd.core.multimodal.image import ImageMapping           # noqa: E402

DEV = "cuda:0"
F = 8


def parents(n, side, gen):
    """n distinct integer voxel coordinates in a side^3 cube -> index of their stride-2 parent voxel."""
    lin = torch.randperm(side ** 3, generator=gen, device=DEV)[:n]
    c = torch.stack([lin % side, (lin // side) % side, lin // (side * side)], 1) // 2
    key = (c[:, 2] * side + c[:, 1]) * side + c[:, 0]
    return torch.unique(key, return_inverse=True)[1]


def exact_mapping(sizes, n_images, gen):
    """Exact mapping (one pixel per view): point i sees sizes[i] distinct images, ascending."""
    n = sizes.shape[0]
    order = torch.rand(n, n_images, generator=gen, device=DEV).argsort(dim=1)
    keep = torch.arange(n_images, device=DEV).view(1, -1) < sizes.view(-1, 1)
    imgs = torch.where(keep, order, torch.full_like(order, n_images)).sort(dim=1).values
    images = imgs[imgs < n_images].contiguous()
    pointers = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
    v = images.shape[0]
    pixels = torch.stack([torch.randint(0, 1024, (v,), generator=gen, device=DEV),
                          torch.randint(0, 512, (v,), generator=gen, device=DEV)], 1).to(torch.int16)
    feats = torch.randn(v, F, generator=gen, device=DEV)
    nested = CSRData(torch.arange(v + 1, device=DEV), pixels, dense=False)
    return ImageMapping(pointers, images, nested, feats, dense=False, is_index_value=[True, False, False])


def scene(name, gen):
    if name == "headline":
        n = 1 << 20
        sizes = torch.full((n,), 32, dtype=torch.long, device=DEV)
        return exact_mapping(sizes, 32, gen), parents(n, 128, gen)
    n = 300000
    k = torch.empty(n, device=DEV).geometric_(0.2, generator=gen).long()     # trials to the first success = 1 + Geom
    sizes = torch.clamp(k, max=32)
    sizes[torch.rand(n, generator=gen, device=DEV) < 0.1] = 0
    return exact_mapping(sizes, 32, gen), parents(n, 100, gen)


def run_shape(name, reps):
    gen = torch.Generator(device=DEV).manual_seed(1234)
    m, idx = scene(name, gen)

    def run(on_device):
        ImageMapping.MERGE_ON_DEVICE = on_device
        try:
            return m.select_points(idx, mode='merge')
        finally:
            ImageMapping.MERGE_ON_DEVICE = True

    out = run(True)
    ref = run(False)                                                     # warm-up of both routes, and a parity check
    same = all(torch.equal(a, b) for a, b in ((out.pointers, ref.pointers), (out.images, ref.images),
                                              (out.values[1].pointers, ref.values[1].pointers),
                                              (out.pixels, ref.pixels)))
    err = float((out.features - ref.features).abs().max())
    ms, _ = measure.alternate({True: lambda: run(True), False: lambda: run(False)}, reps, measure.host_window,
                              warmup=0)                                  # both routes are warm from the parity check
    ops.TIMER = ops.KernelTimer(only=("mapping_merge_count", "mapping_merge_fill"))
    run(True)
    kernels = {k: round(v["ms"], 4) for k, v in ops.TIMER.summary().items()}
    ops.TIMER = None
    n, v, p = m.num_groups, m.num_views, m.num_atoms
    mm, v2, p2 = out.num_groups, out.num_views, out.num_atoms
    nbytes = n * 8 + v * 16 + p * 4 + v * F * 4 + (mm + 1) * 8 + v2 * 16 + p2 * 4 + v2 * F * 4
    dev_ms, comp_ms = (measure.summarise(ms[r], 4) for r in (True, False))
    runs = lambda x: [round(t, 4) for t in x]
    return {
        "shape": name, "points": n, "views": v, "atoms": p, "voxels": mm, "views_out": v2, "atoms_out": p2, "F": F,
        "indices_equal": bool(same), "features_max_abs_diff": err,
        "device_op_ms": {"median": dev_ms["median"], "spread": dev_ms["spread"], "runs": runs(ms[True]),
                         "entries_event_ms": kernels},
        "composition_ms": {"median": comp_ms["median"], "spread": comp_ms["spread"], "runs": runs(ms[False])},
        "algorithmic_bytes": nbytes, "device_op_GBps": round(nbytes / dev_ms["median"] / 1e6, 2),
        "speedup": round(comp_ms["median"] / dev_ms["median"], 2),
        "device_op_wins": bool(comp_ms["median"] - dev_ms["median"] > max(dev_ms["spread"], comp_ms["spread"])),
    }


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapping_merge_bench.json"))
    args = ap.parse_args(argv)
    measure.emit(measure.header("mapping_merge_bench", tile_atoms=ops.MERGE_TILE_ATOMS, reps=args.reps,
                                shapes=[run_shape(s, args.reps) for s in ("headline", "batch")]), args.out)


if __name__ == "__main__":
    main()
