#!/usr/bin/env python
"""Time the online image chain of one sample on the device, deferred against eager, at the image sizes of the shipped
configs, images and mappings resident on the device:

  s3dis_32 / s3dis_64   32 / 64 seen equirectangular images of 512 x 1024: SelectMappingFromPointId -> CenterRoll ->
                        PickImagesFromMappingArea -> CropImageGroups(padding 8, min_size 64) ->
                        PickImagesFromMemoryCredit(4 x 1024 x 512, k_coverage 2) -> JitterMappingFeatures -> the train tail
  kitti360_32           32 images of 1408 x 376, the same chain without CenterRoll
  crop_group_16         16 images of 512 x 1024, CropImageGroups -> the train tail alone

  eager     fuse_image_tail(chain): every selection, the roll and the crop copy or gather the uint8 images, then
            FusedImageTail reads the crops (the chain as it stood before the deferral)
  deferred  defer_image_windows(chain): DeferImages in front; indices and offsets move, FusedImageTail reads every
            surviving window from the source images through ops.image_window

The mappings are synthetic: every image sees the points through one box of random size and place, so that the chain
drops images, rolls and crops to several sizes as it does on the datasets.  Before timing, the two variants are checked
equal bit for bit (x, mapped pixels, generator state) from the same seeds.

Also ``ops.image_window`` alone against ``update_rollings`` + ``update_cropping`` + ``ops.image_tail`` on the already
selected images (window_256: 16 windows of 256 x 256 out of 512 x 1024; window_full: 8 rolled whole images).

The chains synchronise with the host (``.tolist()``, ``np.random.choice``), so a chain is timed with the host clock
around ``inner`` applications that end in a device synchronise; the two kernels-only cases use device events.  Every
variant is warmed up, the variants alternate inside every repetition, and the figure is the median over --reps windows of
about --window seconds, per application.  Per variant: ``torch_ops`` = aten operator calls on device tensors (each at
least one kernel or copy), ``dva_launches`` = calls into the HIP library, ``peak_bytes`` = the peak of allocated device
memory above what is resident before the chain starts.  ``bytes`` are the algorithmic bytes of the result: per surviving
window pixel 3 read, 3 more for the gray sums of contrast, 12 written; ``share_of_8tb_s`` = bytes / time over the
8 TB/s HBM peak -- the rate at which a variant delivers the result, not the traffic it causes.
One JSON line on stdout; --out writes it (profiles/image_window_bench.json).

Usage:  python tools/image_window_bench.py [--reps 5] [--window 0.25] [--out FILE]
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
from bench_scenes import CASES, JITTER, make_chain, make_scene, run_chain, seed_all  # noqa: E402

HBM_PEAK = 8.0e12


def run_case(name, B, H, W, kind, reps, seconds, gen):
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    dev = torch.device("cuda", 0)
    images, keep = make_scene(B, H, W, gen, dev)
    chain = make_chain(kind, H, W)
    chains = {"eager": T.fuse_image_tail(chain), "deferred": T.defer_image_windows(chain)}
    variants = {k: (lambda v=v: run_chain(v, images, keep)) for k, v in chains.items()}
    # equal results from equal seeds, and what one application launches and allocates
    outs, extra, after = {}, {}, {}
    for key, fn in variants.items():
        fn()
        seed_all(1)
        extra[key] = counters(lambda: outs.update({key: fn()}))
        after[key] = (torch.rand(1), np.random.rand())
    a, b = list(outs["eager"]), list(outs["deferred"])
    assert len(a) == len(b) and after["eager"] == after["deferred"], f"{name}: the variants drew differently"
    for u, v in zip(a, b):
        assert torch.equal(u.x, v.x) and torch.equal(u.mappings.pixels, v.mappings.pixels), f"{name}: variants differ"
    windows = [[im.num_views, 3, int(im.x.shape[2]), int(im.x.shape[3])] for im in a]
    nbytes = sum(n * h * w for n, _, h, w in windows) * (3 + 3 + 12)
    del outs, a, b
    rows = measure_variants(variants, measure.host_window, reps, seconds, nbytes, extra)
    rows["deferred"]["speedup_vs_eager"] = round(rows["eager"]["ms"] / rows["deferred"]["ms"], 2)
    return {"case": name, "source": [B, 3, H, W], "chain": [type(tr).__name__ for tr in chain], "windows": windows,
            "checks": {"deferred_equals_eager": True}, "variants": rows}


def counters(fn):
    profile = measure.profile_once(fn)
    return {k: profile[k] for k in ("torch_ops", "dva_launches", "peak_bytes")}


def measure_variants(variants, window, reps, seconds, nbytes, extra):
    ms, inner = measure.alternate(variants, reps, window, warmup=3, seconds=seconds, probe_inner=3,
                                  before=lambda key, rep: seed_all(2 if rep is None else 3 + rep))
    rows = {}
    for key in variants:
        s = measure.summarise(ms[key], 4)
        med = s["median"]
        rows[key] = {"ms": med, "min_ms": s["min"], "max_ms": s["max"],
                     "applications_per_window": inner[key], "bytes": nbytes,
                     "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 4),
                     "share_of_8tb_s": round(nbytes / (med * 1e-3) / HBM_PEAK, 4), **extra.get(key, {})}
    return rows


def run_kernel_case(name, B, H, W, Wc, Hc, reps, seconds, gen):
    """ops.image_window alone against update_rollings + update_cropping + ops.image_tail on the selected images."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.core.multimodal.image import SameSettingImageData
    dev = torch.device("cuda", 0)
    src = torch.randint(0, 256, (2 * B, 3, H, W), dtype=torch.uint8, generator=gen).to(dev)
    index = torch.randperm(2 * B, generator=gen)[:B].to(dev)
    rolls = torch.randint(0, W, (B,), generator=gen).to(dev)
    offsets = torch.stack([torch.randint(0, W - Wc + 1, (B,), generator=gen),
                           torch.randint(0, H - Hc + 1, (B,), generator=gen)], 1).to(dev)
    picked = src[index]
    jitter = [("saturation", 1.3), ("contrast", 0.7), ("brightness", 1.1)]
    kw = dict(jitter=jitter, flip=True, to_float=True, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])

    def windowed():
        return ops.image_window(src, index, rolls, offsets, (Wc, Hc), **kw)

    def eager():
        im = SameSettingImageData(pos=torch.zeros(B, 3, device=dev), ref_size=(W, H), proj_upscale=1, x=picked)
        im.update_rollings(rolls)
        if (Wc, Hc) != (W, H):
            im.update_cropping((Wc, Hc), offsets)
        return ops.image_tail(im.x, **kw)

    variants = {"eager": eager, "window": windowed}
    assert torch.equal(eager(), windowed()), f"{name}: ops.image_window and the eager composition differ"
    extra = {key: counters(fn) for key, fn in variants.items()}
    nbytes = B * Hc * Wc * (3 + 3 + 12)
    rows = measure_variants(variants, measure.event_window, reps, seconds, nbytes, extra)
    rows["window"]["speedup_vs_eager"] = round(rows["eager"]["ms"] / rows["window"]["ms"], 2)
    return {"case": name, "source": [2 * B, 3, H, W], "windows": [[B, 3, Hc, Wc]],
            "checks": {"window_equals_eager": True}, "variants": rows}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    gen = torch.Generator().manual_seed(0)
    result = measure.header(
        "image_window_bench", reps=args.reps, window_s=args.window, jitter=list(JITTER),
        bytes_per_pixel={"read": 3, "read_contrast": 3, "written": 12},
        chains=[run_case(*case, args.reps, args.window, gen) for case in CASES],
        kernels=[run_kernel_case("window_256", 16, 512, 1024, 256, 256, args.reps, args.window, gen),
                 run_kernel_case("window_full", 8, 512, 1024, 1024, 512, args.reps, args.window, gen)])
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
