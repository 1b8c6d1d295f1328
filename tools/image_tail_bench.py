#!/usr/bin/env python
"""Time the image tail of the multimodal transform chains on the device at the image sizes of the shipped configs:

  uint8 [32, 3, 512, 1024] (S3DIS equirectangular at ref_size), [16, 3, 256, 512] (a crop group), [64, 3, 240, 320]
  (ScanNet) and [32, 3, 376, 1408] (KITTI-360), images resident on the device.

Per shape, the train tail ColorJitter(0.6, 0.6, 0.7) -> RandomHorizontalFlip(p = 1) -> ToFloatImage -> Normalize and the
eval tail ToFloatImage -> Normalize, three ways each:

  fused   FusedImageTail (one pass of csrc/image_tail.hip, two kernels with contrast)
  eager   this package's chain: the ColorJitter and Normalize classes plus the existing flip and ToFloatImage
  torch   the plain torch composition of the same formulas on the device (tests/image_tail_ref.py::torch_tail)

One process; every variant of a shape is warmed up, then the variants alternate inside every repetition; a window is
``inner`` back-to-back applications between two device events, ``inner`` chosen so that a window lasts about
--window seconds; the figure is the median over --reps windows, per application.  Before timing, fused and eager are
checked equal bit for bit from the same generator state; how the torch composition compares is recorded (the device's
torch division by a scalar and its float32 mean need not round as the contract does).

``bytes`` are the algorithmic bytes of the tail: 3 read per pixel (+3 with contrast, the gray-sum pass) and 12 written;
``tb_per_s`` = bytes / time and ``share_of_8tb_s`` its share of the 8 TB/s HBM peak -- for the eager and torch
variants that is the rate at which they deliver the same result, not the traffic they cause.
One JSON line on stdout; --out writes it (profiles/image_tail_bench.json).

Usage:  python tools/image_tail_bench.py [--reps 5] [--window 0.25] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import measure  # noqa: E402

SHAPES = (("s3dis_equirect", (32, 3, 512, 1024)), ("crop_group", (16, 3, 256, 512)), ("scannet", (64, 3, 240, 320)),
          ("kitti360", (32, 3, 376, 1408)))
JITTER = (0.6, 0.6, 0.7)
HBM_PEAK = 8.0e12


def make_setting(x, gen):
    """A SameSettingImageData around the images x with a small random mapping (the flip mirrors its pixel columns)."""
    from deepviewagg_amd.core.multimodal.image import ImageMapping, SameSettingImageData
    B, _, H, W = x.shape
    n, n_points = 4096, 1024
    pts, imgs = torch.randint(0, n_points, (n,), generator=gen), torch.randint(0, B, (n,), generator=gen)
    pix = torch.stack([torch.randint(0, W, (n,), generator=gen), torch.randint(0, H, (n,), generator=gen)], 1).short()
    dev = x.device
    m = ImageMapping.from_dense(pts.to(dev), imgs.to(dev), pix.to(dev), torch.rand(n, 2, generator=gen).to(dev),
                                num_points=n_points)
    return SameSettingImageData(path=np.array([f"img_{i}" for i in range(B)]), pos=torch.zeros(B, 3, device=dev),
                                opk=torch.zeros(B, 3, device=dev), ref_size=(W, H), proj_upscale=1, mappings=m, x=x)


def run_shape(name, shape, reps, seconds, gen):
    import image_tail_ref as R
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    dev = torch.device("cuda", 0)
    x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=gen).to(dev)
    images = make_setting(x, gen)
    cj, flip, tf, nm = T.ColorJitter(*JITTER), T.RandomHorizontalFlip(p=1.0), T.ToFloatImage(), T.Normalize()
    chains = {"train": [cj, flip, tf, nm], "eval": [tf, nm]}

    def through(transforms):
        def fn():
            images.x = x
            data, out = None, images
            for tr in transforms:
                data, out = tr(data, out)
            return out.x
        return fn

    def plain(train):
        def fn():
            return R.torch_tail(x, jitter=cj.draw() if train else (), flip=train, to_float=True, mean=nm.mean,
                                std=nm.std)
        return fn

    variants, checks = {}, {}
    for tag, chain in chains.items():
        variants[f"fused_{tag}"] = through(T.fuse_image_tail(chain))
        variants[f"eager_{tag}"] = through(chain)
        variants[f"torch_{tag}"] = plain(tag == "train")
        outs = {}
        for kind in ("fused", "eager", "torch"):
            torch.manual_seed(1)
            outs[kind] = variants[f"{kind}_{tag}"]()
        assert torch.equal(outs["fused"], outs["eager"]), f"{name} {tag}: fused and eager differ"
        checks[tag] = {"fused_equals_eager": True, "torch_equals_fused": bool(torch.equal(outs["torch"], outs["fused"])),
                       "torch_max_abs_diff": float((outs["torch"] - outs["fused"]).abs().max())}
        del outs
    # warm-up of every variant, and the number of applications that fills a window
    ms, inner = measure.alternate(variants, reps, measure.event_window, warmup=3, seconds=seconds, probe_inner=3)
    pixels = shape[0] * shape[2] * shape[3]
    rows = {}
    for key in variants:
        nbytes = pixels * (3 + (3 if key.endswith("train") else 0) + 12)
        t = measure.summarise(ms[key], 4)
        med = t["median"]
        rows[key] = {"ms": med, "min_ms": t["min"], "max_ms": t["max"],
                     "applications_per_window": inner[key], "bytes": nbytes,
                     "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3),
                     "share_of_8tb_s": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}
    for tag in chains:
        rows[f"fused_{tag}"]["speedup_vs_eager"] = round(rows[f"eager_{tag}"]["ms"] / rows[f"fused_{tag}"]["ms"], 2)
        rows[f"fused_{tag}"]["speedup_vs_torch"] = round(rows[f"torch_{tag}"]["ms"] / rows[f"fused_{tag}"]["ms"], 2)
    return {"shape": name, "x": list(shape), "checks": checks, "variants": rows}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    gen = torch.Generator().manual_seed(0)
    result = measure.header("image_tail_bench", reps=args.reps, window_s=args.window, jitter=list(JITTER), flip_p=1.0,
                            bytes_per_pixel={"read": 3, "read_contrast": 3, "written": 12},
                            shapes=[run_shape(name, shape, args.reps, args.window, gen) for name, shape in SHAPES])
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
