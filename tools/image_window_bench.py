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
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

JITTER = (0.6, 0.6, 0.7)
HBM_PEAK = 8.0e12
N_POINTS = 20000
CASES = (("s3dis_32", 32, 512, 1024, "s3dis"), ("s3dis_64", 64, 512, 1024, "s3dis"),
         ("kitti360_32", 32, 376, 1408, "kitti360"), ("crop_group_16", 16, 512, 1024, "crop"))


class Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class CountDeviceOps(TorchDispatchMode):
    """Counts the aten operator calls that take or return a device tensor."""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        flat = list(args) + list((kwargs or {}).values()) + (list(out) if isinstance(out, (tuple, list)) else [out])
        if any(torch.is_tensor(a) and a.is_cuda for a in flat):
            self.n += 1
        return out


class CountLaunches:
    """ops.TIMER stand-in: counts the calls into the HIP library, no events."""

    def __init__(self):
        self.n = 0

    def launch(self, name, nbytes):
        from deepviewagg_amd import ops
        self.n += 1
        return ops._NO_TIMER


def make_scene(B, H, W, gen, dev):
    """B uint8 images of W x H and a mapping in which image i sees random points through one random box."""
    from deepviewagg_amd.core.multimodal.image import ImageMapping, SameSettingImageData
    x = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=gen).to(dev)
    pts, imgs, pix = [], [], []
    for i in range(B):
        bw, bh = int(torch.randint(40, W // 2, (1,), generator=gen)), int(torch.randint(40, H // 2, (1,), generator=gen))
        x0, y0 = int(torch.randint(0, W - bw, (1,), generator=gen)), int(torch.randint(0, H - bh, (1,), generator=gen))
        n = int(torch.randint(bw * bh // 2, bw * bh, (1,), generator=gen))
        pts.append(torch.randint(0, N_POINTS, (n,), generator=gen))
        imgs.append(torch.full((n,), i))
        pix.append(torch.stack([x0 + torch.randint(0, bw, (n,), generator=gen),
                                y0 + torch.randint(0, bh, (n,), generator=gen)], 1).short())
    pts, imgs, pix = torch.cat(pts), torch.cat(imgs), torch.cat(pix)
    m = ImageMapping.from_dense(pts.to(dev), imgs.to(dev), pix.to(dev), torch.rand(pts.shape[0], 2, generator=gen).to(dev),
                                num_points=N_POINTS)
    images = SameSettingImageData(path=np.array([f"img_{i}" for i in range(B)]), pos=torch.zeros(B, 3, device=dev),
                                  opk=torch.zeros(B, 3, device=dev), ref_size=(W, H), proj_upscale=1, mappings=m, x=x)
    keep = torch.randperm(N_POINTS, generator=gen)[:N_POINTS // 2].to(dev)
    return images, keep


def make_chain(kind, H, W):
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    tail = [T.ColorJitter(*JITTER), T.RandomHorizontalFlip(), T.ToFloatImage(), T.Normalize()]
    if kind == "crop":
        return [T.CropImageGroups(padding=8, min_size=64)] + tail
    head = [T.SelectMappingFromPointId()] + ([T.CenterRoll()] if kind == "s3dis" else [])
    return head + [T.PickImagesFromMappingArea(use_bbox=False), T.CropImageGroups(padding=8, min_size=64),
                   T.PickImagesFromMemoryCredit(img_size=[W, H], n_img=4, k_coverage=2),
                   T.JitterMappingFeatures(sigma=0.02, clip=0.03)] + tail


def seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def run_case(name, B, H, W, kind, reps, seconds, gen):
    from deepviewagg_amd import ops
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    dev = torch.device("cuda", 0)
    images, keep = make_scene(B, H, W, gen, dev)
    chain = make_chain(kind, H, W)
    chains = {"eager": T.fuse_image_tail(chain), "deferred": T.defer_image_windows(chain)}

    def through(transforms):
        def fn():
            # the chain's first transform builds new settings and leaves `images` as it is; `data` is rewritten
            data = Data(pos=torch.zeros(keep.shape[0], 3, device=dev), mapping_index=keep, num_nodes=keep.shape[0])
            out = images
            for tr in transforms:
                data, out = tr(data, out)
            return out
        return fn

    variants = {k: through(v) for k, v in chains.items()}
    # equal results from equal seeds, and what one application launches and allocates
    outs, extra, after = {}, {}, {}
    for key, fn in variants.items():
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        seed_all(1)
        counter = CountLaunches()
        ops.TIMER = counter
        try:
            with CountDeviceOps() as mode:
                outs[key] = fn()
        finally:
            ops.TIMER = None
        torch.cuda.synchronize()
        after[key] = (torch.rand(1), np.random.rand())
        extra[key] = {"torch_ops": mode.n, "dva_launches": counter.n,
                      "peak_bytes": int(torch.cuda.max_memory_allocated() - base)}
    a, b = list(outs["eager"]), list(outs["deferred"])
    assert len(a) == len(b) and after["eager"] == after["deferred"], f"{name}: the variants drew differently"
    for u, v in zip(a, b):
        assert torch.equal(u.x, v.x) and torch.equal(u.mappings.pixels, v.mappings.pixels), f"{name}: variants differ"
    windows = [[im.num_views, 3, int(im.x.shape[2]), int(im.x.shape[3])] for im in a]
    nbytes = sum(n * h * w for n, _, h, w in windows) * (3 + 3 + 12)
    del outs, a, b

    def host_window(fn, inner):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / inner

    rows = measure(variants, host_window, reps, seconds, nbytes, extra)
    rows["deferred"]["speedup_vs_eager"] = round(rows["eager"]["ms"] / rows["deferred"]["ms"], 2)
    return {"case": name, "source": [B, 3, H, W], "chain": [type(tr).__name__ for tr in chain], "windows": windows,
            "checks": {"deferred_equals_eager": True}, "variants": rows}


def measure(variants, window, reps, seconds, nbytes, extra):
    inner = {}
    for key, fn in variants.items():
        for _ in range(3):
            seed_all(2)
            fn()
        torch.cuda.synchronize()
        inner[key] = max(1, int(seconds * 1e3 / max(window(fn, 3), 1e-3)))
    ms = {key: [] for key in variants}
    for rep in range(reps):
        for key, fn in variants.items():
            seed_all(3 + rep)
            ms[key].append(window(fn, inner[key]))
    rows = {}
    for key in variants:
        med = statistics.median(ms[key])
        rows[key] = {"ms": round(med, 4), "min_ms": round(min(ms[key]), 4), "max_ms": round(max(ms[key]), 4),
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
    extra = {}
    for key, fn in variants.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        counter = CountLaunches()
        ops.TIMER = counter
        try:
            with CountDeviceOps() as mode:
                fn()
        finally:
            ops.TIMER = None
        torch.cuda.synchronize()
        extra[key] = {"torch_ops": mode.n, "dva_launches": counter.n,
                      "peak_bytes": int(torch.cuda.max_memory_allocated() - base)}

    def event_window(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    nbytes = B * Hc * Wc * (3 + 3 + 12)
    rows = measure(variants, event_window, reps, seconds, nbytes, extra)
    rows["window"]["speedup_vs_eager"] = round(rows["eager"]["ms"] / rows["window"]["ms"], 2)
    return {"case": name, "source": [2 * B, 3, H, W], "windows": [[B, 3, Hc, Wc]],
            "checks": {"window_equals_eager": True}, "variants": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from deepviewagg_amd import _lib
    gen = torch.Generator().manual_seed(0)
    result = {"tool": "image_window_bench", "device": torch.cuda.get_device_name(0),
              "dva_version": _lib.load().dva_version(), "source_sha256": _lib.source_sha256(), "reps": args.reps,
              "window_s": args.window, "jitter": list(JITTER), "bytes_per_pixel": {"read": 3, "read_contrast": 3, "written": 12},
              "chains": [run_case(*case, args.reps, args.window, gen) for case in CASES],
              "kernels": [run_kernel_case("window_256", 16, 512, 1024, 256, 256, args.reps, args.window, gen),
                          run_kernel_case("window_full", 8, 512, 1024, 1024, 512, args.reps, args.window, gen)]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
