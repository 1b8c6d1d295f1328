#!/usr/bin/env python
"""Time ``CenterRoll`` and ``PickImagesFromMemoryCredit`` on the device: the routes through ``mapping_pick.hip``
(``CenterRoll.ON_DEVICE`` / ``PickImagesFromMemoryCredit.ON_DEVICE`` = True) against the kept compositions (the switches
off: their text is the parent commit's method bodies, moved unchanged into ``_process_composition``).

Rows:
  CenterRoll                   32 and 64 images of 1024 x 512 on a 3 x 10^5-point sample, in the deferred form the shipped
                               chains hand it (no pixel work in this step: the roll goes into ``source_roll``)
  PickImagesFromMemoryCredit   the crop-group ImageData of s3dis_32 / s3dis_64 (SelectMappingFromPointId, CenterRoll,
                               PickImagesFromMappingArea, CropImageGroups in front; n_img = 4) and of kitti360_32 (the
                               same without CenterRoll) on a 3 x 10^5-point sample; a ScanNet-like setting: 100 images
                               of 320 x 240, n_img = 25, 10^5 points; k_coverage = 2 everywhere
  chains                       the three online chains of tools/image_window_bench.py (its 2 x 10^4-point scenes), both
                               switches on against both off

A call ends in host read-backs, so it is timed with the host clock between two device synchronisations, read-backs
included; both routes are warmed up and alternate inside every repetition, on fresh inputs and the same random seeds; the
figure is the median over --reps repetitions with the min and max.  ``torch_ops`` = aten operator calls on device
tensors, ``dva_launches`` = calls into the HIP library, ``syncs`` = host synchronisations seen by torch's sync debug
mode, ``peak_bytes`` = peak allocated device memory above what is resident before the call.
One JSON line on stdout; --out writes it (profiles/image_pick_bench.json).

Usage:  python tools/image_pick_bench.py [--reps 15] [--out FILE]
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
from bench_scenes import CASES, Data, make_chain, make_scene, run_chain, seed_all  # noqa: E402

ARMS = {"device": True, "composition": False}


def set_switch(on):
    from deepviewagg_amd.core.data_transform.multimodal.image import CenterRoll, PickImagesFromMemoryCredit
    CenterRoll.ON_DEVICE = PickImagesFromMemoryCredit.ON_DEVICE = on


def big_scene(B, H, W, n_points, gen, dev, pixels=True):
    """B images of W x H over ``n_points`` points: image i sees random points through one random box (the scene of
    tools/bench_scenes.py at another point count)."""
    from deepviewagg_amd.core.multimodal.image import ImageMapping, SameSettingImageData
    pts, imgs, pix = [], [], []
    for i in range(B):
        bw, bh = int(torch.randint(40, W // 2, (1,), generator=gen)), int(torch.randint(40, H // 2, (1,), generator=gen))
        x0, y0 = int(torch.randint(0, W - bw, (1,), generator=gen)), int(torch.randint(0, H - bh, (1,), generator=gen))
        n = int(torch.randint(bw * bh // 2, bw * bh, (1,), generator=gen))
        pts.append(torch.randint(0, n_points, (n,), generator=gen))
        imgs.append(torch.full((n,), i))
        pix.append(torch.stack([x0 + torch.randint(0, bw, (n,), generator=gen),
                                y0 + torch.randint(0, bh, (n,), generator=gen)], 1).short())
    pts, imgs, pix = torch.cat(pts), torch.cat(imgs), torch.cat(pix)
    m = ImageMapping.from_dense(pts.to(dev), imgs.to(dev), pix.to(dev), torch.rand(pts.shape[0], 2, generator=gen).to(dev),
                                num_points=n_points)
    x = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=gen).to(dev) if pixels else None
    images = SameSettingImageData(path=np.array([f"img_{i}" for i in range(B)]), pos=torch.zeros(B, 3, device=dev),
                                  opk=torch.zeros(B, 3, device=dev), ref_size=(W, H), proj_upscale=1, mappings=m, x=x)
    return images


def time_both(fn, prepare, reps):
    """``fn(prepare(rep))`` with the switches on ('device') and off ('composition'), alternating inside every
    repetition; ``prepare`` (fresh inputs, seeds) is outside the timed region."""
    args = []

    def before(key, rep):
        set_switch(ARMS[key])
        args[:] = [prepare(rep or 0)]

    call = lambda: fn(args[0])
    profile = {}
    for key in ARMS:                                    # warm up, then what one call does, before any timed window
        for _ in range(3):
            before(key, None)
            call()
        before(key, None)
        profile[key] = measure.profile_once(call)
    ms, _ = measure.alternate(dict.fromkeys(ARMS, call), reps, measure.host_window, warmup=0, before=before)
    rows = {}
    for key in ARMS:
        s = measure.summarise(ms[key], 4)
        rows[key] = {"ms": s["median"], "min_ms": s["min"], "max_ms": s["max"], "reps": reps, **profile[key]}
    set_switch(True)
    rows["device"]["speedup_vs_composition"] = round(rows["composition"]["ms"] / rows["device"]["ms"], 2)
    rows["device"]["range_below_composition"] = rows["device"]["max_ms"] < rows["composition"]["min_ms"]
    return rows


def mappings_equal(a, b):
    return all(torch.equal(p, q) for p, q in ((a.pointers, b.pointers), (a.images, b.images),
                                              (a.values[1].pointers, b.values[1].pointers), (a.pixels, b.pixels)))


def run_center_roll(name, B, H, W, n_points, reps, gen, dev):
    from deepviewagg_amd.core.data_transform.multimodal.image import CenterRoll
    from deepviewagg_amd.core.multimodal.image import WindowedSameSettingImageData
    images = big_scene(B, H, W, n_points, gen, dev)
    data = Data(pos=torch.zeros(n_points, 3, device=dev), num_nodes=n_points)
    tr = CenterRoll()

    def prepare(rep):
        # the transform rolls the mapped columns in place, and a mapping's clone shares its tensors: fresh pixels
        im = WindowedSameSettingImageData.defer(images)
        im.mappings.values[1] = im.mappings.values[1].clone()
        im.mappings.pixels = images.mappings.pixels.clone()
        return im

    def fn(args):
        return tr(data, args)[1]
    outs = {}
    for key, on in (("device", True), ("composition", False)):
        set_switch(on)
        outs[key] = fn(prepare(0))
    set_switch(True)
    assert torch.equal(outs["device"].rollings, outs["composition"].rollings), f"{name}: rollings differ"
    assert torch.equal(outs["device"].source_roll, outs["composition"].source_roll)
    assert mappings_equal(outs["device"].mappings, outs["composition"].mappings), f"{name}: mappings differ"
    m = images.mappings
    return {"transform": "CenterRoll", "case": name, "images": B, "size": [W, H], "points": n_points,
            "views": m.num_views, "atoms": m.num_atoms, "variants": time_both(fn, prepare, reps)}


def run_memory_credit(name, images, n_points, W, H, n_img, reps, dev):
    from deepviewagg_amd.core.data_transform.multimodal.image import PickImagesFromMemoryCredit
    data = Data(pos=torch.zeros(n_points, 3, device=dev), num_nodes=n_points)
    tr = PickImagesFromMemoryCredit(img_size=[W, H], n_img=n_img, k_coverage=2)

    def prepare(rep):
        seed_all(3 + rep)
        return images                                         # the transform selects from it and leaves it alone

    def fn(args):
        return tr(data, args)[1]
    outs, after = {}, {}
    for key, on in (("device", True), ("composition", False)):
        set_switch(on)
        outs[key] = list(fn(prepare(0)))
        after[key] = np.random.rand()
    set_switch(True)
    assert after["device"] == after["composition"] and len(outs["device"]) == len(outs["composition"])
    for u, v in zip(outs["device"], outs["composition"]):
        assert list(u.path) == list(v.path) and mappings_equal(u.mappings, v.mappings), f"{name}: picks differ"
    return {"transform": "PickImagesFromMemoryCredit", "case": name, "settings": len(images),
            "images": images.num_views, "points": n_points, "views": sum(im.mappings.num_views for im in images),
            "n_img": n_img, "picked": sum(u.num_views for u in outs["device"]), "output_settings": len(outs["device"]),
            "variants": time_both(fn, prepare, reps)}


def crop_groups(B, H, W, kind, n_points, gen, dev):
    """The ImageData that reaches PickImagesFromMemoryCredit in the shipped chains."""
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    images = big_scene(B, H, W, n_points, gen, dev)
    keep = torch.randperm(n_points, generator=gen)[:n_points].to(dev)
    data = Data(pos=torch.zeros(n_points, 3, device=dev), mapping_index=keep, num_nodes=n_points)
    head = [T.SelectMappingFromPointId()] + ([T.CenterRoll()] if kind == "s3dis" else [])
    head += [T.PickImagesFromMappingArea(use_bbox=False), T.CropImageGroups(padding=8, min_size=64)]
    out = images
    for tr in T.defer_image_windows(head):
        data, out = tr(data, out)
    return out


def run_chain_case(name, B, H, W, kind, reps, gen, dev):
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    images, keep = make_scene(B, H, W, gen, dev)
    transforms = T.defer_image_windows(make_chain(kind, H, W))

    def prepare(rep):
        seed_all(3 + rep)

    def fn(args):
        return run_chain(transforms, images, keep)
    outs, after = {}, {}
    for key, on in ARMS.items():
        set_switch(on)
        seed_all(1)
        outs[key] = list(fn(None))
        after[key] = (torch.rand(1), np.random.rand())
    set_switch(True)
    assert after["device"] == after["composition"] and len(outs["device"]) == len(outs["composition"])
    for u, v in zip(outs["device"], outs["composition"]):
        assert torch.equal(u.x, v.x) and mappings_equal(u.mappings, v.mappings), f"{name}: chains differ"
    del outs
    return {"case": name, "source": [B, 3, H, W], "chain": [type(tr).__name__ for tr in transforms],
            "variants": time_both(fn, prepare, reps)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-chains", action="store_true")
    args = ap.parse_args(argv)
    from deepviewagg_amd.core.multimodal.image import ImageData
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    result = measure.header("image_pick_bench", reps=args.reps,
                            composition="the parent commit's method bodies (ON_DEVICE = False)", rows=[], chains=[])
    n = 300000
    for B in (32, 64):
        result["rows"].append(run_center_roll(f"center_roll_{B}", B, 512, 1024, n, args.reps, gen, dev))
        torch.cuda.empty_cache()
    for name, B, H, W, kind in (("s3dis_32", 32, 512, 1024, "s3dis"), ("s3dis_64", 64, 512, 1024, "s3dis"),
                                ("kitti360_32", 32, 376, 1408, "kitti360")):
        groups = crop_groups(B, H, W, kind, n, gen, dev)
        result["rows"].append(run_memory_credit(name, groups, n, W, H, 4, args.reps, dev))
        del groups
        torch.cuda.empty_cache()
    scannet = ImageData([big_scene(100, 240, 320, 100000, gen, dev)])
    result["rows"].append(run_memory_credit("scannet_like_100", scannet, 100000, 320, 240, 25, args.reps, dev))
    del scannet
    if not args.skip_chains:
        for name, B, H, W, kind in CASES:
            if name == "s3dis_64":
                continue
            result["chains"].append(run_chain_case(name, B, H, W, kind, args.reps, gen, dev))
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
