#!/usr/bin/env python
"""Time the four mapping selections on the device, the one-op route (``ImageMapping.SELECT_ON_DEVICE = True``,
``ops.select_mapping``) against the kept torch compositions (the switch off: their text is the parent commit's method
bodies, moved unchanged into ``_select_images_composition``, ``_select_views_composition``, ``_crop_composition`` and
the CSR indexing of a pick).

Per method, at two sizes (an area: 2^20 points; the reference batch: 3 x 10^5 points; about 8 views per point, one
pixel per view, 300 images, 8 mapping features):
  pick     10^5 random points (3 x 10^4 at the batch size)
  images   256 of the 300 images in permuted order
  views    a mask that keeps 30 % of the views (the image count given, as SameSettingImageData gives it)
  crop     256 x 256 windows at random per-image offsets of 1024 x 512 images
Per sample: the three online chains of tools/image_window_bench.py (s3dis_32, kitti360_32, crop_group_16), deferred
form, switch on against switch off.

A selection ends in a host readback, so a call is timed with the host clock between two device synchronisations
(``ms``) and with device events around the same call (``device_ms``); both sides are warmed up, alternate inside every
repetition, and the figure is the median over --reps repetitions with the min and max.  ``torch_ops`` = aten operator
calls on device tensors, ``dva_launches`` = calls into the HIP library, ``syncs`` = host synchronisations seen by
torch's sync debug mode, ``peak_bytes`` = peak allocated device memory above what is resident before the call.
``bytes`` = the algorithmic bytes of the selection (the mapping rows of the selected points read once, the result
written once); ``share_of_8tb_s`` = bytes / device time over the 8 TB/s HBM peak.
One JSON line on stdout; --out writes it (profiles/mapping_select_bench.json).

Usage:  python tools/mapping_select_bench.py [--reps 20] [--out FILE]
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
from bench_scenes import CASES, make_chain, make_scene, make_select_mapping, run_chain, seed_all  # noqa: E402

HBM_PEAK = 8.0e12
N_IMAGES, N_FEAT = 300, 8
SIZES = (("area_2^20", 1 << 20, 100000), ("batch_3e5", 300000, 30000))
ARMS = {"device": True, "composition": False}


def set_switch(on):
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    ImageMapping.SELECT_ON_DEVICE = on


def time_both(fn, reps, seed=False):
    """fn with the switch on ('device') and off ('composition'), alternating inside every repetition; with ``seed``
    every call starts from the seeds of its repetition."""
    def before(key, rep):
        set_switch(ARMS[key])
        if seed:
            seed_all(3 + (rep or 0))

    profile = {}
    for key in ARMS:                                    # warm up, then what one call does, before any timed window
        for _ in range(3):
            before(key, None)
            fn()
        before(key, None)
        profile[key] = measure.profile_once(fn)
    both, _ = measure.alternate(dict.fromkeys(ARMS, fn), reps, measure.both_window, warmup=0, before=before)
    rows = {}
    for key in ARMS:
        host, dev = (measure.summarise(ms, 4) for ms in zip(*both[key]))
        rows[key] = {"ms": host["median"], "min_ms": host["min"], "max_ms": host["max"], "device_ms": dev["median"],
                     "device_min_ms": dev["min"], "device_max_ms": dev["max"], "reps": reps, **profile[key]}
    set_switch(True)
    rows["device"]["speedup_vs_composition"] = round(rows["composition"]["ms"] / rows["device"]["ms"], 2)
    rows["device"]["ranges_overlap"] = measure.ranges_overlap(
        *((rows[key]["min_ms"], rows[key]["max_ms"]) for key in ARMS))
    return rows


def mapping_bytes(m, rows_read):
    """Bytes of ``rows_read`` (points, views, atoms) read plus the whole of mapping ``m`` written."""
    f = m.features.shape[1] if m.has_features else 0
    read = rows_read[0] * 16 + rows_read[1] * (24 + 4 * f) + rows_read[2] * 4
    written = (m.num_groups + 1) * 8 + m.num_views * (24 + 4 * f) + m.num_atoms * 4
    return int(read + written)


def run_methods(name, n, n_pick, reps, gen, dev):
    m = make_select_mapping(n, N_IMAGES, N_FEAT, gen, dev)
    pick = torch.randperm(n, generator=gen)[:n_pick].to(dev)
    idx = torch.randperm(N_IMAGES, generator=gen)[:256].to(dev)
    mask = (torch.rand(m.num_views, generator=gen) < 0.3).to(dev)
    offsets = torch.stack([torch.randint(0, 1024 - 256, (N_IMAGES,), generator=gen),
                           torch.randint(0, 512 - 256, (N_IMAGES,), generator=gen)], 1).to(dev)
    methods = {"pick": lambda: m.select_points(pick, mode='pick'), "images": lambda: m.select_images(idx),
               "views": lambda: m.select_views(mask, num_images=N_IMAGES)[0],
               "crop": lambda: m.crop((256, 256), offsets)}
    out = {"case": name, "points": n, "views": m.num_views, "atoms": m.num_atoms, "images": N_IMAGES,
           "features": N_FEAT, "methods": {}}
    for key, fn in methods.items():
        set_switch(True)
        got = fn()
        set_switch(False)
        comp = fn()
        set_switch(True)
        same = all(torch.equal(a, b) for a, b in ((got.pointers, comp.pointers), (got.images, comp.images),
                                                  (got.values[1].pointers, comp.values[1].pointers),
                                                  (got.pixels, comp.pixels), (got.features, comp.features)))
        assert same, f"{name} {key}: the device route and the composition differ"
        if key == "pick":
            sel_views = int((m.pointers[pick + 1] - m.pointers[pick]).sum())
            rows_read = (n_pick, sel_views, sel_views)
        else:
            rows_read = (n, m.num_views, m.num_atoms)
        nbytes = mapping_bytes(got, rows_read)
        del got, comp
        rows = time_both(fn, reps)
        for row in rows.values():
            row["bytes"] = nbytes
            row["share_of_8tb_s"] = round(nbytes / (row["device_ms"] * 1e-3) / HBM_PEAK, 5)
        out["methods"][key] = rows
    return out


def run_chain_case(name, B, H, W, kind, reps, gen, dev):
    from deepviewagg_amd.core.data_transform.multimodal import image as T
    images, keep = make_scene(B, H, W, gen, dev)
    transforms = T.defer_image_windows(make_chain(kind, H, W))
    fn = lambda: run_chain(transforms, images, keep)
    outs, after = {}, {}
    for key, on in ARMS.items():
        set_switch(on)
        seed_all(1)
        outs[key] = list(fn())
        after[key] = (torch.rand(1), np.random.rand())
    set_switch(True)
    assert after["device"] == after["composition"] and len(outs["device"]) == len(outs["composition"])
    for u, v in zip(outs["device"], outs["composition"]):
        assert torch.equal(u.x, v.x) and torch.equal(u.mappings.pixels, v.mappings.pixels), f"{name}: chains differ"
        assert torch.equal(u.mappings.pointers, v.mappings.pointers) and torch.equal(u.mappings.images, v.mappings.images)
    del outs
    return {"case": name, "source": [B, 3, H, W], "chain": [type(tr).__name__ for tr in transforms],
            "variants": time_both(fn, reps, seed=True)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-chains", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    result = measure.header("mapping_select_bench", reps=args.reps,
                            composition="the parent commit's method bodies (ImageMapping.SELECT_ON_DEVICE = False)",
                            methods=[run_methods(name, n, k, args.reps, gen, dev) for name, n, k in SIZES], chains=[])
    if not args.skip_chains:
        for name, B, H, W, kind in CASES:
            if name == "s3dis_64":
                continue
            result["chains"].append(run_chain_case(name, B, H, W, kind, args.reps, gen, dev))
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
