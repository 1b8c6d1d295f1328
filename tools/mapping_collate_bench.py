#!/usr/bin/env python
"""Time the collation of mappings on the device: the one-op route (``ImageMapping.COLLATE_ON_DEVICE = True``,
``ops.collate_mapping``) against the kept torch composition (the switch off: the parent commit's
``CSRBatch.from_csr_list``, moved unchanged into ``_from_csr_list_composition``, followed by ``insert_empty_groups``).

Whole calls are timed, on samples that live on the device:
  from_csr_list   ``ImageMappingBatch.from_csr_list`` of the samples' mappings
  image_batch     ``ImageBatch.from_data_list`` of the samples' image data, with one setting and with two (every second
                  sample lacks the second setting, so its points become empty groups of that setting's batch)
Batches of 2, 4, 8 and 16 samples that add up to the reference's training batch (3 x 10^5 points), and one batch of 8
samples with 2^20 points.  Exact mappings (one pixel per view), 0 .. 5 views per point, 8 mapping features, 10 images per
sample and setting, no image features (``x`` None: the concatenation of ``x`` is the same on both sides).

A call is timed with the host clock between two device synchronisations (``ms``) and with device events around the same
call (``device_ms``); both sides are warmed up, alternate inside every repetition, and the figure is the median over
--reps repetitions with the min and max.  ``torch_ops`` = aten operator calls on device tensors, ``dva_calls`` = calls
into the HIP library (one ``dva_mapping_collate`` is ``kernel_launches`` launches: maxima, scan, fill for up to 32
items), ``syncs`` = host synchronisations seen by torch's sync debug mode.  ``bytes`` = the mappings read once and the
batch written once; ``share_of_8tb_s`` = bytes / device time over the 8 TB/s HBM peak.
One JSON line on stdout; --out writes it (profiles/mapping_collate_bench.json).

Usage:  python tools/mapping_collate_bench.py [--reps 20] [--out FILE]
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
from bench_scenes import make_collate_mapping  # noqa: E402

HBM_PEAK = 8.0e12
N_IMAGES, N_FEAT = 10, 8
BATCHES = (("batch_3e5", 300000, (2, 4, 8, 16)), ("batch_2^20", 1 << 20, (8,)))
ARMS = {"device": True, "composition": False}


def make_setting(mapping, ref_size, dev):
    from deepviewagg_amd.core.multimodal.image import SameSettingImageData
    return SameSettingImageData(path=np.array([f"i{i}" for i in range(N_IMAGES)]), pos=torch.zeros(N_IMAGES, 3, device=dev),
                                opk=torch.zeros(N_IMAGES, 3, device=dev), ref_size=ref_size, proj_upscale=1,
                                mappings=mapping)


def set_switch(on):
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    ImageMapping.COLLATE_ON_DEVICE = on


def time_both(fn, reps):
    """fn with the switch on ('device') and off ('composition'), alternating inside every repetition."""
    before = lambda key, rep: set_switch(ARMS[key])
    profiles = {}
    for key in ARMS:                                    # warm up, then what one call does, before any timed window
        before(key, None)
        for _ in range(3):
            fn()
        profiles[key] = measure.profile_once(fn)
    both, _ = measure.alternate(dict.fromkeys(ARMS, fn), reps, measure.both_window, warmup=0, before=before)
    rows = {}
    for key in ARMS:
        host, dev = (measure.summarise(ms, 4) for ms in zip(*both[key]))
        profile = profiles[key]
        rows[key] = {"ms": host["median"], "min_ms": host["min"], "max_ms": host["max"], "device_ms": dev["median"],
                     "device_min_ms": dev["min"], "device_max_ms": dev["max"], "reps": reps,
                     "torch_ops": profile["torch_ops"], "dva_calls": profile["dva_launches"], "syncs": profile["syncs"]}
    set_switch(True)
    rows["device"]["speedup_vs_composition"] = round(rows["composition"]["ms"] / rows["device"]["ms"], 2)
    rows["device"]["ranges_overlap"] = measure.ranges_overlap(
        *((rows[key]["min_ms"], rows[key]["max_ms"]) for key in ARMS))
    return rows


def mappings_equal(a, b):
    return all(torch.equal(u, v) for u, v in ((a.pointers, b.pointers), (a.images, b.images),
                                              (a.values[1].pointers, b.values[1].pointers), (a.pixels, b.pixels),
                                              (a.features, b.features)))


def both(fn):
    set_switch(True)
    got = fn()
    set_switch(False)
    comp = fn()
    set_switch(True)
    return got, comp


def moved_bytes(batches):
    """Every mapping of the batch read once and written once."""
    total = 0
    for m in batches:
        total += 2 * ((m.num_groups + 1) * 8 + m.num_views * (24 + 4 * N_FEAT) + m.num_atoms * 4)
    return int(total)


def finish(rows, nbytes, n_items):
    launches = sum(2 * ((k + 31) // 32) + 1 for k in n_items)
    for row in rows.values():
        row["bytes"] = nbytes
        row["share_of_8tb_s"] = round(nbytes / (row["device_ms"] * 1e-3) / HBM_PEAK, 5)
    rows["device"]["kernel_launches"] = launches
    return rows


def run_batch(name, n_points, n_samples, reps, gen, dev):
    from deepviewagg_amd.core.multimodal.image import ImageBatch, ImageData, ImageMappingBatch
    per = [n_points // n_samples + (1 if i < n_points % n_samples else 0) for i in range(n_samples)]
    first = [make_collate_mapping(n, N_IMAGES, N_FEAT, gen, dev) for n in per]
    second = [make_collate_mapping(n, N_IMAGES, N_FEAT, gen, dev) if i % 2 == 0 else None for i, n in enumerate(per)]
    one = [ImageData([make_setting(m, (1024, 512), dev)]) for m in first]
    two = [ImageData([make_setting(m, (1024, 512), dev)] + ([make_setting(s, (512, 256), dev)] if s is not None else []))
           for m, s in zip(first, second)]
    out = {"case": name, "points": n_points, "samples": n_samples, "views": sum(m.num_views for m in first),
           "features": N_FEAT, "calls": {}}

    fn = lambda: ImageMappingBatch.from_csr_list(first)
    got, comp = both(fn)
    assert mappings_equal(got, comp), f"{name} x {n_samples}: from_csr_list differs from the composition"
    nbytes = moved_bytes([got])
    del got, comp
    out["calls"]["from_csr_list"] = finish(time_both(fn, reps), nbytes, [n_samples])

    for key, items in (("image_batch_1_setting", one), ("image_batch_2_settings", two)):
        fn = lambda items=items: ImageBatch.from_data_list(items)
        got, comp = both(fn)
        assert len(got) == len(comp) and all(mappings_equal(a.mappings, b.mappings) for a, b in zip(got, comp)), \
            f"{name} x {n_samples}: {key} differs from the composition"
        nbytes = moved_bytes([im.mappings for im in got])
        n_items = [im.mappings.__sizes__.shape[0] for im in got]
        del got, comp
        out["calls"][key] = finish(time_both(fn, reps), nbytes, n_items)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    result = measure.header(
        "mapping_collate_bench", reps=args.reps,
        composition="the parent commit's from_csr_list + insert_empty_groups (ImageMapping.COLLATE_ON_DEVICE = False)",
        batches=[run_batch(name, n, k, args.reps, gen, dev) for name, n, sizes in BATCHES for k in sizes])
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
