#!/usr/bin/env python
"""Loading images on the device (csrc/image_load.hip) against the PIL composition of the reference on the host, at the
source and target sizes of the three datasets the reference's multimodal data configs serve:

  s3dis      4096 x 2048 equirectangular PNG -> resolution_2d [1024, 512]; NonStaticMask at proj_upscale 2 (2048 x 1024)
  scannet    1296 x 968 JPEG                 -> resolution_2d [320, 240];  NonStaticMask at proj_upscale 1
  kitti360   1408 x 376 PNG                  -> resolution_2d [1408, 376]: no resize, the op is a copy into the planar
                                                layout (one pass); NonStaticMask at proj_upscale 1

Per dataset:
  decoded    from already decoded arrays: ``ops.read_images_u8`` on sources resident on the device (device events: the
             time of its launches), the same with the upload of the sources (host clock, synchronised), and the PIL
             composition on the host plus the upload of its result (host clock, synchronised)
  load       the whole ``SameSettingImageData.load()`` from files, decoding included, device route against host route
  mask       ``NonStaticMask`` end to end (draw, decode, resize to proj_size, compare), device route against host route

For the op: its launches, and the achieved bytes per second over the ALGORITHMIC bytes of every pass (source read once,
intermediate written once and read once, result written once) as a share of the 8 TB/s HBM specification.  Results of
the two routes are compared byte for byte before anything is timed.  Every figure is the median of ``--reps`` windows of
about ``--window`` seconds, the two routes alternating; min and max are reported with it.

One JSON line on stdout; --out writes it (profiles/image_load_bench.json).

Usage:  python tools/image_load_bench.py [--reps 5] [--window 0.5] [--out FILE]
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import measure  # noqa: E402

HBM_PEAK = 8.0e12
# name, views, source (W, H), ref_size, proj_upscale, file type
CASES = (("s3dis", 8, (4096, 2048), (1024, 512), 2, "png"),
         ("scannet", 16, (1296, 968), (320, 240), 1, "jpg"),
         ("kitti360", 16, (1408, 376), (1408, 376), 1, "png"))


def scene_image(W, H, seed):
    """A smooth image with some noise (a photograph's statistics matter to the decoder, not to the resample)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    planes = [127 + 100 * np.sin(xx / (37.0 + 11 * c) + seed) * np.cos(yy / (23.0 + 7 * c)) for c in range(3)]
    img = np.stack(planes, axis=2) + rng.normal(0, 6, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def algorithmic_bytes(N, Hs, Ws, size):
    """Bytes of the passes of a plain load (resize to ``size``, no roll, no crop, downscale 1), 3 per pixel."""
    W, H = size
    sizes = [(Hs, Ws)]
    if Ws != W:
        sizes.append((Hs, W))
    if Hs != H:
        sizes.append((H, W))
    if len(sizes) == 1:
        sizes.append((H, W))
    return sum(3 * N * (a[0] * a[1] + b[0] * b[1]) for a, b in zip(sizes[:-1], sizes[1:]))


def windows(variants, window_fn, reps, seconds):
    ms, inner = measure.alternate(variants, reps, window_fn, warmup=1, seconds=seconds)
    rows = {}
    for key in variants:
        s = measure.summarise(ms[key], 4)
        rows[key] = {"ms": s["median"], "min_ms": s["min"], "max_ms": s["max"], "calls_per_window": inner[key]}
    return rows


def run_case(name, N, src_size, ref_size, upscale, ext, reps, seconds, tmp):
    from PIL import Image
    from deepviewagg_amd import ops
    from deepviewagg_amd.core.data_transform.multimodal.image import NonStaticMask
    from deepviewagg_amd.core.multimodal import image as I
    dev = torch.device("cuda", 0)
    Ws, Hs = src_size
    decoded, paths = [], []
    for i in range(N):
        path = os.path.join(tmp, f"{name}_{i}.{ext}")
        Image.fromarray(scene_image(Ws, Hs, i)).save(path, **({"quality": 90} if ext == "jpg" else {}))
        paths.append(path)
        decoded.append(I.decode_image(path))
    zeros2 = torch.zeros((N, 2), dtype=torch.int64)
    rolls = torch.zeros(N, dtype=torch.int64)

    def pil():
        return I._read_images_pil(decoded, ref_size, rolls, ref_size, zeros2, 1).to(dev)

    resident = torch.from_numpy(np.stack(decoded)).to(dev)

    def op():
        return ops.read_images_u8(resident, ref_size, downscale=1)

    def upload_op():
        return ops.read_images_u8(torch.from_numpy(np.stack(decoded)).to(dev), ref_size, downscale=1)
    assert torch.equal(op(), pil()) and torch.equal(upload_op(), pil()), f"{name}: the device op and PIL differ"
    with measure.launch_counter() as counter:
        op()
    nbytes = algorithmic_bytes(N, Hs, Ws, ref_size)
    kernel = windows({"op": op}, measure.event_window, reps, seconds)["op"]
    kernel.update(launches=counter.names, algorithmic_bytes=nbytes,
                  tb_per_s=round(nbytes / (kernel["ms"] * 1e-3) / 1e12, 4),
                  share_of_8tb_s=round(nbytes / (kernel["ms"] * 1e-3) / HBM_PEAK, 4))
    decoded_rows = windows({"device_upload_and_op": upload_op, "pil_and_upload": pil}, measure.host_window, reps, seconds)
    decoded_rows["op_on_resident_sources"] = kernel

    def setting(on_device):
        im = I.SameSettingImageData(path=np.array(paths), pos=torch.zeros(N, 3, device=dev), ref_size=ref_size,
                                    proj_upscale=upscale)
        im.LOAD_ON_DEVICE = on_device                           # on the instance: the class default stands
        return im

    def load(on_device):
        return lambda: setting(on_device).load().x
    assert torch.equal(load(True)(), load(False)()), f"{name}: load() differs between the routes"
    decode_ms = measure.host_window(lambda: [I.decode_image(p) for p in paths])
    load_rows = windows({"device": load(True), "host": load(False)}, measure.host_window, reps, seconds)
    load_rows["decode_alone_ms"] = round(decode_ms, 3)

    tr = NonStaticMask(ref_size=ref_size, proj_upscale=upscale, n_sample=5)

    def mask(on_device):
        def fn():
            torch.manual_seed(5)
            return tr(None, setting(on_device))[1].mask
        return fn
    assert torch.equal(mask(True)(), mask(False)()), f"{name}: NonStaticMask differs between the routes"
    mask_rows = windows({"device": mask(True), "host": mask(False)}, measure.host_window, reps, seconds)
    for rows in (decoded_rows, load_rows, mask_rows):
        if "device" in rows:
            rows["device"]["speedup_vs_host"] = round(rows["host"]["ms"] / rows["device"]["ms"], 2)
    decoded_rows["device_upload_and_op"]["speedup_vs_pil"] = round(
        decoded_rows["pil_and_upload"]["ms"] / decoded_rows["device_upload_and_op"]["ms"], 2)
    return {"case": name, "views": N, "source": [Ws, Hs], "ref_size": list(ref_size), "proj_upscale": upscale, "files": ext,
            "checks": {"device_equals_pil": True}, "decoded": decoded_rows, "load": load_rows, "nonstatic_mask": mask_rows}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of work per timed window")
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "image_load_bench measures on a HIP device"
    import PIL
    with tempfile.TemporaryDirectory() as tmp:
        cases = [run_case(*c, args.reps, args.window, tmp) for c in CASES if c[0] in args.cases.split(",")]
    measure.emit(measure.header("image_load_bench", pillow=PIL.__version__, host_cpu_threads=torch.get_num_threads(),
                                reps=args.reps, window_s=args.window, cases=cases), args.out)


if __name__ == "__main__":
    main()
