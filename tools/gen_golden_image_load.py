#!/usr/bin/env python
"""Generate tests/golden/image_load.npz: what the REFERENCE's own ``SameSettingImageData.read_images`` and
``NonStaticMask._process`` give, over the installed Pillow, for small lossless PNGs written to a temporary directory.

TEST INFRASTRUCTURE, runnable only where the reference and PIL are importable (the reference is made importable by
oracle/gen_golden.py, whose stub-import helpers this tool uses as they are).  Nothing in the product or the tests runs
it; they read the committed file.

The fixture holds array data only: the decoded sources (``src/<name>``, uint8 [H, W, 3]), the cases as one JSON string
(``cases``: per case the source names, ``size``, ``rollings``, ``crop_size``, ``crop_offsets``, ``downscale``, ``idx``),
the expected batches (``out/<case>``, uint8 [B, 3, H, W]), the mask cases (``mask_cases``; ``mask/<case>`` bool [W, H],
``rng/<case>`` the host generator state after the transform), the Pillow version and ``producer`` (``reference``: the
reference's own lines ran, not a restatement of them).  The archive is written with fixed timestamps, so the same
inputs give the same bytes.

Usage:  PYTORCH_JIT=0 python tools/gen_golden_image_load.py
"""
import io
import json
import os
import sys
import tempfile
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import PIL  # noqa: E402
from PIL import Image  # noqa: E402

import gen_golden as G  # noqa: E402  (puts the reference and the shims on sys.path, imports ref_image)

OUT = os.path.join(ROOT, "tests", "golden", "image_load.npz")

ROLL3 = [5, -7, 200]                                        # a negative one and one >= W
OFFS3 = [[0, 0], [37, 8], [20, 3]]                          # (40, 11) in (77, 19): left/top, right/bottom, inside
A3 = ["a0", "a1", "a2"]

CASES = [
    dict(name="down_odd", sources=A3, size=(77, 19)),
    dict(name="roll", sources=A3, size=(77, 19), rollings=ROLL3),
    dict(name="crop", sources=A3, size=(77, 19), rollings=ROLL3, crop_size=(40, 11), crop_offsets=OFFS3),
    dict(name="crop_ds1", sources=A3, size=(77, 19), rollings=ROLL3, crop_size=(40, 11), crop_offsets=OFFS3, downscale=1),
    dict(name="crop_ds2", sources=A3, size=(77, 19), rollings=ROLL3, crop_size=(40, 11), crop_offsets=OFFS3, downscale=2),
    dict(name="crop_ds2p5", sources=A3, size=(77, 19), rollings=ROLL3, crop_size=(40, 11), crop_offsets=OFFS3,
         downscale=2.5),
    dict(name="crop_wfull_ds2", sources=A3, size=(77, 19), rollings=ROLL3, crop_size=(77, 11),
         crop_offsets=[[0, 0], [0, 8], [0, 3]], downscale=2),
    dict(name="crop_hfull_ds1", sources=A3, size=(77, 19), rollings=ROLL3, crop_size=(40, 19),
         crop_offsets=[[0, 0], [37, 0], [20, 0]], downscale=1),
    dict(name="full_ds1", sources=A3, size=(77, 19), rollings=ROLL3, downscale=1),
    dict(name="full_ds2", sources=A3, size=(77, 19), rollings=ROLL3, downscale=2),
    dict(name="full_ds2p5", sources=A3, size=(77, 19), rollings=ROLL3, downscale=2.5),
    dict(name="ksize33", sources=["c0"], size=(20, 8)),
    dict(name="up", sources=["b0", "b1"], size=(100, 77)),
    dict(name="width_only", sources=["b0"], size=(100, 30)),
    dict(name="height_only", sources=["b0"], size=(40, 77)),
    dict(name="same", sources=["b0", "b1"], size=(40, 30), rollings=[3, -1]),
    dict(name="same_ds1", sources=["b0", "b1"], size=(40, 30), rollings=[3, -1], downscale=1),
    dict(name="same_crop", sources=["b0", "b1"], size=(40, 30), rollings=[3, -1], crop_size=(17, 9),
         crop_offsets=[[23, 21], [1, 0]]),
    dict(name="wide", sources=["e0"], size=(1100, 6)),
    dict(name="w1", sources=["d0"], size=(1, 4)),
    dict(name="w3", sources=["d0"], size=(3, 4)),
    dict(name="w5", sources=["d0"], size=(5, 4)),
    dict(name="checker_up", sources=["chk"], size=(100, 77)),
    dict(name="checker_down", sources=["chk"], size=(13, 9)),
    dict(name="two_sizes", sources=["a0", "b0", "a1", "b1"], size=(33, 21), rollings=[1, 2, -3, 40]),
    dict(name="idx_int", sources=A3, size=(77, 19), idx=1, rollings=[4]),
    dict(name="idx_tensor", sources=A3, size=(77, 19), idx=[2, 0], rollings=[4, -4]),
    dict(name="idx_slice", sources=A3, size=(77, 19), idx=["slice", 0, 3, 2], rollings=[4, -4]),
]

MASK_VIEWS = ["m0", "m1", "m2", "m3", "m4", "m5"]
MASK_CASES = [dict(name=f"mask_n{n}", sources=MASK_VIEWS, ref_size=(8, 6), proj_upscale=2, n_sample=n, seed=10 + n)
              for n in (1, 2, 5)]


def make_sources():
    rng = np.random.default_rng(20260101)

    def noise(h, w):
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    src = {f"a{i}": noise(67, 301) for i in range(3)}
    src.update({f"b{i}": noise(30, 40) for i in range(2)})
    src["c0"], src["d0"], src["e0"] = noise(64, 160), noise(9, 11), noise(5, 300)
    yy, xx = np.mgrid[0:30, 0:40]
    board = (((xx + yy) % 2) * 255).astype(np.uint8)
    src["chk"] = np.stack([board, board, 255 - board], axis=2)    # 0 / 255 only: both ends of the clamp
    # the mask views: view i differs from m0 in one channel on row i, in two channels on row 6 + i, and in all three on
    # column 2 i and on a few pixels of its own
    base = noise(12, 16)
    src["m0"] = base
    for i in range(1, 6):
        v = base.copy()
        v[i, :, 0] ^= 0xFF
        v[6 + i, :, :2] ^= 0xFF
        v[:, 2 * i, :] ^= 0xFF
        pix = rng.integers(0, [12, 16], (4, 2))
        v[pix[:, 0], pix[:, 1], :] = base[pix[:, 0], pix[:, 1], :] ^ 0x55
        src[f"m{i}"] = v
    return src


def case_idx(spec):
    if spec is None or isinstance(spec, int):
        return spec
    if spec[0] == "slice":
        return slice(*spec[1:])
    return torch.tensor(spec)


def main():
    ref_image = G.ref_image
    transforms = G.import_ref_transforms()
    sources = make_sources()
    arrays = {f"src/{k}": v for k, v in sources.items()}
    with tempfile.TemporaryDirectory() as tmp:
        for name, a in sources.items():
            Image.fromarray(a).save(os.path.join(tmp, name + ".png"))
            with Image.open(os.path.join(tmp, name + ".png")) as im:
                assert np.array_equal(np.asarray(im.convert("RGB")), a), "the PNG round trip is lossless"

        def setting(names, **kw):
            return ref_image.SameSettingImageData(path=np.array([os.path.join(tmp, n + ".png") for n in names]),
                                                  pos=torch.zeros(len(names), 3), **kw)
        for c in CASES:
            kw = {}
            if c.get("rollings") is not None:
                kw["rollings"] = torch.tensor(c["rollings"], dtype=torch.int64)
            if c.get("crop_size") is not None:
                kw["crop_size"] = tuple(c["crop_size"])
                kw["crop_offsets"] = torch.tensor(c["crop_offsets"], dtype=torch.int64)
            out = setting(c["sources"]).read_images(idx=case_idx(c.get("idx")), size=tuple(c["size"]),
                                                    downscale=c.get("downscale"), **kw)
            arrays[f"out/{c['name']}"] = np.ascontiguousarray(out.numpy())
        for c in MASK_CASES:
            images = setting(c["sources"])
            t = transforms.NonStaticMask(ref_size=c["ref_size"], proj_upscale=c["proj_upscale"], n_sample=c["n_sample"])
            torch.manual_seed(c["seed"])
            _, images = t._process(None, images)
            arrays[f"mask/{c['name']}"] = images.mask.numpy()
            arrays[f"rng/{c['name']}"] = torch.get_rng_state().numpy()
    arrays["cases"] = np.array(json.dumps(CASES))
    arrays["mask_cases"] = np.array(json.dumps(MASK_CASES))
    arrays["pillow_version"] = np.array(PIL.__version__)
    arrays["producer"] = np.array("reference")

    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"{os.path.relpath(OUT, ROOT)}  {os.path.getsize(OUT) / 1024:.1f} KiB  ({len(arrays)} arrays, "
          f"Pillow {PIL.__version__})")


if __name__ == "__main__":
    main()
