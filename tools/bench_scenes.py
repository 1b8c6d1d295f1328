"""The synthetic scenes, chains and mappings that more than one side benchmark (``tools/*_bench.py``) measures on."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

JITTER = (0.6, 0.6, 0.7)
N_POINTS = 20000
# the online image chains of the shipped configs: name, images, H, W, kind
CASES = (("s3dis_32", 32, 512, 1024, "s3dis"), ("s3dis_64", 64, 512, 1024, "s3dis"),
         ("kitti360_32", 32, 376, 1408, "kitti360"), ("crop_group_16", 16, 512, 1024, "crop"))


class Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


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


def run_chain(transforms, images, keep):
    """One application of ``transforms`` to the scene: the first transform builds new settings and leaves ``images``
    as it is; ``data`` is rewritten."""
    data = Data(pos=torch.zeros(keep.shape[0], 3, device=keep.device), mapping_index=keep, num_nodes=keep.shape[0])
    out = images
    for tr in transforms:
        data, out = tr(data, out)
    return out


def _exact_mapping(pointers, images, n_feat, gen, dev):
    from deepviewagg_amd.core.multimodal.csr import CSRData
    from deepviewagg_amd.core.multimodal.image import ImageMapping
    v = images.shape[0]
    pixels = torch.stack([torch.randint(0, 1024, (v,), generator=gen), torch.randint(0, 512, (v,), generator=gen)], 1)
    feats = torch.rand(v, n_feat, generator=gen)
    nested = CSRData(torch.arange(v + 1).to(dev), pixels.short().to(dev), dense=False)
    return ImageMapping(pointers.to(dev), images.to(dev), nested, feats.to(dev), dense=False,
                        is_index_value=[True, False, False])


def make_select_mapping(n, n_images, n_feat, gen, dev):
    """n points with 0 .. 16 views each of distinct images, one pixel per view."""
    sizes = torch.randint(0, 17, (n,), generator=gen)
    pointers = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    v = int(pointers[-1])
    point = torch.arange(n).repeat_interleave(sizes)
    within = torch.arange(v) - pointers[:-1].repeat_interleave(sizes)
    images = (torch.randint(0, n_images, (n,), generator=gen)[point] + within) % n_images
    return _exact_mapping(pointers, images, n_feat, gen, dev)


def make_collate_mapping(n, n_images, n_feat, gen, dev):
    """n points with 0 .. 5 views each, one pixel per view; every image is seen."""
    sizes = torch.randint(0, 6, (n,), generator=gen)
    pointers = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    images = torch.randint(0, n_images, (int(pointers[-1]),), generator=gen)
    images[:n_images] = torch.arange(n_images)
    return _exact_mapping(pointers, images, n_feat, gen, dev)
