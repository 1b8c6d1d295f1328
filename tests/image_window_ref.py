"""The windowed image tail's oracle and the scenes its tests share, no test by itself.

``window_np``     the window of ``ops.image_window`` on numpy arrays: per output image ``np.roll`` of its source image
                  along W, then a slice.  It composes with ``image_tail_ref.numpy_tail``; every comparison made with
                  it is byte for byte.
``host_kernels``  stand-ins that let the mapping side of the online chains run on host tensors.  The product sorts,
                  de-duplicates and averages mappings with HIP kernels only (no CPU fallback), so a host test of the
                  chains replaces exactly those three primitives by their torch / numpy definitions -- for the eager
                  and the deferred chain alike; what such a test compares is the image side.
``golden_setting`` / ``s3dis_head``  the setting and the chain of the chain tests, on any device."""
import contextlib

import numpy as np
import torch

from conftest import load_golden, t


def window_np(src, index, rolls, offsets, size):
    """src uint8 [N, 3, H, W], index [B], rolls [B], offsets [B, 2] = (x, y), size = (Wc, Hc) -> uint8 [B, 3, Hc, Wc]."""
    Wc, Hc = int(size[0]), int(size[1])
    W = src.shape[-1]
    out = np.empty((len(index), src.shape[1], Hc, Wc), dtype=src.dtype)
    for b, i in enumerate(index):
        rolled = np.roll(src[int(i)], int(rolls[b]) % W, axis=-1)
        x, y = int(offsets[b][0]), int(offsets[b][1])
        assert 0 <= x <= W - Wc and 0 <= y <= src.shape[-2] - Hc
        out[b] = rolled[:, y:y + Hc, x:x + Wc]
    return out


# ---- the mapping primitives on the host -----------------------------------------------------------------------------

def _argsort_keys(keys):
    order = torch.sort(keys, stable=True).indices
    return order, keys[order]


def _argunique_keys(keys):
    return torch.from_numpy(np.unique(keys.numpy(), return_index=True)[1])


def _segment_mean(src, pointers, reduce='mean'):
    assert reduce == 'mean'
    sizes = (pointers[1:] - pointers[:-1])
    group = torch.arange(sizes.shape[0]).repeat_interleave(sizes)
    sums = torch.zeros((sizes.shape[0], src.shape[1]), dtype=src.dtype).index_add_(0, group, src)
    return sums / sizes.clamp(min=1).view(-1, 1).to(src.dtype)


@contextlib.contextmanager
def host_kernels():
    from deepviewagg_amd import ops
    from deepviewagg_amd.core.multimodal import image as I
    from deepviewagg_amd.utils import multimodal as U
    saved = (U.argsort_keys, U.argunique_keys, ops.segment_csr, I._compute_device)
    U.argsort_keys, U.argunique_keys, ops.segment_csr, I._compute_device = (
        _argsort_keys, _argunique_keys, _segment_mean, lambda tensor: tensor.device)
    try:
        yield
    finally:
        U.argsort_keys, U.argunique_keys, ops.segment_csr, I._compute_device = saved


# ---- the scene of the chain tests -----------------------------------------------------------------------------------

class Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def golden_setting(dev, seed=0):
    """The six images and the mappings of tests/golden/transforms.npz with three random uint8 planes of 64 x 128
    (built like tests/test_gpu_transforms_golden.py::fresh), and a ``data`` that keeps 100 of its 150 points."""
    from deepviewagg_amd.core.multimodal.image import ImageMapping, SameSettingImageData
    g = load_golden("transforms")
    N, B = int(g["num_points"]), g["x"].shape[0]
    W, H = (int(v) for v in g["ref_size"])
    m = ImageMapping.from_dense(t(g["point_ids"], dev), t(g["image_ids"], dev), t(g["pixels_dense"], dev),
                                t(g["map_features_dense"], dev), num_points=N)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, 3, H, W), generator=gen, dtype=torch.uint8)
    images = SameSettingImageData(path=np.array([f"img_{i}" for i in range(B)]), pos=t(g["pos"], dev),
                                  opk=torch.zeros(B, 3, device=dev), ref_size=(W, H), proj_upscale=1, mappings=m,
                                  x=x.to(dev))
    keep = torch.randperm(N, generator=gen)[:100].to(dev)
    data = Data(pos=torch.rand(100, 3, generator=gen).to(dev), mapping_index=keep, num_nodes=100)
    return data, images


def s3dis_head(T, roll=True, min_size=16, credit=128 * 64 * 2):
    """The image side of the S3DIS train chain in front of the tail; the KITTI-360 chain is the same without CenterRoll."""
    head = [T.SelectMappingFromPointId()] + ([T.CenterRoll(angular_res=16)] if roll else [])
    return head + [T.PickImagesFromMappingArea(area_ratio=0.003, n_max=5), T.CropImageGroups(padding=2, min_size=min_size),
                   T.PickImagesFromMemoryCredit(credit=credit, k_coverage=2)]


def run_chain(transforms, data, images, seed):
    """The chain from equal torch / numpy / random states; returns what it made and the next draw of each generator."""
    import random
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    for tr in transforms:
        data, images = tr(data, images)
    return data, images, (torch.rand(1), np.random.rand(), random.random())


def settings_of(images):
    from deepviewagg_amd.core.multimodal.image import ImageData
    return list(images) if isinstance(images, ImageData) else [images]


def assert_same_settings(a, b):
    """x, mappings and the roll / crop state of every setting, bit for bit."""
    a, b = settings_of(a), settings_of(b)
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert tuple(u.crop_size) == tuple(v.crop_size) and u.num_views == v.num_views
        assert torch.equal(u.crop_offsets, v.crop_offsets)
        assert torch.equal(u.rollings.cpu(), v.rollings.cpu())
        assert torch.equal(u.pos, v.pos)
        mu, mv = u.mappings, v.mappings
        assert torch.equal(mu.pointers, mv.pointers) and torch.equal(mu.images, mv.images)
        assert torch.equal(mu.values[1].pointers, mv.values[1].pointers) and torch.equal(mu.pixels, mv.pixels)
        assert torch.equal(mu.features, mv.features)
        xu, xv = u.x, v.x
        assert xu.dtype == xv.dtype and xu.shape == xv.shape
        assert torch.equal(xu.contiguous().view(torch.uint8), xv.contiguous().view(torch.uint8))
