"""Numpy restatements, on raw arrays, of the two image picks (reference core/data_transform/multimodal/image.py):
CenterRoll's offsets (:999-1029: unique, uint8 wrap-around, scatter min / max, cost, first minimum) and the dense
coverage matrix of PickImagesFromMemoryCredit (:803-868).  The yardsticks of tests/test_image_pick_host.py and
tests/test_gpu_image_pick.py; nothing here imports the package."""
import numpy as np

WIDTHS = (1, 3, 64, 1000, 1296, 1408, 4097, 32767)


def view_images_of_atoms(images, atom_ptr):
    return np.repeat(np.asarray(images, dtype=np.int64), np.diff(np.asarray(atom_ptr, dtype=np.int64)))


def col8_float(x, width):
    """``(x.float() * 256 / W).long()`` with every operation rounded to fp32, as the tensors compute it."""
    x = np.asarray(x).astype(np.float32)
    return ((x * np.float32(256)) / np.float32(width)).astype(np.int64)


def candidates(angular_res):
    return np.arange(0, 256, int(256 / angular_res), dtype=np.int64)


def center_rollings_reference(image_of_atom, x_of_atom, num_images, width, angular_res):
    """``(rollings int64 [B], images without atoms)`` the way the reference computes them: float columns, the distinct
    (image, column) pairs, uint8 wrap-around, per-image min / max per candidate, float cost, first minimum."""
    img = np.asarray(image_of_atom, dtype=np.int64)
    pairs = np.unique(np.stack([img, col8_float(x_of_atom, width)], axis=1), axis=0) if img.size else np.zeros((0, 2), np.int64)
    cand = candidates(angular_res)
    lo = np.full((num_images, cand.size), 255, dtype=np.int64)
    hi = np.zeros((num_images, cand.size), dtype=np.int64)
    rolled = (pairs[:, 1].astype(np.uint8)[:, None] + cand.astype(np.uint8)[None, :]).astype(np.int64)   # wraps
    np.minimum.at(lo, pairs[:, 0], rolled)
    np.maximum.at(hi, pairs[:, 0], rolled)
    centre = np.abs((hi.astype(np.float32) + lo.astype(np.float32)) / np.float32(2) - np.float32(128))
    cost = (hi - lo).astype(np.int32) + centre.astype(np.int32)
    best = cand[np.argmin(cost, axis=1)]                  # the first minimum
    rollings = (best.astype(np.float32) / np.float32(256) * np.float32(width)).astype(np.int64)
    empty = np.setdiff1d(np.arange(num_images), pairs[:, 0])
    rollings[empty] = 0
    return rollings, int(empty.size)


def center_rollings_integer(image_of_atom, x_of_atom, num_images, width, angular_res):
    """The integer restatement the kernels compute: a 256-bit occupancy set per image, rotated by every candidate."""
    img, x = np.asarray(image_of_atom, dtype=np.int64), np.asarray(x_of_atom, dtype=np.int64)
    occ = np.zeros((num_images, 256), dtype=bool)
    occ[img, (x * 256) // width] = True
    step = 256 // angular_res
    out = np.zeros(num_images, dtype=np.int64)
    empty = 0
    for i in range(num_images):
        cols = np.flatnonzero(occ[i])
        if cols.size == 0:
            empty += 1
            continue
        best = None
        for k, r in enumerate(range(0, 256, step)):
            rolled = (cols + r) % 256
            lo, hi = int(rolled.min()), int(rolled.max())
            key = ((hi - lo) + (abs(hi + lo - 256) >> 1), k)
            best = key if best is None or key < best else best
        out[i] = (best[1] * step * width) >> 8
    return out, empty


def roll_pixels_reference(images, atom_ptr, pixels, rollings, width):
    """``update_rollings``' mapping half (:610-621) on a copy of ``pixels`` (int16 [P, 2])."""
    out = np.array(pixels, copy=True)
    roll = np.asarray(rollings, dtype=np.int64)[view_images_of_atoms(images, atom_ptr)]
    out[:, 0] = ((out[:, 0].astype(np.int64) + roll) % width).astype(out.dtype)
    return out


class DenseCoverage:
    """The reference's dense matrix: ``unseen[i, p]`` = global image ``i`` sees point ``p`` and no picked image does.
    ``items``: ``(pointers, images, num_images)`` per setting over the same ``num_points`` points."""

    def __init__(self, items, num_points):
        total = sum(int(k) for _, _, k in items)
        self.unseen = np.zeros((total, num_points), dtype=bool)
        first = 0
        for pointers, images, k in items:
            pointers = np.asarray(pointers, dtype=np.int64)
            pts = np.repeat(np.arange(pointers.size - 1), np.diff(pointers))
            self.unseen[np.asarray(images, dtype=np.int64) + first, pts] = True
            first += int(k)

    def step(self, pick=-1):
        if pick >= 0:
            self.unseen &= ~self.unseen[pick]
        return self.unseen.sum(axis=1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------
# small mappings
# ---------------------------------------------------------------------------------------------------------------

def mapping_from_views(num_points, views):
    """``views``: list of (point, image, [x, ...]) in any order -> (pointers, images, atom_ptr, pixels int16 [P, 2]) with
    the views of a point in the order given, y = 0."""
    views = sorted(views, key=lambda v: v[0])
    counts = np.zeros(num_points, dtype=np.int64)
    for p, _, _ in views:
        counts[p] += 1
    pointers = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    images = np.array([v[1] for v in views], dtype=np.int64)
    atom_ptr = np.concatenate([[0], np.cumsum([len(v[2]) for v in views])]).astype(np.int64)
    xs = np.array([x for v in views for x in v[2]], dtype=np.int16)
    pixels = np.stack([xs, np.zeros_like(xs)], axis=1).reshape(-1, 2)
    return pointers, images, atom_ptr, pixels


def random_mapping(rng, num_points, num_images, width, height=8, max_views=5, max_atoms=4, p_view=0.7, span=None):
    """A random mapping with distinct (point, image) pairs; the columns of image i sit in a window of ``span`` columns
    (the whole width without it) that may wrap around the seam."""
    views = []
    start = rng.integers(0, width, num_images)
    for p in range(num_points):
        if rng.random() > p_view:
            continue
        k = int(rng.integers(1, min(max_views, num_images) + 1))
        for i in rng.choice(num_images, size=k, replace=False):
            n = int(rng.integers(0, max_atoms + 1))
            s = width if span is None else min(span, width)
            xs = (start[i] + rng.integers(0, s, n)) % width
            views.append((p, int(i), [int(x) for x in xs]))
    pointers, images, atom_ptr, pixels = mapping_from_views(num_points, views)
    pixels[:, 1] = rng.integers(0, height, pixels.shape[0])
    return pointers, images, atom_ptr, pixels
