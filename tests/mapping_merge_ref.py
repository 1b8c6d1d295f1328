"""Plain numpy / Python restatement of the mapping merge (``ImageMapping.select_points(mode='merge')``, reference
core/multimodal/image.py:2211-2273 followed by ``from_dense`` :1728-1795), and the small mappings the merge tests
share.  Not a test module.

Contract: point i becomes voxel idx[i], M = max(idx) + 1.  The views of voxel j are the distinct images among the views
of its points, ascending; the atoms of view (j, b) the distinct (x, y) of the source views with image b, ascending x
then y; its features f_1 .. f_c of the c source views in ascending point order, summed one after the other in fp32
and divided by float(c).  ``idx`` of the wrong length, or an id in [0, M) without a point: the mapping is returned
unchanged (None here).
"""
import numpy as np


def merge_reference(pointers, images, atom_ptr, pixels, features, idx):
    """dict(pointers, images, atom_ptr, pixels, features, c) of the merged mapping, or None where the mapping is
    returned unchanged.  ``c`` = source views per merged view."""
    pointers, images, atom_ptr, idx = (np.asarray(a, dtype=np.int64) for a in (pointers, images, atom_ptr, idx))
    pixels = np.asarray(pixels)
    n = len(pointers) - 1
    if len(idx) != n or n == 0:
        return None
    m = int(idx.max()) + 1
    if idx.min() < 0 or set(idx.tolist()) != set(range(m)):
        return None
    feats = None
    if features is not None:
        feats = np.asarray(features, dtype=np.float32).reshape(len(images), -1)
    atoms, sources = {}, {}
    for i in range(n):                                    # ascending point index
        j = int(idx[i])
        for v in range(pointers[i], pointers[i + 1]):
            a0, a1 = atom_ptr[v], atom_ptr[v + 1]
            if a1 == a0:
                continue
            key = (j, int(images[v]))
            atoms.setdefault(key, set()).update((int(x), int(y)) for x, y in pixels[a0:a1])
            sources.setdefault(key, []).append(v)
    out_ptr, out_img, out_aptr, out_pix, out_feat, out_c = [0], [], [0], [], [], []
    keys = sorted(atoms)
    k = 0
    for j in range(m):
        while k < len(keys) and keys[k][0] == j:
            key = keys[k]
            out_img.append(key[1])
            out_pix.extend(sorted(atoms[key]))
            out_aptr.append(len(out_pix))
            src = sources[key]
            out_c.append(len(src))
            if feats is not None:
                s = feats[src[0]].copy()
                for v in src[1:]:
                    s = (s + feats[v]).astype(np.float32)
                out_feat.append((s / np.float32(len(src))).astype(np.float32))
            k += 1
        out_ptr.append(len(out_img))
    out = dict(pointers=np.array(out_ptr, dtype=np.int64), images=np.array(out_img, dtype=np.int64),
               atom_ptr=np.array(out_aptr, dtype=np.int64),
               pixels=np.array(out_pix, dtype=np.int16).reshape(-1, 2), c=np.array(out_c, dtype=np.int64),
               features=None)
    if feats is not None:
        f = np.array(out_feat, dtype=np.float32).reshape(len(out_img), feats.shape[1])
        out["features"] = f.reshape(-1) if np.asarray(features).ndim == 1 else f
    return out


# ---------------------------------------------------------------------------------------------------------------
# mappings
# ---------------------------------------------------------------------------------------------------------------

def build_mapping(views, n_feat=6, seed=0):
    """``views[i]`` = list of (image, [(x, y), ...]) of point i, ascending image.  Returns (pointers, images, atom_ptr,
    pixels, features); n_feat None: no features, 0: 1-D features."""
    pointers, images, atom_ptr, pixels = [0], [], [0], []
    for vs in views:
        assert [b for b, _ in vs] == sorted(set(b for b, _ in vs)), "views of a point: ascending distinct images"
        for b, px in vs:
            images.append(b)
            pixels.extend(px)
            atom_ptr.append(len(pixels))
        pointers.append(len(images))
    rng = np.random.default_rng(seed + 1000)
    v = len(images)
    if n_feat is None:
        feats = None
    elif n_feat == 0:
        feats = rng.standard_normal(v).astype(np.float32)
    else:
        feats = rng.standard_normal((v, n_feat)).astype(np.float32)
    return (np.array(pointers, dtype=np.int64), np.array(images, dtype=np.int64), np.array(atom_ptr, dtype=np.int64),
            np.array(pixels, dtype=np.int16).reshape(-1, 2), feats)


def random_views(seed, n, image_ids, max_views, max_atoms, p_unseen=0.2, pix=40):
    """n points; a point is unseen with probability p_unseen, else sees 1 .. max_views of ``image_ids`` with
    1 .. max_atoms distinct pixels in [0, pix)^2 each (a small range: merged points share pixels)."""
    rng = np.random.default_rng(seed)
    image_ids = np.asarray(image_ids)
    views = []
    for _ in range(n):
        if rng.random() < p_unseen:
            views.append([])
            continue
        k = int(rng.integers(1, min(max_views, len(image_ids)) + 1))
        imgs = np.sort(rng.choice(image_ids, size=k, replace=False))
        vs = []
        for b in imgs:
            a = int(rng.integers(1, max_atoms + 1))
            cells = rng.choice(pix * pix, size=a, replace=False)
            vs.append((int(b), [(int(c // pix), int(c % pix)) for c in cells]))
        views.append(vs)
    return views


def random_idx(seed, n, m, sort=False):
    """n parents covering [0, m)."""
    rng = np.random.default_rng(seed + 7)
    idx = np.concatenate([np.arange(m), rng.integers(0, m, size=n - m)])
    return np.sort(idx) if sort else rng.permutation(idx)


def straddle_case(tile, seed=3):
    """Three voxels with tile - 1, tile and tile + 1 distinct atoms (4 members each, several atoms per view) among
    ordinary voxels: both routes of the kernel in one call."""
    rng = np.random.default_rng(seed)
    views, idx = [], []
    for j, total in enumerate((tile - 1, tile, tile + 1)):
        cells = rng.permutation(200 * 200)[:total]
        px = [(int(c // 200), int(c % 200)) for c in cells]
        cuts = np.sort(rng.choice(np.arange(1, total), size=11, replace=False))
        parts = [px[a:b] for a, b in zip(np.r_[0, cuts], np.r_[cuts, total])]     # 12 views, 3 per member
        for mem in range(4):
            imgs = [10 * t + mem % 2 for t in range(3)]                            # members 0, 2 and 1, 3 share images
            views.append(sorted((b, parts[3 * mem + t]) for t, b in enumerate(imgs)))
            idx.append(2 * j + 1)                                                  # voxels 1, 3, 5
    small = random_views(seed, 40, np.arange(6), 3, 5)
    views += small
    idx += [0, 2, 4, 6] + list(2 * rng.integers(0, 4, size=36))              # the three voxels keep their atom counts
    order = rng.permutation(len(views))
    return [views[o] for o in order], np.array(idx, dtype=np.int64)[order]


def cases(tile):
    """name -> (mapping arrays, idx).  The smallest shapes at which each branch of the kernel can fail."""
    out = {}
    out["n1"] = (build_mapping([[(3, [(5, 7)])]]), np.zeros(1, dtype=np.int64))
    for n in (64, 65):      # one voxel, every point sees the same 3 images, few distinct pixels: c = n, heavy dedupe
        rng = np.random.default_rng(n)
        views = [[(b, [(int(rng.integers(0, 3)), int(rng.integers(0, 3)))]) for b in (2, 5, 7)] for _ in range(n)]
        out[f"dedupe{n}"] = (build_mapping(views), np.zeros(n, dtype=np.int64))
    # voxels without views in the middle (2, 3) and at the end (8, 9); unseen points mixed with seen ones elsewhere
    views = random_views(11, 60, np.arange(5), 4, 1, p_unseen=0.3)
    idx = random_idx(11, 60, 10)
    for i in range(60):
        if idx[i] in (2, 3, 8, 9):
            views[i] = []
    out["empty_voxels"] = (build_mapping(views), idx)
    out["unseen_mixed"] = (build_mapping(random_views(12, 200, np.arange(7), 5, 3, p_unseen=0.5)),
                           random_idx(12, 200, 37))
    # the same (voxel, image) from k members: identical pixels -> one atom; different pixels -> k atoms in (x, y) order
    k = 5
    same = [[(4, [(9, 9)])] for _ in range(k)]
    diff_px = [(7, 3), (7, 1), (0, 32767), (32767, 0), (7, 2)]
    diff = [[(4, [p])] for p in diff_px]
    out["same_pixels"] = (build_mapping(same + diff), np.array([0] * k + [1] * k, dtype=np.int64))
    views, idx = straddle_case(tile)
    out["tile_straddle"] = (build_mapping(views), idx)
    out["one_image"] = (build_mapping(random_views(13, 150, np.array([0]), 1, 4, pix=6)), random_idx(13, 150, 20))
    ids = np.sort(np.random.default_rng(14).choice(100000, size=300, replace=False))
    out["images300"] = (build_mapping(random_views(14, 120, ids, 70, 2, pix=8)), random_idx(14, 120, 9))
    base = random_views(15, 300, np.arange(12), 6, 3, pix=10)
    for name, f in (("nofeat", None), ("feat1", 1), ("feat1d", 0), ("feat8", 8)):
        out[name] = (build_mapping(base, n_feat=f), random_idx(15, 300, 40))
    out["idx_sorted"] = (build_mapping(base), random_idx(15, 300, 40, sort=True))
    return out


def golden_case(g):
    return ((g["pointers"], g["images"], g["atom_pointers"], g["pixels"], g["features"]), g["merge_idx"])
