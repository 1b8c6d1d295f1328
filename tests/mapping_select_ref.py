"""Plain numpy / Python restatement of the four mapping selections (``ImageMapping.select_points(mode='pick')``,
``select_images``, ``select_views``, ``crop``; reference core/multimodal/image.py:2029-2093, 2095-2165, 2167-2210,
2279-2342, csr.py:235-294), of the per-image statistics, and the small mappings the selection tests share.  Not a
test module.

Contract.  Output point m is source point ``point_idx[m]`` (all points in order without it).  Its views are the
source views of that point, in their order, that pass ``view_mask`` and whose image is in ``image_idx`` (new id: the
place of the image in ``image_idx``).  ``compact``: new id = rank of the image among the distinct images of all
surviving views, ``seen``.  ``crop = (W, H, offsets)``: the atoms of a view become ``pixel - offsets[image]`` in the
pixel dtype (wrapping), those outside ``[0, W) x [0, H)`` are dropped, a view without atoms is dropped, the views of a
point are ordered by image (stable), the features of a view with c atoms are ``acc = 0; acc += f`` c times,
``acc /= float32(c)``; two views of one point with the same image would be united by ``from_dense``: 'unsupported'
here.  A crop that keeps no atom at all returns the mapping with shifted pixels and nothing else changed."""
import numpy as np


def select_reference(pointers, images, atom_ptr, pixels, features, point_idx=None, view_mask=None, image_idx=None,
                     compact=False, crop=None):
    """dict(pointers, images, atom_ptr, pixels, features, seen) or dict(unsupported=True)."""
    pointers, images, atom_ptr = (np.asarray(a, dtype=np.int64) for a in (pointers, images, atom_ptr))
    pixels = np.asarray(pixels)
    feats = None if features is None else np.asarray(features)
    n = len(pointers) - 1
    points = range(n) if point_idx is None else [int(p) for p in point_idx]
    new_id = None if image_idx is None else {int(b): i for i, b in enumerate(image_idx)}
    if crop is not None:
        width, height, offsets = crop
        offsets = np.asarray(offsets).astype(pixels.dtype)
    groups, any_atom = [], False
    for p in points:
        views = []
        for v in range(pointers[p], pointers[p + 1]):
            if view_mask is not None and not view_mask[v]:
                continue
            image = int(images[v])
            if new_id is not None:
                if image not in new_id:
                    continue
                image = new_id[image]
            atoms = pixels[atom_ptr[v]:atom_ptr[v + 1]]
            if crop is not None:
                moved = atoms - offsets[image]
                inside = (moved[:, 0] >= 0) & (moved[:, 1] >= 0) & (moved[:, 0] < width) & (moved[:, 1] < height)
                atoms = moved[inside]
                if len(atoms) == 0:
                    continue
                any_atom = True
            views.append((image, v, atoms))
        if crop is not None:
            if len(set(b for b, _, _ in views)) != len(views):
                return dict(unsupported=True)
            views.sort(key=lambda r: r[0])                # stable
        groups.append(views)
    if crop is not None and not any_atom:
        image_of_atom = np.repeat(images, np.diff(atom_ptr))
        return dict(pointers=pointers, images=images, atom_ptr=atom_ptr, pixels=pixels - offsets[image_of_atom],
                    features=feats, seen=None, early=True)
    seen = None
    if compact:
        seen = np.array(sorted(set(b for views in groups for b, _, _ in views)), dtype=np.int64)
        rank = {int(b): i for i, b in enumerate(seen)}
    out_ptr, out_img, out_aptr, out_pix, out_feat = [0], [], [0], [], []
    total = 0
    for views in groups:
        for image, v, atoms in views:
            out_img.append(rank[image] if compact else image)
            out_pix.append(atoms)
            total += len(atoms)
            out_aptr.append(total)
            if feats is not None:
                if crop is None:
                    out_feat.append(feats[v])
                else:
                    f = feats[v].astype(np.float32)
                    acc = np.zeros_like(f)
                    with np.errstate(all='ignore'):
                        for _ in range(len(atoms)):
                            acc = (acc + f).astype(np.float32)
                        acc = (acc / np.float32(len(atoms))).astype(np.float32)
                    out_feat.append(acc)
        out_ptr.append(len(out_img))
    out = dict(pointers=np.array(out_ptr, dtype=np.int64), images=np.array(out_img, dtype=np.int64),
               atom_ptr=np.array(out_aptr, dtype=np.int64),
               pixels=(np.concatenate(out_pix) if out_pix else pixels[:0]).reshape(-1, 2).astype(pixels.dtype),
               features=None, seen=seen)
    if feats is not None:
        dtype = np.float32 if crop is not None else feats.dtype
        out["features"] = np.array(out_feat, dtype=dtype).reshape((len(out_img),) + feats.shape[1:])
    return out


def image_stats_reference(images, atom_ptr, pixels, num_images):
    """int64 [5, B]: atoms, x min, x max, y min, y max per image; int64 max / min for an image without atoms."""
    big = np.iinfo(np.int64)
    stats = np.zeros((5, num_images), dtype=np.int64)
    stats[1], stats[3] = big.max, big.max
    stats[2], stats[4] = big.min, big.min
    for v, b in enumerate(images):
        for x, y in pixels[atom_ptr[v]:atom_ptr[v + 1]]:
            stats[0, b] += 1
            stats[1, b], stats[2, b] = min(stats[1, b], x), max(stats[2, b], x)
            stats[3, b], stats[4, b] = min(stats[3, b], y), max(stats[4, b], y)
    return stats


# ---------------------------------------------------------------------------------------------------------------
# mappings
# ---------------------------------------------------------------------------------------------------------------

def random_mapping(seed, view_counts, num_images, atoms=(1,), n_feat=4, pix=40, sort_images=True):
    """Point i has view_counts[i] views of distinct images (ascending unless sort_images is off), view k of the
    mapping atoms[k mod len(atoms)] pixels in [0, pix)^2.  n_feat None: no features, 0: 1-D features."""
    rng = np.random.default_rng(seed)
    pointers, images, atom_ptr, pixels = [0], [], [0], []
    for k in view_counts:
        ids = rng.choice(num_images, size=k, replace=False)
        images.extend(np.sort(ids) if sort_images else ids)
        pointers.append(len(images))
    for v in range(len(images)):
        a = atoms[v % len(atoms)]
        pixels.append(rng.integers(0, pix, size=(a, 2)))
        atom_ptr.append(atom_ptr[-1] + a)
    v = len(images)
    pixels = (np.concatenate(pixels) if pixels else np.zeros((0, 2))).astype(np.int16).reshape(-1, 2)
    if n_feat is None:
        feats = None
    elif n_feat == 0:
        feats = rng.standard_normal(v).astype(np.float32)
    else:
        feats = rng.standard_normal((v, n_feat)).astype(np.float32)
    return (np.array(pointers, dtype=np.int64), np.array(images, dtype=np.int64), np.array(atom_ptr, dtype=np.int64),
            pixels, feats)


def make_case(seed, view_counts, num_images, point_idx=None, crop_size=(24, 20), **kw):
    """A mapping and one argument for each of the four methods (random unless given): ``point_idx`` with repeats in
    permuted order, a view mask that keeps about 60 %, a non-monotone ``image_idx`` that drops about a third of the
    images, and a crop whose per-image offsets keep some atoms of some views and none of others."""
    mapping = random_mapping(seed, view_counts, num_images, **kw)
    rng = np.random.default_rng(seed + 500)
    n, v = len(view_counts), len(mapping[1])
    if point_idx is None:
        point_idx = rng.integers(0, n, size=max(1, (3 * n) // 2))
    keep = max(1, (2 * num_images) // 3)
    case = dict(mapping=mapping, num_images=num_images, point_idx=np.asarray(point_idx, dtype=np.int64),
                view_mask=rng.random(v) < 0.6, image_idx=rng.permutation(num_images)[:keep].astype(np.int64))
    return with_crop(case, crop_size, seed)


def with_crop(case, crop_size=(24, 20), seed=0):
    """``crop`` wants one offset per distinct image of the mapping and indexes them by image id: ``crop_mapping`` is
    the mapping with its images renumbered to their ranks (which keeps their order), ``crop`` the size and offsets."""
    m = case["mapping"]
    present, ranks = np.unique(m[1], return_inverse=True)
    case["crop_mapping"] = (m[0], ranks.astype(np.int64).reshape(-1), m[2], m[3], m[4])
    offsets = np.random.default_rng(seed + 900).integers(0, 25, size=(len(present), 2)).astype(np.int64)
    case["crop"] = (crop_size[0], crop_size[1], offsets)
    return case


def special_features(feats):
    """NaN, -0.0, the smallest denormal and a larger one spread over the rows."""
    feats = feats.copy()
    flat = feats.reshape(-1)
    specials = np.array([np.nan, -0.0, 1e-45, -3e-39, np.inf], dtype=np.float32)
    flat[::3] = np.resize(specials, len(flat[::3]))
    return feats


def cases(tile):
    """name -> case.  The smallest shapes at which each branch of the kernels can fail (tile = the views of a point
    the crop orders in LDS)."""
    out = {}
    out["n1"] = make_case(1, [1], 1, point_idx=[0], pix=20)
    out["n1"]["crop"] = (24, 20, np.zeros((1, 2), dtype=np.int64))
    out["n1"]["view_mask"][:] = False
    out["empties"] = make_case(2, [0, 0, 3, 0, 0, 0, 2, 1, 0, 0], 5, atoms=(1, 2))
    dropped = make_case(3, [2, 0, 4, 1], 6, atoms=(1, 3))
    dropped["view_mask"][:] = False
    dropped["image_idx"] = np.array([7, 6], dtype=np.int64)
    dropped["crop"] = (24, 20, np.full_like(dropped["crop"][2], 1000))
    out["all_dropped"] = dropped
    out["views63_64_65"] = make_case(4, [63, 64, 65], 70, atoms=(1, 2))
    out["views300"] = make_case(5, [5, 300, 2], 300)
    out["views_T_plus_1"] = make_case(6, [3, tile + 1, 1], tile + 4, atoms=(2, 1), sort_images=False)
    out["atoms_0_1_2_65"] = make_case(7, [3, 1, 4, 0, 2, 5, 1], 6, atoms=(0, 1, 2, 65))
    # the mapping after a non-monotone select_images: the images of a point are no longer ascending
    base = make_case(8, [4, 0, 6, 3, 5, 1, 6], 6, atoms=(1, 2, 3))
    sel = select_reference(*base["mapping"], image_idx=np.array([4, 0, 5, 2, 1], dtype=np.int64))
    out["unsorted_images"] = make_case(8, [1], 5)
    out["unsorted_images"]["mapping"] = (sel["pointers"], sel["images"], sel["atom_ptr"], sel["pixels"], sel["features"])
    rng = np.random.default_rng(8)
    out["unsorted_images"].update(point_idx=rng.integers(0, 7, size=9).astype(np.int64),
                                  view_mask=rng.random(len(sel["images"])) < 0.6)
    with_crop(out["unsorted_images"], seed=8)
    out["image_map_perm"] = make_case(9, [7, 0, 40, 3, 12, 1], 300)
    out["pick_dup_perm"] = make_case(10, [3, 0, 2, 5, 1, 4], 7, point_idx=[5, 5, 0, 3, 1, 3, 3, 2, 0, 5, 4, 4])
    rng = np.random.default_rng(11)
    out["pick70000"] = make_case(11, rng.integers(0, 4, size=3000), 9, point_idx=rng.integers(0, 3000, size=70000),
                                 n_feat=2)
    shapes = [3, 0, 2, 5, 1, 4, 0, 6]
    for name, f in (("nofeat", None), ("feat1d", 0), ("feat1", 1), ("feat8", 8)):
        out[name] = make_case(12, shapes, 7, atoms=(1, 3, 2), n_feat=f)
    special = make_case(13, shapes, 7, atoms=(1, 3, 2, 7), n_feat=5)
    m = special["mapping"]
    special["mapping"] = m[:4] + (special_features(m[4]),)
    with_crop(special, seed=13)
    out["special_feats"] = special
    return out


def golden_mapping(g):
    return (g["in_pointers"], g["in_images"], g["in_atom_pointers"], g["in_pixels"], g["in_features"])
