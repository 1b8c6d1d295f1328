"""numpy restatement of the contract of ``ops.voxel_level`` (include/dva.h, "One strided level of the voxel pyramid"),
and the coordinate cases the host and the device tests share.  tests/test_voxel_level_host.py holds the restatement to
the oracles (``sparseconv_oracle.downsample_coords`` / ``kernel_map_sorted``, ``voxel_oracle.voxel_parent_index``);
tests/test_gpu_voxel_level.py holds the device op to the restatement."""
import numpy as np

FLAG_STRIDE, FLAG_KEY = 1, 2


def voxel_level_ref(coords, ratio, in_stride):
    """dict(out_coords int32 [n_out, 4], parent int64 [n], nbr int32 [8, n_out] | None, nbr_t int32 [8, n] | None,
    flags): the unique rows of (floor(xyz / ratio) * ratio, batch) ascending (batch, z, y, x), the row of each input's
    floored coordinates among them, and -- for ratio == 2 * in_stride on multiples of in_stride -- the kernel map pair
    of the offsets {0, in_stride}^3, z fastest: with d = (c - floor(c)) / in_stride and k = (dx * 2 + dy) * 2 + dz,
    nbr_t[k, i] = parent[i], nbr[k, parent[i]] = the smallest such i, -1 elsewhere."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    n = c.shape[0]
    fl = c.copy()
    fl[:, :3] = np.floor_divide(c[:, :3], ratio) * ratio
    flags = FLAG_STRIDE if n and (c[:, :3] % in_stride != 0).any() else 0
    if n:
        span = [int(v) for v in fl.max(0) - fl.min(0) + 1]
        if span[0] * span[1] * span[2] * span[3] >= 2 ** 62:       # Python ints: no overflow
            return dict(out_coords=None, parent=None, nbr=None, nbr_t=None, flags=flags | FLAG_KEY)
    order = np.lexsort((fl[:, 0], fl[:, 1], fl[:, 2], fl[:, 3]))   # ascending (batch, z, y, x)
    srt = fl[order]
    head = np.ones(n, dtype=bool)
    head[1:] = (srt[1:] != srt[:-1]).any(1)
    parent = np.empty(n, dtype=np.int64)
    parent[order] = np.cumsum(head) - 1
    out = srt[head].astype(np.int32)
    nbr = nbr_t = None
    if ratio == 2 * in_stride and not flags & FLAG_STRIDE:
        d = (c[:, :3] - fl[:, :3]) // in_stride
        k = (d[:, 0] * 2 + d[:, 1]) * 2 + d[:, 2]
        rows = np.arange(n)
        first = np.full((8, out.shape[0]), np.iinfo(np.int64).max, dtype=np.int64)
        np.minimum.at(first, (k, parent), rows)
        nbr = np.where(first == np.iinfo(np.int64).max, -1, first).astype(np.int32)
        nbr_t = np.full((8, n), -1, dtype=np.int32)
        nbr_t[k, rows] = parent
    return dict(out_coords=out, parent=parent, nbr=nbr, nbr_t=nbr_t, flags=flags)


def _shuffled(rows, seed):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return rows[np.random.default_rng(seed).permutation(rows.shape[0])].astype(np.int32)


def random_cloud(n, span, batches, seed):
    """``n`` distinct rows with xyz in [-span, span) and ``batches`` batch ids, in random order."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((0, 4), dtype=np.int64)
    while rows.shape[0] < n:
        more = np.concatenate([rng.integers(-span, span, (2 * n + 8, 3)), rng.integers(0, batches, (2 * n + 8, 1))], 1)
        rows = np.unique(np.concatenate([rows, more]), axis=0)
    return _shuffled(rows[rng.permutation(rows.shape[0])[:n]], seed + 1)


def straddle_rows():
    """Parents along x: the first holds 4 children, the 40 after it all 8, so in sorted order the runs end at 4, 12,
    ..., and one run covers positions 60..67 (across 63 | 64) and one 252..259 (across 255 | 256)."""
    cube = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    rows = [np.concatenate([cube[:4] + [-6, -2, 4], np.zeros((4, 1), dtype=np.int64)], 1)]
    for j in range(1, 41):
        rows.append(np.concatenate([cube + [-6 + 2 * j, -2, 4], np.zeros((8, 1), dtype=np.int64)], 1))
    return np.concatenate(rows)


def unit_cases():
    """{name: int32 [n, 4]} at tensor stride 1 (scale xyz by the stride for a coarser tensor): every n at which a
    kernel takes another path (0, 1, around a wavefront, around a block, several blocks) and the contents that can go
    wrong."""
    cube = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    cases = {"n0": np.zeros((0, 4), dtype=np.int32),
             "n1_minus_one": np.array([[-1, -1, -1, 0]], dtype=np.int32)}          # -1 floors to -2
    for i, n in enumerate((63, 64, 65, 256, 257)):
        cases[f"n{n}"] = random_cloud(n, 5, 3, 10 + i)                             # dense: parents of many children
    cases["n5000"] = random_cloud(5000, 14, 3, 20)
    # every voxel alone in its parent (even coordinates at stride 1): n_out == n
    cases["sparse_n_out_is_n"] = _shuffled(_rows_with_batch(
        np.unique(np.random.default_rng(3).integers(-40, 40, (300, 3)), axis=0) * 2, 0), 4)
    cases["two_batches_same_xyz"] = _shuffled(np.concatenate(
        [_rows_with_batch(cube + [-3, 5, -1], 0), _rows_with_batch(cube + [-3, 5, -1], 2),
         _rows_with_batch(cube[:3] + [7, 7, 7], 1)]), 5)
    cases["full_parent_and_singles"] = _shuffled(np.concatenate(
        [_rows_with_batch(cube + [4, -8, 2], 0), _rows_with_batch([[-1, -1, -1], [9, 3, -5], [0, 0, 0], [21, 1, 1]], 0)]), 6)
    cases["straddle_63_and_255"] = _shuffled(straddle_rows(), 7)
    cases["one_parent"] = _shuffled(_rows_with_batch(cube[[6, 1, 3, 0, 5]] + [-2, -2, -2], 1), 8)
    return cases


def _rows_with_batch(xyz, b):
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([xyz, np.full((xyz.shape[0], 1), b, dtype=np.int64)], 1)


def level_cases():
    """[(name, coords int32 [n, 4], ratio, in_stride)]: every unit case at strides 1, 2 and 4 with ratio = 2 * stride,
    and at stride 1 with ratio 3 (coordinates and parents only)."""
    out = []
    for name, c in unit_cases().items():
        for s in (1, 2, 4):
            scaled = c.copy()
            scaled[:, :3] *= s
            out.append((f"{name}-s{s}", scaled, 2 * s, s))
        out.append((f"{name}-ratio3", c.copy(), 3, 1))
    return out
