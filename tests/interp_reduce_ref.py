"""References and the shared case generator of the fused bilinear gather + max / mean / sum / min pool
(csrc/interp_reduce.hip).  Plain Python, imported by name like ``gather_reduce_ref.py``.

* ``taps_ref``: the taps of the bilinear gather as include/dva.h states them (q = coord * (H, W) + 0.5 in the 1-padded map,
  4 taps floor(q), floor(q + 1), weights |prod(q - opposite)|, padded index i -> clamp(i - 1)), in fp32.
* ``forward_ref``: a numpy restatement of the forward contract of ``dva_interp_segment_reduce_fwd``, written from the
  header text and not from the kernel: the item value ((w0 x0 + w1 x1) + w2 x2) + w3 x3 with every product and sum rounded
  to fp32 on its own, rounded once to the storage type; on those values fp32 accumulation from 0 in item order, the mean
  divides once by the fp32 count, one rounding, empty segments give 0, max / min take the first item on ties (a NaN wins
  only as the first item) and keep the uint16 offset of the winner, 0xffff for none.
* ``forward_f64`` / ``backward_f64``: the same pool and its gradient w.r.t. the stacked map rows in float64.
* ``make_case``: the maps, coordinates and segments every test of this feature shares (see its docstring).
"""
import numpy as np
import torch

from gather_reduce_ref import round_to, stored, segment_sizes      # noqa: F401  (re-exported for the tests)

GEOMETRY = [(2, 4, 6), (1, 5, 3)]              # (maps, H, W) of the two settings: 48 + 15 = 63 stacked map rows
ROW_OFFSET = [0, 48]
R_ROWS = 63
# map rows no tap touches: (y 2, x 3) of both maps of the first setting, (y 1, x 1) of the second
COLD_ROWS = (15, 39, 52)
HOT_HITS = 320                                  # items on one cell: map 0 of the first setting, rows 0-1, columns 4-5
HOT_COORDS = [(0.3, 0.8), (0.3125, 0.8125), (0.3, 0.8), (0.34375, 0.796875)]     # (cy, cx); one of them twice: ties
IRREGULAR_CY = 0.125 - 2.0 ** -26               # H = 4: q = 1 - 2^-24, floor(q) = 0 and floor(q + 1) = 2 in fp32
N_IRREGULAR = 3
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # half an ulp at 1


def taps_ref(images, coords, H, W):
    """(tap rows int64 [P, 4] numbered inside the setting, tap weights fp32 [P, 4], regular bool [P]) in the tap order
    top-left, top-right, bottom-left, bottom-right.  ``coords`` fp32 [P, 2] = (y, x) in [0, 1]."""
    f = np.float32
    c = np.asarray(coords, dtype=f)
    qy = (c[:, 0] * f(H)).astype(f) + f(0.5)
    qx = (c[:, 1] * f(W)).astype(f) + f(0.5)
    top, bottom = np.floor(qy), np.floor((qy + f(1)).astype(f))
    left, right = np.floor(qx), np.floor((qx + f(1)).astype(f))
    w = np.stack([np.abs(((qy - bottom).astype(f) * (qx - right).astype(f)).astype(f)),
                  np.abs(((qy - bottom).astype(f) * (qx - left).astype(f)).astype(f)),
                  np.abs(((qy - top).astype(f) * (qx - right).astype(f)).astype(f)),
                  np.abs(((qy - top).astype(f) * (qx - left).astype(f)).astype(f))], 1).astype(f)
    clamp = lambda v, n: np.clip(v.astype(np.int64) - 1, 0, n - 1)
    it, ib, il, ir = clamp(top, H), clamp(bottom, H), clamp(left, W), clamp(right, W)
    base = np.asarray(images, dtype=np.int64) * H
    rows = np.stack([(base + it) * W + il, (base + it) * W + ir, (base + ib) * W + il, (base + ib) * W + ir], 1)
    regular = (bottom == top + 1) & (right == left + 1) & (top >= 0) & (left >= 0) & (top <= H) & (left <= W)
    return rows, w, regular


def item_values(rows, tap_rows, tap_weights, dtype):
    """fp32 [P, C]: what the [P, C] tensor of the materialised gather holds (products and sums rounded one by one)."""
    f = np.float32
    rows = np.asarray(rows, dtype=f)
    t, w = np.asarray(tap_rows, dtype=np.int64), np.asarray(tap_weights, dtype=f)
    if t.shape[0] == 0:
        return np.zeros((0, rows.shape[1]), dtype=f)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = (w[:, 0:1] * rows[t[:, 0]]).astype(f)
        for k in (1, 2, 3):
            acc = (acc + (w[:, k:k + 1] * rows[t[:, k]]).astype(f)).astype(f)
    return round_to(acc, dtype)


def forward_ref(rows, tap_rows, tap_weights, ptr, reduce, dtype):
    """(out fp32 values of the stored result [S, C], arg uint16 [S, C] or None).  ``rows`` fp32 numpy holding the stored
    values of the stacked map rows."""
    v = item_values(rows, tap_rows, tap_weights, dtype)
    S, C = len(ptr) - 1, np.asarray(rows).shape[1]
    out = np.zeros((S, C), dtype=np.float32)
    extremum = reduce in ("max", "min")
    arg = np.full((S, C), 0xffff, dtype=np.uint16) if extremum else None
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            beg, end = int(ptr[s]), int(ptr[s + 1])
            acc = np.zeros(C, dtype=np.float32)
            for a in range(beg, end):
                if extremum:
                    better = ((v[a] > acc) if reduce == "max" else (v[a] < acc)) if a > beg else np.ones(C, dtype=bool)
                    acc = np.where(better, v[a], acc)
                    arg[s] = np.where(better, np.uint16(a - beg), arg[s])
                else:
                    acc = (acc + v[a]).astype(np.float32)
            if reduce == "mean" and end > beg:
                acc = (acc / np.float32(end - beg)).astype(np.float32)
            out[s] = acc
    return round_to(out, dtype), arg


def winners(arg, ptr):
    """int64 [S, C]: the winning ITEM of every (segment, channel) from the uint16 offsets, -1 for none."""
    a = np.asarray(arg).astype(np.int64)
    return np.where(a == 0xffff, -1, a + np.asarray(ptr, dtype=np.int64)[:-1, None])


def forward_f64(rows, tap_rows, tap_weights, ptr, reduce):
    """(out float64 [S, C], arg int64 [S, C] = winning ITEM, -1 for none; None for sum / mean), and the per-element
    magnitude ``scale`` float64 [S, C] a rounding bound refers to: the sum (mean: the mean, max / min: the maximum) over the
    segment's items of sum_k |w_k x_k|."""
    r = np.asarray(rows, dtype=np.float64)
    t, w = np.asarray(tap_rows, dtype=np.int64), np.asarray(tap_weights, dtype=np.float64)
    C = r.shape[1]
    x = np.zeros((t.shape[0], C))
    mag = np.zeros((t.shape[0], C))
    for k in range(4):
        x += w[:, k:k + 1] * r[t[:, k]]
        mag += np.abs(w[:, k:k + 1] * r[t[:, k]])
    S = len(ptr) - 1
    out, scale = np.zeros((S, C)), np.zeros((S, C))
    arg = np.full((S, C), -1, dtype=np.int64) if reduce in ("max", "min") else None
    for s in range(S):
        beg, end = int(ptr[s]), int(ptr[s + 1])
        if end <= beg:
            continue
        seg = x[beg:end]
        if reduce == "sum":
            out[s], scale[s] = seg.sum(0), mag[beg:end].sum(0)
        elif reduce == "mean":
            out[s], scale[s] = seg.sum(0) / (end - beg), mag[beg:end].sum(0) / (end - beg)
        else:
            k = seg.argmax(0) if reduce == "max" else seg.argmin(0)       # numpy: the first occurrence
            arg[s] = beg + k
            out[s], scale[s] = seg[k, np.arange(C)], mag[beg:end].max(0)
    return out, arg, scale


def backward_f64(gout, tap_rows, tap_weights, ptr, reduce, arg, n_rows):
    """float64 [R, C]: gradient of ``(forward(rows) * gout).sum()`` w.r.t. the stacked map rows, every tap of every item
    summed (the taps of the irregular views among them); ``arg`` = winning items of the forward that is being
    differentiated (max / min)."""
    g = np.asarray(gout, dtype=np.float64)
    t, w = np.asarray(tap_rows, dtype=np.int64), np.asarray(tap_weights, dtype=np.float64)
    S, C = g.shape
    gitem = np.zeros((t.shape[0], C))
    for s in range(S):
        beg, end = int(ptr[s]), int(ptr[s + 1])
        if end <= beg:
            continue
        if reduce in ("max", "min"):
            gitem[arg[s], np.arange(C)] += g[s]
        else:
            gitem[beg:end] = g[s] / (end - beg) if reduce == "mean" else g[s]
    grows = np.zeros((n_rows, C))
    for k in range(4):
        np.add.at(grows, t[:, k], w[:, k:k + 1] * gitem)
    return grows


def case_sizes(seed):
    """``segment_sizes`` (empty segments first and last, sizes 1 and 2, one of 70, one of 300) with sixty more segments of 0
    to 10 items before the last one: about 800 items."""
    gen = torch.Generator().manual_seed(7000 + seed)
    base = segment_sizes(seed)
    return base[:-1] + torch.randint(0, 11, (60,), generator=gen).tolist() + [0]


def make_case(C, dtype, seed=0, settings=(0, 1)):
    """CPU tensors of one case over the settings ``settings`` of ``GEOMETRY`` (both: a ``cat`` with a shuffled order; one:
    a single gather).  Per item of the pooled order: its setting, map and (cy, cx), drawn so that every kind of tap block
    occurs -- interior points, points on the four borders and in the four corners (clamped taps: a row named twice or four
    times), exact pixel centres (weights 0 and 1), HOT_HITS items on one cell (a few distinct coordinates, one of them
    twice: ties), N_IRREGULAR views without the 2 x 2 structure on the 4-row setting, and COLD_ROWS touched by no tap.

    Returns ``x`` (list of [B, C, H, W] maps in ``dtype``, values on a coarse grid), ``setting`` / ``images`` / ``coords``
    per item of the pooled order, ``parts`` (per setting: the positions of its items, shuffled when there are several settings) and ``order`` (position
    in the pooled order -> index into the concatenation of the parts), ``rows`` [R, C] stacked, numpy ``tap_rows`` /
    ``tap_weights`` in the stacked numbering, ``irregular`` (positions), ``ptr``, ``gout``."""
    gen = torch.Generator().manual_seed(1000 * seed + C + 17 * len(settings))
    sizes = case_sizes(seed)
    ptr = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
    P, S = int(ptr[-1]), len(sizes)
    rnd = lambda n: torch.rand(n, generator=gen)
    pick = lambda vals, n: torch.tensor(vals)[torch.randint(0, len(vals), (n,), generator=gen)]
    setting = pick(list(settings), P)
    images = torch.zeros(P, dtype=torch.int64)
    for s in settings:
        on = setting == s
        images[on] = torch.randint(0, GEOMETRY[s][0], (int(on.sum()),), generator=gen)
    # interior points, half of them on a grid of 1 / 64 (dyadic weights)
    coords = 0.02 + 0.96 * torch.stack([rnd(P), rnd(P)], 1)
    grid = rnd(P) < 0.5
    coords[grid] = (coords[grid] * 64).round() / 64
    slots = torch.randperm(P, generator=gen).tolist()
    take = lambda n: torch.tensor([slots.pop() for _ in range(n)])
    # borders and corners
    edge = take(48)
    coords[edge[:12], 0], coords[edge[12:24], 0] = 0.0, 1.0
    coords[edge[24:36], 1], coords[edge[36:48], 1] = 0.0, 1.0
    corner = take(8)
    coords[corner] = torch.tensor([[0., 0.], [0., 1.], [1., 0.], [1., 1.]]).repeat(2, 1)
    # exact pixel centres: (k + 0.5) / size exactly representable
    centre = take(40)
    for p in centre.tolist():
        if int(setting[p]) == 0:
            coords[p] = torch.stack([pick([0.125, 0.375, 0.625, 0.875], 1)[0], pick([0.25, 0.75], 1)[0]])
        else:
            coords[p] = torch.tensor([0.5, 0.5])
    # the hot cell and the irregular views live on the first setting
    first = settings[0]
    assert first == 0, "the hot cell and the irregular views are defined on the 4 x 6 setting"
    hot = take(HOT_HITS)
    setting[hot], images[hot] = 0, 0
    coords[hot] = torch.tensor(HOT_COORDS)[torch.randint(0, len(HOT_COORDS), (HOT_HITS,), generator=gen)].float()
    irregular = take(N_IRREGULAR)
    setting[irregular] = 0
    images[irregular] = torch.randint(0, GEOMETRY[0][0], (N_IRREGULAR,), generator=gen)
    coords = coords.float()
    coords[irregular, 0] = float(np.float32(IRREGULAR_CY))
    assert float(coords[irregular[0], 0]) < 0.125, "fp32 holds 0.125 - 2^-26"

    def taps_of():
        rows4 = np.zeros((P, 4), dtype=np.int64)
        w4 = np.zeros((P, 4), dtype=np.float32)
        reg = np.ones(P, dtype=bool)
        for s in settings:
            on = (setting == s).numpy()
            _, H, W = GEOMETRY[s]
            r, w, g = taps_ref(images.numpy()[on], coords.numpy()[on], H, W)
            off = ROW_OFFSET[s] if len(settings) > 1 else 0
            rows4[on], w4[on], reg[on] = r + off, w, g
        return rows4, w4, reg
    cold = [r for r in COLD_ROWS if r < (R_ROWS if len(settings) > 1 else ROW_OFFSET[1])]
    rows4, w4, reg = taps_of()
    # items with a tap on a cold row move onto the hot cell
    bad = torch.from_numpy(np.isin(rows4, cold).any(1))
    setting[bad], images[bad] = 0, 0
    coords[bad] = torch.tensor(HOT_COORDS[0])
    rows4, w4, reg = taps_of()
    assert not np.isin(rows4, cold).any()
    assert sorted(np.nonzero(~reg)[0].tolist()) == sorted(irregular.tolist()), "exactly the planted views are irregular"
    # the maps: a coarse grid, a part of the entries with a random component
    x = []
    for s in settings:
        B, H, W = GEOMETRY[s]
        v = torch.randint(-8, 9, (B, C, H, W), generator=gen).float() / 4
        v = v + torch.randn(B, C, H, W, generator=gen) * (torch.rand(B, C, H, W, generator=gen) < 0.3)
        x.append(v.to(dtype))
    rows = torch.cat([m.permute(0, 2, 3, 1).reshape(-1, C) for m in x], 0)
    parts = []
    for s in settings:
        pos = torch.nonzero(setting == s).reshape(-1)
        parts.append(pos[torch.randperm(pos.shape[0], generator=gen)] if len(settings) > 1 else pos)
    concat = torch.cat(parts)
    order = torch.empty(P, dtype=torch.int64)
    order[concat] = torch.arange(P)
    gout = torch.randn(S, C, generator=gen).to(dtype)
    return dict(x=x, setting=setting, images=images, coords=coords, parts=parts, order=order, rows=rows,
                tap_rows=rows4, tap_weights=w4, irregular=irregular, cold=tuple(cold), ptr=ptr, gout=gout, S=S, P=P,
                R=rows.shape[0], C=C, settings=tuple(settings))
