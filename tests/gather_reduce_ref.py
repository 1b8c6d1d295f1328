"""References and the shared case generator of the fused gather + max / mean / sum / min pool (csrc/gather_reduce.hip).
Plain Python, imported by name like ``tolerances.py`` and ``primitives_ref.py``.

* ``forward_ref``: a numpy restatement of the kernel contract, written from include/dva.h and the reference's
  expressions (``segment_csr(x[idx], ptr, mode)``, pooling.py:14-71 on image.py:1285) and not from the kernels: fp32
  accumulation from 0 in item order, the mean divides once by the fp32 count, one rounding to the storage type, empty
  segments give 0, max and min take the first item on ties (a NaN wins only as the first item) and keep the uint16
  offset of the winner, 0xffff for none.
* ``forward_f64`` / ``backward_f64``: the same pool and its gradient w.r.t. the map rows in float64.
* ``make_case``: the segment sizes and row indices every test of this feature shares (see its docstring).
"""
import numpy as np
import torch

R_ROWS = 96                       # map rows of every generated case
HOT_ROW, HOT_HITS = 5, 320        # one map row gathered by >= 300 items
COLD_ROWS = (0, 17, 95)           # map rows no item gathers
NP_DTYPE = {torch.float32: np.float32, torch.float16: np.float16}
EXTREMA = ("max", "min")          # the modes that keep the offset of the winning item


def round_to(x32, dtype):
    """fp32 array rounded once (to nearest, ties to even) to ``dtype``, returned as the fp32 values of the stored bits."""
    x32 = np.asarray(x32, dtype=np.float32)
    if dtype == torch.float32:
        return x32
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).astype(np.float32)
    assert dtype == torch.bfloat16
    bits = x32.view(np.uint32).astype(np.uint64)
    rounded = ((bits + 0x7fff + ((bits >> 16) & 1)) & 0xffff0000).astype(np.uint32)
    out = rounded.view(np.float32).copy()
    nan = np.isnan(x32)
    out[nan] = np.nan
    return out


def stored(t):
    """The values a torch tensor of a storage type holds, as fp32 numpy (exact)."""
    return t.detach().float().cpu().numpy()


def forward_ref(rows, row_idx, ptr, reduce, dtype):
    """(out fp32 values of the stored result [S, C], arg uint16 [S, C] or None).  ``rows`` fp32 numpy holding the stored
    values, ``row_idx`` / ``ptr`` integer arrays."""
    rows = np.asarray(rows, dtype=np.float32)
    S, C = len(ptr) - 1, rows.shape[1]
    out = np.zeros((S, C), dtype=np.float32)
    arg = np.full((S, C), 0xffff, dtype=np.uint16) if reduce in EXTREMA else None
    for s in range(S):
        beg, end = int(ptr[s]), int(ptr[s + 1])
        acc = np.zeros(C, dtype=np.float32)
        for a in range(beg, end):
            v = rows[int(row_idx[a])]
            if reduce in EXTREMA:
                better = (v > acc if reduce == "max" else v < acc) if a > beg else np.ones(C, dtype=bool)
                acc = np.where(better, v, acc)
                arg[s] = np.where(better, np.uint16(a - beg), arg[s])
            else:
                acc = (acc + v).astype(np.float32)
        if reduce == "mean" and end > beg:
            acc = (acc / np.float32(end - beg)).astype(np.float32)
        out[s] = acc
    return round_to(out, dtype), arg


def forward_f64(rows, row_idx, ptr, reduce):
    """(out float64 [S, C], arg int64 [S, C] = winning ITEM (not offset), -1 for none; None for sum / mean)."""
    x = np.asarray(rows, dtype=np.float64)[np.asarray(row_idx, dtype=np.int64)]
    S, C = len(ptr) - 1, x.shape[1]
    out = np.zeros((S, C), dtype=np.float64)
    arg = np.full((S, C), -1, dtype=np.int64) if reduce in EXTREMA else None
    for s in range(S):
        beg, end = int(ptr[s]), int(ptr[s + 1])
        if end <= beg:
            continue
        seg = x[beg:end]
        if reduce == "sum":
            out[s] = seg.sum(0)
        elif reduce == "mean":
            out[s] = seg.sum(0) / (end - beg)
        else:
            k = seg.argmax(0) if reduce == "max" else seg.argmin(0)      # numpy: the first occurrence
            arg[s] = beg + k
            out[s] = seg[k, np.arange(C)]
    return out, arg


def backward_f64(gout, row_idx, ptr, reduce, arg, n_rows):
    """float64 [R, C]: gradient of ``(forward(rows) * gout).sum()`` w.r.t. the map rows; ``arg`` = winning items of the
    forward that is being differentiated (max / min)."""
    g = np.asarray(gout, dtype=np.float64)
    row_idx = np.asarray(row_idx, dtype=np.int64)
    S, C = g.shape
    grows = np.zeros((n_rows, C), dtype=np.float64)
    for s in range(S):
        beg, end = int(ptr[s]), int(ptr[s + 1])
        if end <= beg:
            continue
        if reduce in EXTREMA:
            np.add.at(grows, (row_idx[arg[s]], np.arange(C)), g[s])
        else:
            np.add.at(grows, row_idx[beg:end], g[s] / (end - beg) if reduce == "mean" else g[s])
    return grows


def segment_sizes(seed):
    """Sizes that every case holds: empty segments (the first and the last among them), sizes 1 and 2, one segment of
    70 items and one of 300, shuffled small ones around them."""
    gen = torch.Generator().manual_seed(seed)
    mid = torch.randint(0, 6, (40,), generator=gen).tolist()
    fixed = [1, 2, 70, 0, 300, 0, 3]
    body = fixed + mid
    order = torch.randperm(len(body), generator=gen).tolist()
    return [0] + [body[i] for i in order] + [0]


def make_case(C, dtype, seed=0):
    """CPU tensors of one case: rows [R_ROWS, C] in ``dtype`` (values on a coarse grid, so that duplicates -- ties of the
    max and the min -- occur in every segment of a few items), row_idx int32 [P] with HOT_ROW gathered by HOT_HITS items spread over
    the segments and COLD_ROWS by none, ptr int64 [S + 1], and an output gradient [S, C] in ``dtype``."""
    gen = torch.Generator().manual_seed(1000 * seed + C)
    sizes = segment_sizes(seed)
    ptr = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
    P, S = int(ptr[-1]), len(sizes)
    allowed = torch.tensor([r for r in range(R_ROWS) if r not in COLD_ROWS and r != HOT_ROW])
    row_idx = allowed[torch.randint(0, len(allowed), (P,), generator=gen)]
    hot = torch.randperm(P, generator=gen)[:HOT_HITS]
    row_idx[hot] = HOT_ROW
    rows = (torch.randint(-8, 9, (R_ROWS, C), generator=gen).float() / 4
            + torch.randn(R_ROWS, C, generator=gen) * (torch.rand(R_ROWS, C, generator=gen) < 0.5)).to(dtype)
    gout = torch.randn(S, C, generator=gen).to(dtype)
    return dict(rows=rows, row_idx=row_idx.to(torch.int32), ptr=ptr, gout=gout, S=S, P=P, R=R_ROWS, C=C)
