"""Float64 references of the view-attention kernels (csrc/attention.hip) and the cases the GPU tests run them on.
Plain Python, imported by name like ``primitives_ref.py``; ``tests/test_attention_ref_host.py`` holds it to the oracle
and asserts the input conditions of every case on the CPU, ``tests/test_gpu_attention_f64.py`` holds the kernels to it.

The references are written from the reference project's expressions (pooling.py:284-300 the tail, :758-810 the segment
softmax, :748-755 + :737-745 the channel groups, :690-715 ``Gating`` = ``tanh(relu(max * w + b))``), not from the
kernels.  Every function takes ``dtype``: ``torch.float64`` is the reference, ``torch.float32`` the plain torch
evaluation of the same case whose own error may raise a gate (``tolerances.gate``).  Inputs are always the *stored*
tensors (bf16 / fp16 are cast up exactly).

Semantics of the tail, as the reference project has them:

* an empty segment gives a zero output row, a zero group max (so its gate is ``tanh(relu(b))``) and no argmax (-1);
* ``scaling`` divides by sqrt(segment size) AFTER centring on the group max;
* ``eps`` sits in the denominator ``sum + eps``; the group max stays in the graph (it is a ``segment_csr(.., 'max')``
  the reference differentiates through), so its first row also receives the gate's gradient;
* ties of the max go to the FIRST row of the segment;
* channel c belongs to the group ``group_sizes(C, G)`` puts it in (C = 7, G = 2: 4 + 3 channels).

The ReLU of the gate has a kink at a zero pre-activation: an entry whose float64 pre-activation lies within
``FP32_HEADROOM`` x the measured ``|pre32 - pre64|`` may legitimately fall on either side in fp32, so it takes its side
from the run under test (``gate > 0``), as ``primitives_ref.kink_side`` does for LeakyReLU; their number is reported.
"""
import functools

import torch

import tolerances as T
from oracle import pooling_oracle as O

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPE_CODE = {F32: 0, BF16: 1, F16: 2}       # DVA_F32 / DVA_BF16 / DVA_F16
SPECIALISED = ((8, 8), (16, 4), (8, 4), (16, 2))     # compiled (lpr, rows) instances; any other team pair is run-time


def vec_of(dtype):
    return 4 if dtype == F32 else 8


def group_index(C, G):
    """Group of every channel (pooling.py:737-755: ``expand_group_feat`` over ``group_sizes``)."""
    if G == 1:
        return torch.zeros(C, dtype=torch.long)
    if G >= C:
        return torch.arange(C)
    return torch.repeat_interleave(torch.arange(G), O.group_sizes(C, G))


# ----------------------------------------------------------------------------------------------
# the tail
# ----------------------------------------------------------------------------------------------
def tail_ref(rows, row_idx, compat, ptr, gate_w, gate_b, scaling, w, eps=1e-12, side=None, dtype=torch.float64):
    """pooling.py:284-300 on ``val = rows[row_idx]`` (``row_idx`` None: ``val = rows``), and by autograd the gradients
    of ``(out * w).sum()``.  ``side`` [N, G] bool: the side of the ReLU kink every gate entry is evaluated and
    differentiated on (None: ``relu``'s own).  Returns a dict: out [N, C], att [V, G], gate [N, G] (ones without
    gating), arg [N, G] (first row of the group max, -1 for empty segments), pre [N, G] (None without gating),
    grad_rows (w.r.t. ``rows``), grad_val (w.r.t. the gathered ``val``), grad_compat, grad_gate_w, grad_gate_b."""
    N, (V, G), C = ptr.shape[0] - 1, compat.shape, rows.shape[1]
    x = rows.detach().to(dtype).requires_grad_()
    val = x if row_idx is None else x[row_idx.long()]
    c = compat.detach().to(dtype).requires_grad_()
    idx = O.dense_index(ptr)
    sizes = ptr[1:] - ptr[:-1]
    gidx = group_index(C, G)
    # segment_csr(compat, 'max'): the first row attaining it, 0 for empty segments, part of the graph
    arg = O.segment_arg_fast(c.detach(), ptr, "max")
    c0 = torch.cat([c, torch.zeros((1, G), dtype=dtype)])
    mx = c0.gather(0, torch.where(arg < 0, torch.full_like(arg, V), arg))
    centered = c - mx[idx]
    if scaling:
        centered = centered / sizes.to(dtype).sqrt()[idx].view(-1, 1)
    e = centered.exp()
    att = e / (torch.zeros((N, G), dtype=dtype).index_add(0, idx, e) + eps)[idx]
    out = torch.zeros((N, C), dtype=dtype).index_add(0, idx, val * att[:, gidx])
    gating = gate_w is not None
    pre, params = None, []
    gate = torch.ones((N, G), dtype=dtype)
    if gating:
        gw = gate_w.detach().to(dtype).reshape(1, G).requires_grad_()
        gb = gate_b.detach().to(dtype).reshape(1, G).requires_grad_()
        params = [gw, gb]
        pre = mx * gw + gb
        gate = torch.tanh(torch.relu(pre) if side is None else torch.where(side, pre, torch.zeros_like(pre)))
        out = out * gate[:, gidx]
    res = dict(out=out.detach(), att=att.detach(), gate=gate.detach(), arg=arg,
               pre=None if pre is None else pre.detach())
    if w is not None:
        ins = [x, c] + ([val] if row_idx is not None else []) + params
        grads = list(torch.autograd.grad((out * w.detach().to(dtype)).sum(), ins))
        res["grad_rows"], res["grad_compat"] = grads[0], grads[1]
        res["grad_val"] = grads[2] if row_idx is not None else grads[0]
        if gating:
            res["grad_gate_w"], res["grad_gate_b"] = grads[-2].reshape(-1), grads[-1].reshape(-1)
    return res


def kink_window(pre32, pre64):
    """Half-width of the window around a zero pre-activation inside which fp32 may take either ReLU side."""
    return T.FP32_HEADROOM * float((pre32.double() - pre64).abs().max())


def kink_side(pre64, gate_got, window):
    """(side [N, G] with the entries inside the window taken from the run under test, their number)."""
    near = pre64.abs() <= window
    return torch.where(near, gate_got.detach().cpu().double() > 0, pre64 > 0), int(near.sum())


# ----------------------------------------------------------------------------------------------
# segmented sums over a row plan
# ----------------------------------------------------------------------------------------------
def make_records(att, gate, view_point, rs):
    """The fp32 view records of ``dva_view_gather_attention_bwd``: [point (int32 bits) | gate * attention per group |
    padding] of stride ``rs``; the product is the fp32 one the kernel stores."""
    V, G = att.shape
    rec = torch.zeros((V, rs), dtype=torch.float32)
    rec[:, 0] = view_point.to(torch.int32).view(torch.float32)
    g = torch.ones_like(att) if gate is None else gate[view_point.long()]
    rec[:, 1:1 + G] = att * g
    return rec


def rows_grad_ref(gout, row_idx, n_rows, C, G, att=None, gate=None, view_point=None, rec=None, dtype=torch.float64):
    """``dva_view_gather_rows_grad``: grows[r] = sum over the views v of row r of gout[p_v] * att[v, g] * gate[p_v, g]
    (from ``att`` / ``gate`` / ``view_point``, or from the stored records)."""
    gidx = group_index(C, G)
    if rec is not None:
        p = rec[:, 0].contiguous().view(torch.int32).long()
        s = rec[:, 1:1 + G].to(dtype)
    else:
        p = view_point.long()
        s = att.to(dtype) * (gate.to(dtype)[p] if gate is not None else 1.0)
    contrib = gout.detach().to(dtype)[p] * s[:, gidx]
    return torch.zeros((n_rows, C), dtype=dtype).index_add(0, row_idx.long(), contrib)


def rows_sum_ref(gout, row_idx, n_rows, weights=None, atom_shift=0, dtype=torch.float64):
    """``dva_gather_rows_sum``: grows[r] = sum over the entries e of row r of weights[e] * gout[e >> atom_shift]."""
    e = torch.arange(row_idx.shape[0])
    contrib = gout.detach().to(dtype)[e >> atom_shift]
    if weights is not None:
        contrib = contrib * weights.to(dtype).view(-1, 1)
    return torch.zeros((n_rows, gout.shape[1]), dtype=dtype).index_add(0, row_idx.long(), contrib)


def anchor_rows_sum_ref(gout, anchors, n_anchors, weights, dtype=torch.float64):
    """``dva_anchor_rows_sum``: S[a][k] = sum over the views v of anchor a of weights[v][k] * gout[v]."""
    contrib = weights.to(dtype).unsqueeze(2) * gout.detach().to(dtype).unsqueeze(1)          # [V, 4, C]
    return torch.zeros((n_anchors, 4, gout.shape[1]), dtype=dtype).index_add(0, anchors.long(), contrib)


# ----------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------
def team_consts(dtype, lpr, rows):
    """(U, cap) of the backward team kernel: the register path holds ``U * rows`` views, the LDS-parked path of the
    gather form ``cap / G`` (1024 floats per wavefront, shared by its 64 / ts teams)."""
    U = 8 if (lpr, rows) == (16, 4) and dtype == F32 else 4
    return U, 1024 * lpr * rows // 64


def geometry_of(lib, dtype, C, G, N, V):
    """(team, lpr, rows) from the library's own rule (host only, no device)."""
    import ctypes
    lpr, rows = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = lib.dva_view_attention_geometry(C, G, N, V, DTYPE_CODE[dtype], ctypes.byref(lpr), ctypes.byref(rows))
    assert rc in (0, 1), rc
    return rc, lpr.value, rows.value


# name -> dtype, C, G, (lpr, rows) or None = generic, gating, scaling, filler segments are randint(0, fill + 1), the
# average the padding stops at (None: 60 fillers, the special segments dominate), algo, integer-valued compat
def _case(dtype, C, G, geom, gating, scaling, fill, avg=None, algo=0, ints=False, n_grid=0):
    return dict(dtype=dtype, C=C, G=G, geom=geom, gating=gating, scaling=scaling, fill=fill, avg=avg, algo=algo, ints=ints,
                n_grid=n_grid)


CASES = {
    # compiled geometries: G takes 1, 2, 4, 8; every geometry meets scaling on and off, gating on and off
    "f32-8x8": _case(F32, 32, 1, (8, 8), True, True, 9),
    "bf16-8x8": _case(BF16, 64, 8, (8, 8), True, False, 9),
    "f16-8x8": _case(F16, 64, 2, (8, 8), False, True, 9),
    "f32-8x4": _case(F32, 32, 2, (8, 4), False, False, 5, avg=4.4),
    "bf16-8x4": _case(BF16, 64, 4, (8, 4), True, True, 5, avg=4.4),
    "f16-8x4": _case(F16, 64, 8, (8, 4), True, False, 5, avg=4.4),
    "f32-16x4": _case(F32, 64, 4, (16, 4), True, True, 9),
    "bf16-16x4": _case(BF16, 128, 2, (16, 4), False, False, 9),
    "f32-16x2": _case(F32, 64, 8, (16, 2), True, False, 3, avg=2.3),
    "bf16-16x2": _case(BF16, 128, 1, (16, 2), False, True, 3, avg=2.3),
    # the run-time geometry
    "f32-rt-4x16": _case(F32, 16, 1, (4, 16), True, True, 9),
    "f32-rt-32x2-G32": _case(F32, 128, 32, (32, 2), True, False, 9),
    "bf16-rt-64x1": _case(BF16, 512, 4, (64, 1), True, True, 5),
    "bf16-rt-8x2": _case(BF16, 64, 4, (8, 2), False, True, 3, avg=2.3),
    # the generic kernels
    "f32-gen-C7": _case(F32, 7, 2, None, True, True, 9),
    "f32-gen-C20": _case(F32, 20, 5, None, False, False, 9),
    "f32-gen-algo1": _case(F32, 64, 4, None, True, True, 9, algo=1),
    "bf16-gen-C12": _case(BF16, 12, 4, None, True, False, 9),
    # ties: integer compat in {-2 .. 2}
    "f32-16x4-ties": _case(F32, 64, 4, (16, 4), True, True, 5, ints=True),
    "f32-gen-C20-ties": _case(F32, 20, 5, None, True, True, 5, ints=True),
    # more than one sweep of the capped grid (4096 blocks of 256 / ts points): the two-step prefetch of the last sweep
    # runs past N.  Segments of 0 .. 4 views; the bf16 case adds long segments until the average passes 5.33, which
    # the <8, 8> instance needs
    "f32-16x4-grid": _case(F32, 64, 4, (16, 4), True, True, 4, n_grid=4096 * 4 + 3),
    "bf16-8x8-grid": _case(BF16, 64, 4, (8, 8), True, False, 4, n_grid=4096 * 4 + 3),
}
TEAM_CASES = [k for k, c in CASES.items() if c["geom"] is not None]
GENERIC_CASES = [k for k, c in CASES.items() if c["geom"] is None]


def special_sizes(case):
    """The segment lengths at the boundaries of the backward team kernel's three paths (register / LDS / round trip)."""
    if case["geom"] is None:
        return [0, 1, 16, 17, 300]
    U, cap = team_consts(case["dtype"], *case["geom"])
    rows, G = case["geom"][1], case["G"]
    return [0, 1, U * rows, U * rows + 1, cap // G, cap // G + 1, max(300, cap // G + 40)]


def case_sizes(name):
    case = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if case["n_grid"]:
        n = case["n_grid"]
        sizes = torch.multinomial(torch.tensor([1.0, 1.0, 2.0, 4.0, 6.0]), n, replacement=True, generator=gen)
        if case["geom"] == (8, 8):
            where = torch.randperm(n - 2, generator=gen)[:64] + 1
            sizes[where] = 700
        sizes[0] = sizes[-1] = 0
        return sizes
    special = special_sizes(case)
    fill = lambda k: torch.randint(0, case["fill"] + 1, (k,), generator=gen)
    sizes = torch.cat([torch.tensor(special), fill(60)])
    if case["avg"] is not None:
        while float(sizes.sum()) / sizes.shape[0] > case["avg"]:
            sizes = torch.cat([sizes, fill(20)])
    sizes = sizes[torch.randperm(sizes.shape[0], generator=gen)]
    return torch.cat([torch.zeros(1, dtype=torch.long), sizes, torch.zeros(1, dtype=torch.long)])   # empty first and last


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The stored tensors of a case, on the CPU, from a fixed seed: ptr [N + 1], rows [R, C] and row_idx int32 [V]
    (``val = rows[row_idx]`` is the materialised form), compat fp32 [V, G], gate_w / gate_b [1, G] or None, and the
    output gradient w [N, C] (multiples of 1/4: exact in every storage type)."""
    case = CASES[name]
    dtype, C, G = case["dtype"], case["C"], case["G"]
    sizes = case_sizes(name)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    N, V = sizes.shape[0], int(ptr[-1])
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    R = max(8, V // 3)
    rows = torch.randn(R, C, generator=gen).to(dtype)
    row_idx = torch.randint(0, R, (V,), generator=gen).int()
    if case["ints"]:
        compat = torch.randint(-2, 3, (V, G), generator=gen).float()
    else:
        compat = torch.randn(V, G, generator=gen) * 2
    w = torch.randint(-8, 9, (N, C), generator=gen).float() / 4
    gw = gb = None
    if case["gating"]:
        # the gate's weight and bias put the kink inside the distribution of the group max, so that both ReLU sides
        # are populated: the threshold of a group is the midpoint between two neighbouring values of its max (empty
        # segments: 0) that splits the points most evenly -- from the inputs alone
        arg = O.segment_arg_fast(compat, ptr, "max")
        mx = torch.cat([compat, torch.zeros(1, G)]).gather(0, torch.where(arg < 0, torch.full_like(arg, V), arg))
        gw = (0.5 + torch.rand(1, G, generator=gen)) * (torch.randint(0, 2, (1, G), generator=gen) * 2 - 1).float()
        thr = torch.zeros(1, G)
        for g in range(G):
            u, cnt = torch.unique(mx[:, g], return_counts=True)
            below = cnt.cumsum(0)[:-1].float() / N
            k = int(torch.minimum(below, 1 - below).argmax())
            thr[0, g] = (u[k] + u[k + 1]) / 2
        gb = -gw * thr
    return dict(case, name=name, ptr=ptr, sizes=sizes, N=N, V=V, R=R, rows=rows, row_idx=row_idx, val=rows[row_idx.long()],
                compat=compat, gate_w=gw, gate_b=gb, w=w)


@functools.lru_cache(maxsize=None)
def reference(name, form):
    """(float64 reference, plain fp32 twin, kink window) of a case with ReLU's own sides; ``form`` is "val" (the
    materialised [V, C] values) or "gather" (``rows[row_idx]``)."""
    d = make_case(name)
    args = ((d["rows"], d["row_idx"]) if form == "gather" else (d["val"], None)) + (
        d["compat"], d["ptr"], d["gate_w"], d["gate_b"], d["scaling"], d["w"])
    r32 = tail_ref(*args, dtype=torch.float32)
    r64 = tail_ref(*args, dtype=torch.float64)
    window = kink_window(r32["pre"], r64["pre"]) if d["gating"] else 0.0
    return r64, r32, window


def reference_for(name, form, gate_got):
    """The pair of ``reference`` with the gate entries inside the kink window evaluated on the side the run under
    test took, and the number of such entries."""
    d = make_case(name)
    r64, r32, window = reference(name, form)
    if not d["gating"]:
        return r64, r32, 0
    side, n_kink = kink_side(r64["pre"], gate_got, window)
    if torch.equal(side, r64["pre"] > 0) and torch.equal(side, r32["pre"] > 0):
        return r64, r32, n_kink
    args = ((d["rows"], d["row_idx"]) if form == "gather" else (d["val"], None)) + (
        d["compat"], d["ptr"], d["gate_w"], d["gate_b"], d["scaling"], d["w"])
    return (tail_ref(*args, side=side, dtype=torch.float64), tail_ref(*args, side=side, dtype=torch.float32), n_kink)


# ----------------------------------------------------------------------------------------------
# row plans of the segmented sums
# ----------------------------------------------------------------------------------------------
def plan_rows(populations, n_rows, seed):
    """A row index whose rows have the given populations (the first ``len(populations)`` rows, shuffled over all
    ``n_rows`` rows; every other row gets 0 or 1 entries), entries in random order."""
    gen = torch.Generator().manual_seed(seed)
    counts = (torch.rand(n_rows, generator=gen) < 0.5).long()
    where = torch.randperm(n_rows, generator=gen)[:len(populations)]
    counts[where] = torch.tensor(populations)
    idx = torch.repeat_interleave(torch.arange(n_rows), counts)
    return idx[torch.randperm(idx.shape[0], generator=gen)].int(), counts
