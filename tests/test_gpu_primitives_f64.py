"""-m gpu: the CSR segment primitives (csrc/segment.hip) and the weighted row BatchNorm (csrc/rowbn.hip) against the
float64 references of tests/primitives_ref.py, on every branch their dispatchers can take.

Gates: ``tolerances.gate`` for fp32 storage, the half-ulp rule for bf16 / fp16 storage (one round-to-nearest-even of an
fp32 result), ``torch.equal`` for what is exact.  ``Report.hold`` picks the rule from the storage type; ``-s`` prints
every measured error next to its gate.  All float64 work runs on the CPU.

Branches and the case that reaches each (caps as in the launchers):

segment.hip  ``vec_ok``: C % 4 (fp32) / C % 8 (16-bit) and 16-byte aligned pointers -> 16-byte kernels, else scalar.
  SEG_C has both sides of C % 4 and C % 8; ``test_segment_misaligned_*`` makes the pointer half false;
  ``grid_for`` caps the grid at 8192 blocks x 256 threads: ``test_segment_grid_stride`` wraps it, scalar and vector.
  ``dva_gather_csr``: 16-byte copy when the row is a multiple of 16 bytes and aligned, else 4- / 2-byte moves.
rowbn.hip  ``rv_ok``: C % VEC == 0, C / VEC a power of two <= 256, aligned -> vector kernels, else scalar.
  ROWBN_C: C / VEC = 1 (256 rows per block, every shuffle step), 16, 32 (last shuffle width), 64 / 128 / 256 (LDS
  atomics only), 512 (> 256: scalar), 3 (not a power of two: scalar), C % VEC != 0 (scalar), C = 4096 (largest).
  Per-sweep capacities: scalar statistics 2048 blocks x 4 rows, vector statistics 512 blocks x (256 / (C / VEC)) rows
  x 4 rows in flight, apply kernels 4096 blocks x 256 threads: ``test_rowbn_multi_sweep`` wraps each with a partial
  last sweep.  ``test_rowbn_misaligned`` makes the pointer half of ``rv_ok`` false at a vector width.
"""
import functools

import pytest
import torch

import primitives_ref as P
import tolerances as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
REDUCES = ["sum", "mean", "max", "min"]
SEG_C = [1, 3, 4, 8, 12, 64, 130, 136]
SEG_GRID_CAP = 8192 * 256            # grid_for(): 256 * 32 blocks of 256 threads, grid-stride beyond
INF = float("inf")


def dname(dtype):
    return {F32: "fp32", BF16: "bf16", F16: "fp16"}[dtype]


def seg_vec(dtype):
    return 4 if dtype == F32 else 8


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def misaligned(t):
    """A contiguous copy of ``t`` that starts one element into a flat buffer: its pointer is no multiple of 16."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
    return v


# ----------------------------------------------------------------------------------------------
# segments
# ----------------------------------------------------------------------------------------------
SEG_INF_GROUPS = (6, 10)      # 2 and 4 rows


@functools.lru_cache(maxsize=None)
def seg_ptr():
    """Ragged CSR: 25 % empty groups (the first and the last among them), groups of 1 and 2 rows, one of 5000 rows."""
    gen = torch.Generator().manual_seed(11)
    n = 240
    sizes = torch.randint(1, 10, (n,), generator=gen)
    sizes[torch.rand(n, generator=gen) < 0.25] = 0
    for g, s in ((0, 0), (3, 5000), (5, 1), (6, 2), (7, 0), (8, 1), (10, 4), (n - 2, 2), (n - 1, 0)):
        sizes[g] = s
    assert 0.15 < float((sizes == 0).float().mean()) < 0.35
    return torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])


@functools.lru_cache(maxsize=None)
def seg_data(C, kind):
    """fp32 master data [M, C] and output gradient [n, C] (multiples of 1/4: exact in every storage type)."""
    ptr = seg_ptr()
    gen = torch.Generator().manual_seed(100 * C + (kind == "ints"))
    M, n = int(ptr[-1]), ptr.shape[0] - 1
    if kind == "randn":
        x = torch.randn(M, C, generator=gen)
    else:       # integers in [-3, 3]: almost every max / min ties, sums are exact in fp32
        x = torch.randint(-3, 4, (M, C), generator=gen).float()
    w = torch.randint(-8, 9, (n, C), generator=gen).float() / 4
    return x, w


def seg_src(C, kind, reduce, dtype):
    """The stored source of a case: +-inf rows such that a group is all -inf for max, all +inf for min (the arg is its
    first row), and holds one +inf row for sum / mean (the sum is +inf)."""
    x = seg_data(C, kind)[0].clone()
    ptr = seg_ptr()
    for g in SEG_INF_GROUPS:
        b, e = int(ptr[g]), int(ptr[g + 1])
        if reduce == "max":
            x[b:e] = -INF
        elif reduce == "min":
            x[b:e] = INF
        else:
            x[b + 1] = INF
    return x.to(dtype)


def check_segment(rep, case, src, ptr, w, reduce, src_dev=None):
    """Forward, arg and backward of one (source, reduce) against float64; returns the device tensors."""
    from deepviewagg_amd import ops
    dtype = src.dtype
    s_dev = (src.to(DEV) if src_dev is None else src_dev).requires_grad_()
    p_dev = ptr.to(DEV)
    out = ops.segment_csr(s_dev, p_dev, reduce=reduce)
    (gsrc,) = torch.autograd.grad(out, s_dev, grad_outputs=w.to(dtype).to(DEV))
    ref64, arg64 = P.segment_ref(src, ptr, reduce)
    if reduce in ("sum", "mean"):
        ref32, _ = P.segment_ref(src, ptr, reduce, torch.float32)
        rep.hold(case, "out", "out", out, ref64, ref32)
        g64 = P.segment_grad_ref(w, ptr, reduce, None, src.shape[0])
        g32 = P.segment_grad_ref(w, ptr, reduce, None, src.shape[0], torch.float32)
        rep.hold(case, "grad_src", "grad_in", gsrc, g64, g32)
    else:
        # exact: the value is a copy of a stored element, the arg the first row attaining it, and the gradient goes
        # to that row only
        assert torch.equal(out.detach().cpu(), ref64.to(dtype)), (case, "values")
        vals, arg = ops.segment_csr_arg(s_dev, p_dev, reduce)
        assert torch.equal(arg.cpu().long(), arg64), (case, "arg")
        assert torch.equal(bits(vals), bits(out)), (case, "segment_csr_arg values")
        g64 = P.segment_grad_ref(w, ptr, reduce, arg64, src.shape[0])
        assert torch.equal(gsrc.cpu(), g64.to(dtype)), (case, "grad_src")
    return out.detach(), gsrc


@pytest.mark.parametrize("C", SEG_C)
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_segment_csr_f64(dtype, reduce, C):
    """16-byte kernels where C % seg_vec(dtype) == 0 (fp32: 4, 8, 12, 64, 136; 16-bit: 8, 64, 136), scalar kernels
    elsewhere; random data and tie-heavy integer data, empty groups, groups of 1 / 2 / 5000 rows, +-inf groups."""
    rep = P.Report(f"segment_csr {dname(dtype)} {reduce} C={C}")
    ptr = seg_ptr()
    for kind in ("randn", "ints"):
        src = seg_src(C, kind, reduce, dtype)
        out, _ = check_segment(rep, kind, src, ptr, seg_data(C, kind)[1], reduce)
        for g in SEG_INF_GROUPS:
            want = {"sum": INF, "mean": INF, "max": -INF, "min": INF}[reduce]
            assert bool((out[g].float() == want).all()), (kind, g)
    rep.check()


@pytest.mark.parametrize("C", SEG_C)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_gather_csr_f64(dtype, C):
    """gather_csr (16-byte copy when the row is a multiple of 16 bytes -- fp32 C % 4 == 0, 16-bit C % 8 == 0 -- else
    the 4- / 2-byte copy), its backward (a segment sum) and segment_gather_csr."""
    from deepviewagg_amd import ops
    rep = P.Report(f"gather_csr {dname(dtype)} C={C}")
    ptr = seg_ptr()
    p_dev = ptr.to(DEV)
    x, w = seg_data(C, "randn")
    grp = w.to(dtype)                                       # group-level rows
    g_dev = grp.to(DEV).requires_grad_()
    out = ops.gather_csr(g_dev, p_dev)
    assert torch.equal(bits(out), bits(P.gather_ref(grp, ptr)))
    gout = (torch.round(x * 4) / 4).to(dtype)               # exact in every storage type
    (gg,) = torch.autograd.grad(out, g_dev, grad_outputs=gout.to(DEV))
    rep.hold("backward", "grad_groups", "grad_in", gg, P.segment_ref(gout, ptr, "sum")[0],
             P.segment_ref(gout, ptr, "sum", torch.float32)[0])
    src = x.to(dtype)
    for reduce in REDUCES:
        sg = ops.segment_gather_csr(src.to(DEV), p_dev, reduce=reduce)
        seg = ops.segment_csr(src.to(DEV), p_dev, reduce=reduce)
        assert sg.shape == src.shape and torch.equal(bits(sg), bits(P.gather_ref(seg.cpu(), ptr))), reduce
        ref64 = P.gather_ref(P.segment_ref(src, ptr, reduce)[0], ptr)
        if reduce in ("max", "min"):
            assert torch.equal(sg.cpu(), ref64.to(dtype)), reduce
        else:
            rep.hold(reduce, "segment_gather_csr", "out", sg, ref64,
                     P.gather_ref(P.segment_ref(src, ptr, reduce, torch.float32)[0], ptr))
    rep.check()


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_segment_misaligned_bit_identical(dtype, reduce):
    """The pointer half of ``vec_ok``: C % 8 == 0, but a tensor starts one element past a 16-byte boundary, so the
    launcher must take the scalar kernels.  Both kernels add a channel's rows in the same order: bit-identical."""
    from deepviewagg_amd import _lib
    from deepviewagg_amd import ops
    from deepviewagg_amd._lib import check, dtype_code, ptr as dptr, stream_of
    lib = _lib.load()
    code = _lib.REDUCE_CODE[reduce]
    ptr = seg_ptr()
    p_dev = ptr.to(DEV)
    n = ptr.shape[0] - 1
    for C in (8, 64):
        for kind in ("randn", "ints"):
            src = seg_src(C, kind, reduce, dtype).to(DEV)
            w = seg_data(C, kind)[1].to(dtype).to(DEV)
            M = src.shape[0]
            s_al = src.clone().requires_grad_()
            out_al = ops.segment_csr(s_al, p_dev, reduce=reduce)                    # aligned: 16-byte kernels
            (g_al,) = torch.autograd.grad(out_al, s_al, grad_outputs=w)
            arg_al = ops.segment_csr_arg(src, p_dev, reduce)[1] if code >= _lib.DVA_MAX else None
            # misaligned source through ops (the output is a fresh, aligned tensor)
            s_mis = misaligned(src).requires_grad_()
            out_1 = ops.segment_csr(s_mis, p_dev, reduce=reduce)
            assert torch.equal(bits(out_1), bits(out_al)), (C, kind, "misaligned src")
            if arg_al is not None:
                assert torch.equal(ops.segment_csr_arg(s_mis, p_dev, reduce)[1], arg_al)
            # misaligned output: ops cannot produce one, the C entry can
            out_buf = misaligned(torch.zeros_like(out_al))
            arg_2 = torch.empty((n, C), dtype=torch.int32, device=DEV) if arg_al is not None else None
            check(lib.dva_segment_csr_fwd(dptr(src), dptr(p_dev), dptr(out_buf), dptr(arg_2), n, C, dtype_code(src),
                                          code, stream_of(src)), "dva_segment_csr_fwd")
            assert torch.equal(bits(out_buf), bits(out_al)), (C, kind, "misaligned out")
            if arg_al is not None:
                assert torch.equal(arg_2, arg_al)
            # backward: misaligned grad_out, then misaligned grad_src
            for which in ("grad_out", "grad_src"):
                go = misaligned(w) if which == "grad_out" else w
                gs = torch.zeros((M, C), dtype=dtype, device=DEV)
                if which == "grad_src":
                    gs = misaligned(gs)
                check(lib.dva_segment_csr_bwd(dptr(go), dptr(p_dev), dptr(arg_al), dptr(gs), n, C, dtype_code(src),
                                              code, stream_of(src)), "dva_segment_csr_bwd")
                assert torch.equal(bits(gs), bits(g_al)), (C, kind, "misaligned " + which)
            # gather_csr: misaligned source / destination take the 2- / 4-byte copy
            ga = ops.gather_csr(w, p_dev)
            assert torch.equal(bits(ops.gather_csr(misaligned(w), p_dev)), bits(ga))
            dst = misaligned(torch.zeros_like(ga))
            check(lib.dva_gather_csr(dptr(w), dptr(p_dev), dptr(dst), n, C, dtype_code(w), stream_of(w)),
                  "dva_gather_csr")
            assert torch.equal(bits(dst), bits(ga))


@pytest.mark.parametrize("dtype,C,n,max_size", [(F32, 5, 450_000, 3), (BF16, 8, 2_200_000, 2)],
                         ids=["scalar-fp32-C5", "vector-bf16-C8"])
def test_segment_grid_stride(dtype, C, n, max_size):
    """``grid_for`` caps the grid at 8192 blocks of 256 threads; beyond that the kernels' grid-stride loops must take
    further turns.  Scalar kernels: one thread per (group, channel), C = 5 is no multiple of 4.  Vector kernels: one
    thread per (group, 8 channels) of bf16."""
    from deepviewagg_amd import ops
    vec = C % seg_vec(dtype) == 0
    threads_per_group = C // seg_vec(dtype) if vec else C
    assert n * threads_per_group > SEG_GRID_CAP           # the case wraps the 8192 x 256 cap
    gen = torch.Generator().manual_seed(C)
    sizes = torch.randint(0, max_size + 1, (n,), generator=gen)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    M = int(ptr[-1])
    src = torch.randint(-40, 41, (M, C), generator=gen).float().div_(8).to(dtype)     # ties in max / min now and then
    w = torch.randint(-8, 9, (n, C), generator=gen).float() / 4
    s_dev = src.to(DEV)
    rep = P.Report(f"segment grid-stride {dname(dtype)} C={C} n={n}")
    for reduce in REDUCES:
        check_segment(rep, reduce, src, ptr, w, reduce, src_dev=s_dev.clone())
    grp = w.to(dtype)
    assert torch.equal(bits(ops.gather_csr(grp.to(DEV), ptr.to(DEV), n_rows=M)), bits(P.gather_ref(grp, ptr)))
    rep.check()


SOFTMAX_SIZES = [1, 2, 33, 300, 0, 0, 5, 1, 0, 2, 33, 7, 0, 300, 12, 1]


def softmax_case(G, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.cat([torch.tensor(SOFTMAX_SIZES), torch.randint(0, 13, (40,), generator=gen)])
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    V = int(ptr[-1])
    return ptr, torch.randn(V, G, generator=gen) * 2 * scale, torch.randn(V, G, generator=gen)


def check_softmax(rep, case, src, ptr, w, eps, scaling, hold_grad=True):
    from deepviewagg_amd import ops
    s_dev = src.to(DEV).requires_grad_()
    out = ops.segment_softmax_csr(s_dev, ptr.to(DEV), eps=eps, scaling=scaling)
    assert out.dtype == src.dtype and bool(torch.isfinite(out.float()).all())
    (grad,) = torch.autograd.grad(out, s_dev, grad_outputs=w.to(src.dtype).to(DEV))
    o64, g64 = P.softmax_ref(src, ptr, eps, scaling, w.to(src.dtype))
    o32, g32 = P.softmax_ref(src, ptr, eps, scaling, w.to(src.dtype), torch.float32)
    rep.hold(case, "out", "out", out, o64, o32)
    assert bool(torch.isfinite(grad.float()).all())
    if hold_grad:     # (the 16-bit entry casts around the fp32 kernel: its gradient is one rounding of the fp32 one)
        rep.hold(case, "grad_src", "grad_in", grad, g64, g32)
    return out


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("G", [1, 3, 4, 8])
def test_segment_softmax_f64(G, scaling):
    """Segments of 1, 2, 33 and 300 rows and empty groups, forward and gradient, ``eps`` small and large.  At
    eps = 1e-2 the gradient through the group max (the reference differentiates through it, pooling.py:787) is some
    per cent of the whole: a backward that holds the max constant misses the gate there."""
    rep = P.Report(f"segment_softmax_csr G={G} scaling={scaling}")
    ptr, src, w = softmax_case(G, 7 * G + scaling)
    for eps in (1e-12, 1e-2):
        check_softmax(rep, f"eps={eps:g}", src, ptr, w, eps, scaling)
    rep.check()


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "scaled"])
def test_segment_softmax_large_scores(scaling):
    """Scores of magnitude 1e4: centring on the group max keeps every exponent <= 0, the output is finite and meets
    the gate (the differences of fp32 scores this large are exact where their exponential is not zero).  The
    attention is one-hot to 1e-12 here and its gradient is zero in exact arithmetic: a plain fp32 evaluation has
    nothing but rounding noise in it, so the gradient is held to be finite only."""
    rep = P.Report(f"segment_softmax_csr scores x 1e4 scaling={scaling}")
    ptr, src, w = softmax_case(4, 3, scale=1e4)
    assert float(src.abs().max()) > 5e4
    check_softmax(rep, "x1e4", src, ptr, w, 1e-12, scaling, hold_grad=False)
    rep.check()


@pytest.mark.parametrize("dtype", [BF16, F16], ids=dname)
def test_segment_softmax_16bit(dtype):
    """16-bit scores through ops.segment_softmax_csr: the same storage type back, one rounding of the fp32 result."""
    rep = P.Report(f"segment_softmax_csr {dname(dtype)}")
    for G, scaling in ((1, False), (4, True), (8, False)):
        ptr, src, w = softmax_case(G, 5 + G)
        check_softmax(rep, f"G={G} scaling={scaling}", src.to(dtype), ptr, w, 1e-12, scaling)
    rep.check()


# ----------------------------------------------------------------------------------------------
# row BatchNorm
# ----------------------------------------------------------------------------------------------
ROWBN_C = {F32: [3, 4, 12, 64, 128, 256, 512, 1024, 2048], BF16: [8, 20, 24, 64, 256, 512, 2048],
           F16: [8, 20, 24, 64, 256, 512, 2048]}
ROWBN_STATS_SCALAR_ROWS = 2048 * 4          # rows_grid(): 256 * 8 blocks x RB_ROWS
ROWBN_STATS_VEC_BLOCKS = 512                # dva_rowbn_stats: 256 * 2 blocks, rpb rows each, four rows in flight
ROWBN_APPLY_THREADS = 4096 * 256            # elems_grid(): 256 * 16 blocks of 256 threads
EPS = 1e-5


def rowbn_vec(dtype, C):
    """``rv_ok`` for aligned tensors: the threads per row of the vector kernels, or 0 for the scalar kernels."""
    vec = 4 if dtype == F32 else 8
    cpr = C // vec
    return cpr if (C % vec == 0 and 1 <= cpr <= 256 and cpr & (cpr - 1) == 0) else 0


def rowbn_case(R, C, dtype, seed, with_counts, shift=0.5):
    gen = torch.Generator().manual_seed(seed)
    counts = None
    if with_counts:
        counts = torch.randint(0, 5, (R,), generator=gen, dtype=torch.int32)
        counts[:3] = torch.tensor([2, 1, 3], dtype=torch.int32)[:R]       # never a batch of no views
    y = (torch.randn(R, C, generator=gen) * 1.5 + shift).to(dtype)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.5
    gview = torch.randint(-32, 33, (R, C), generator=gen).float() / 8    # x counts <= 4: exact in every storage type
    running = (torch.randn(C, generator=gen) * 0.3 + shift, torch.rand(C, generator=gen) * 2 + 0.5)
    return y, counts, gamma, beta, gview, running


def run_rowbn(y, counts, gamma, beta, gview, slope, running, misalign=False):
    """ops.rowbn_sums -> ops.bn_table -> ops.rowbn_act and its backward, as batchnorm_act_rows strings them."""
    from deepviewagg_amd import ops
    R, C = y.shape
    bn = torch.nn.BatchNorm1d(C, eps=EPS, affine=gamma is not None).to(DEV)
    if gamma is not None:
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
    y_dev = (misaligned(y.to(DEV)) if misalign else y.to(DEV)).requires_grad_()
    c_dev = counts.to(DEV) if counts is not None else None
    cnt = torch.ones(R) if counts is None else counts.float()
    n = float(cnt.sum())
    sums = None
    if running is None:
        bn.train()
        sums = ops.rowbn_sums(y_dev.detach(), c_dev)
        tab = ops.bn_table(sums, n, bn, True)
    else:
        bn.eval()
        with torch.no_grad():
            bn.running_mean.copy_(running[0])
            bn.running_var.copy_(running[1])
        tab = ops.bn_table(None, 1.0, bn, False)
    out = ops.rowbn_act(y_dev, c_dev, bn.weight if bn.affine else None, bn.bias if bn.affine else None, None, None,
                        n if running is None else 1.0, running is None, slope, bn_tab=tab)
    # the loss over the views, sum_v out_v gview_v: a row's gradient is counts x its view gradient
    gout = (gview * cnt.view(-1, 1)).to(y.dtype).to(DEV)
    grads = torch.autograd.grad(out, [y_dev] + ([bn.weight, bn.bias] if bn.affine else []), grad_outputs=gout)
    return dict(sums=None if sums is None else sums.clone(), n=n, out=out.detach(), dy=grads[0],
                dgamma=grads[1] if bn.affine else None, dbeta=grads[2] if bn.affine else None)


def hold_sums(rep, case, got, r64, r32):
    C = r64["mean"].shape[0]
    mean = got["sums"][:C].cpu() / got["n"]
    var = got["sums"][C:].cpu() / got["n"] - mean * mean
    em, ev = T.bn_errors(mean, var, r64["mean"], r64["var"])
    em32, ev32 = T.bn_errors(r32["mean"], r32["var"], r64["mean"], r64["var"])
    rep.add(case, "batch mean", "bn_mean", em, em32)
    rep.add(case, "batch var", "bn_var", ev, ev32)


def hold_raw_sums(rep, case, got, y, counts):
    idx, _ = P.view_index(y.shape[0], counts)
    C = y.shape[1]
    for name, p in (("sum w y", 1), ("sum w y^2", 2)):
        s = got["sums"][(p - 1) * C:p * C].cpu()
        rep.add(case, name, "out", T.rel_err(s, (y.double()[idx] ** p).sum(0)),
                T.rel_err((y.float()[idx] ** p).sum(0), (y.double()[idx] ** p).sum(0)))


def check_rowbn(rep, case, y, counts, gamma, beta, gview, slope, running, one_row=False, misalign=False):
    """One (case, variant) against ``nn.BatchNorm1d`` in double over the repeated rows.

    ``one_row`` (R = 1 with batch statistics): every view is the same row and the batch variance is zero, so the
    statistics are held as raw sums (an error in units of a zero standard deviation means nothing).  Without counts
    it is a batch of one, which torch refuses: only the sums are held here, the rule by ``test_rowbn_one_row``.  With
    counts = [2] the reference exists: out = leaky(beta), and dy / dgamma are zero in exact arithmetic, differences of
    terms of the size of gamma gout / sqrt(eps) and of dbeta, against which they are measured."""
    got = run_rowbn(y, counts, gamma, beta, gview, slope, running, misalign)
    if one_row:
        hold_raw_sums(rep, case, got, y, counts)
        if counts is None:
            return
    r32f = P.rowbn_ref(y, counts, gamma, beta, slope, None, running, EPS, dtype=torch.float32)
    r64 = P.rowbn_ref(y, counts, gamma, beta, slope, gview, running, EPS, out_got=got["out"], z32=r32f["z"])
    r32 = P.rowbn_ref(y, counts, gamma, beta, slope, gview, running, EPS, side=r64["side"], dtype=torch.float32)
    rep.n_kink = getattr(rep, "n_kink", 0) + (r64["n_kink"] if slope != 1.0 else 0)
    if running is None and not one_row:
        hold_sums(rep, case, got, r64, r32)
    dy_scale = dg_scale = None
    if one_row:
        cnt = counts.double().view(-1, 1)
        dy_scale = gview.double() * cnt * (gamma.double() if gamma is not None else 1.0) / EPS ** 0.5
        dg_scale = r64.get("dbeta")
    rep.hold(case, "out", "out", got["out"], r64["out"], r32["out"])
    rep.hold(case, "dy", "grad_in", got["dy"], r64["dy"], r32["dy"], dy_scale)
    if gamma is not None:
        rep.hold(case, "dgamma", "grad_param", got["dgamma"], r64["dgamma"], r32["dgamma"], dg_scale)
        rep.hold(case, "dbeta", "grad_param", got["dbeta"], r64["dbeta"], r32["dbeta"])


def kink_note(rep):
    rep.notes.append(f"{getattr(rep, 'n_kink', 0)} elements inside the LeakyReLU kink window (side taken from the run)")


ROWBN_WIDTHS = [(d, C) for d in DTYPES for C in ROWBN_C[d]]


@pytest.mark.parametrize("dtype,C", ROWBN_WIDTHS, ids=[f"{dname(d)}-C{C}" for d, C in ROWBN_WIDTHS])
def test_rowbn_f64(dtype, C):
    """Every width of the dispatch (module docstring) at R = 1, 3, 777: counts in 0..4 and None, slope 0.2 / 0 (ReLU)
    / 1 (no activation), batch and given (running) statistics, with and without affine parameters."""
    rep = P.Report(f"rowbn {dname(dtype)} C={C} ({'vector, C/VEC=%d' % rowbn_vec(dtype, C) if rowbn_vec(dtype, C) else 'scalar'})")
    for R in (1, 3, 777):
        for with_counts in (True, False):
            y, counts, gamma, beta, gview, running = rowbn_case(R, C, dtype, 1000 * R + C, with_counts)
            for slope in (0.2, 0.0, 1.0):
                for given in (False, True):
                    case = f"R={R} {'counts' if with_counts else 'ones'} slope={slope:g} {'given' if given else 'batch'}"
                    check_rowbn(rep, case, y, counts, gamma, beta, gview, slope, running if given else None,
                                one_row=(R == 1 and not given))
            if R > 1:
                check_rowbn(rep, f"R={R} {'counts' if with_counts else 'ones'} no affine", y, counts, None, None,
                            gview, 0.2, None)
    kink_note(rep)
    rep.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_rowbn_misaligned(dtype):
    """The pointer half of ``rv_ok``: C = 64 is a vector width for every type, but ``y`` starts one element past a
    16-byte boundary, so all four passes must take the scalar kernels (statistics and apply, forward and backward;
    ``y`` is an operand of each).  Held against float64 like every other case."""
    rep = P.Report(f"rowbn {dname(dtype)} C=64, misaligned y")
    assert rowbn_vec(dtype, 64)
    for with_counts in (True, False):
        y, counts, gamma, beta, gview, running = rowbn_case(777, 64, dtype, 64 + with_counts, with_counts)
        for given in (False, True):
            check_rowbn(rep, f"{'counts' if with_counts else 'ones'} {'given' if given else 'batch'}", y, counts,
                        gamma, beta, gview, 0.2, running if given else None, misalign=True)
    kink_note(rep)
    rep.check()


ROWBN_SWEEPS = [
    # dtype, C, R, counts, the apply kernels wrap too
    (F32, 64, 70_003, True, True),       # vector, shuffle reduction (C/VEC = 16): 32768 rows per sweep
    (F32, 12, 90_001, True, True),       # scalar (C/VEC = 3): 8192 rows per sweep
    (F32, 1024, 5_003, True, True),      # vector, no shuffles (C/VEC = 256): 2048 rows per sweep
    (F32, 4, 600_001, True, False),      # vector, C/VEC = 1: 524288 rows per sweep
    (BF16, 512, 9_001, True, False),     # vector, no shuffles (C/VEC = 64): 8192 rows per sweep
    (F16, 20, 9_001, True, False),       # scalar 16-bit: 8192 rows per sweep
    (BF16, 64, 140_001, False, True),    # vector 16-bit apply kernels beyond 1048576 threads (C/VEC = 8)
]


@pytest.mark.parametrize("dtype,C,R,with_counts,apply_wraps", ROWBN_SWEEPS,
                         ids=[f"{dname(d)}-C{C}-R{R}" for d, C, R, _, _ in ROWBN_SWEEPS])
def test_rowbn_multi_sweep(dtype, C, R, with_counts, apply_wraps):
    """More rows than one sweep of the grid holds, the last sweep partial (the ``ok`` mask of the four rows in flight
    in the vector statistics kernel, the row loop of the scalar one, the grid-stride loop of the apply kernels)."""
    cpr = rowbn_vec(dtype, C)
    sweep = ROWBN_STATS_VEC_BLOCKS * (256 // cpr) * 4 if cpr else ROWBN_STATS_SCALAR_ROWS
    assert R > sweep and R % sweep != 0                    # statistics: more than one sweep, the last one partial
    if cpr:
        assert (R % sweep) % (sweep // 4) != 0             # ... and ends inside one of its four row groups
    threads = R * (cpr if cpr else C)
    assert (threads > ROWBN_APPLY_THREADS) == apply_wraps  # apply kernels: the 4096 x 256 cap
    rep = P.Report(f"rowbn multi-sweep {dname(dtype)} C={C} R={R}")
    y, counts, gamma, beta, gview, running = rowbn_case(R, C, dtype, R + C, with_counts)
    check_rowbn(rep, "batch slope=0.2", y, counts, gamma, beta, gview, 0.2, None)
    rep.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_rowbn_widest(dtype):
    """C = 4096, the largest width the statistics entries accept (scalar kernels, 64 KiB of LDS), at R = 37; C = 4097
    is refused before any launch."""
    from deepviewagg_amd import _lib
    from deepviewagg_amd._lib import dtype_code, ptr as dptr, stream_of
    rep = P.Report(f"rowbn {dname(dtype)} C=4096")
    y, counts, gamma, beta, gview, running = rowbn_case(37, 4096, dtype, 4096, True)
    check_rowbn(rep, "R=37 batch", y, counts, gamma, beta, gview, 0.2, None)
    check_rowbn(rep, "R=37 given", y, None, gamma, beta, gview, 0.0, running)
    rep.check()
    wide = torch.zeros((2, 4097), dtype=dtype, device=DEV)
    sums = torch.zeros(2 * 4097, dtype=torch.float64, device=DEV)
    rc = _lib.load().dva_rowbn_stats(dptr(wide), None, dptr(sums), 2, 4097, dtype_code(wide), stream_of(wide))
    assert _lib._ERRORS[rc].startswith("DVA_ERR_INVALID")
    assert float(sums.abs().sum()) == 0.0


@pytest.mark.parametrize("dtype,C", [(F32, 64), (F32, 12), (F32, 1024), (BF16, 64), (F16, 64), (F16, 24)],
                         ids=["fp32-vec-shuffle", "fp32-scalar", "fp32-vec-lds", "bf16-vec", "fp16-vec", "fp16-scalar"])
def test_rowbn_sums_cancellation(dtype, C):
    """y = 100 + randn: the variance is E[y^2] - mean^2 with |mean| = 100 standard deviations, the cancellation the
    kernel's own comment names (fp64 sums)."""
    from deepviewagg_amd import ops
    rep = P.Report(f"rowbn sums, y = 100 + randn, {dname(dtype)} C={C}")
    for with_counts in (True, False):
        R = 777
        gen = torch.Generator().manual_seed(C + with_counts)
        counts = torch.randint(0, 5, (R,), generator=gen, dtype=torch.int32) if with_counts else None
        y = (100 + torch.randn(R, C, generator=gen)).to(dtype)
        sums = ops.rowbn_sums(y.to(DEV), counts.to(DEV) if with_counts else None)
        r64 = P.rowbn_ref(y, counts, None, None, 1.0)
        r32 = P.rowbn_ref(y, counts, None, None, 1.0, dtype=torch.float32)
        hold_sums(rep, "counts" if with_counts else "ones", dict(sums=sums, n=r64["n"]), r64, r32)
    rep.check()


# ----------------------------------------------------------------------------------------------
# BatchNorm bookkeeping: bn_table / batchnorm_act_rows against nn.BatchNorm1d in double
# ----------------------------------------------------------------------------------------------
def twin_modules(C, affine, track, momentum, seed):
    gen = torch.Generator().manual_seed(seed)
    mods = []
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.5
    rm, rv = torch.randn(C, generator=gen) * 0.3, torch.rand(C, generator=gen) + 0.5
    for dtype, dev in ((torch.float32, DEV), (torch.float64, "cpu"), (torch.float32, "cpu")):
        bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=momentum, affine=affine, track_running_stats=track)
        with torch.no_grad():
            if affine:
                bn.weight.copy_(gamma)
                bn.bias.copy_(beta)
            if track:
                bn.running_mean.copy_(rm)
                bn.running_var.copy_(rv)
        mods.append(bn.to(dtype).to(dev))
    return mods


@pytest.mark.parametrize("momentum", [0.1, None], ids=["momentum0.1", "cumulative"])
@pytest.mark.parametrize("track", [True, False], ids=["track", "notrack"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_batchnorm_bookkeeping(train, track, momentum):
    """train / eval x affine x track_running_stats x momentum 0.1 / None (cumulative average: the generic branch of
    batchnorm_act_rows) x counts / None, two consecutive calls: output, running_mean, running_var (unbiased) and
    num_batches_tracked as nn.BatchNorm1d keeps them over the repeated rows."""
    from deepviewagg_amd.modules.multimodal.pooling import batchnorm_act_rows
    rep = P.Report(f"BatchNorm bookkeeping train={train} track={track} momentum={momentum}")
    R, C, slope = 61, 16, 0.2
    for affine in (True, False):
        for with_counts in (True, False):
            dev, b64, b32 = twin_modules(C, affine, track, momentum, 17)
            for m in (dev, b64, b32):
                m.train(train)
            for call in (1, 2):
                y, counts, *_ = rowbn_case(R, C, F32, 50 * call + affine, with_counts, shift=call)
                idx, cnt = P.view_index(R, counts)
                with torch.no_grad():
                    out = batchnorm_act_rows(y.to(DEV), dev, slope, counts.to(DEV) if with_counts else None,
                                             float(cnt.sum()))
                    o64 = torch.nn.functional.leaky_relu(b64(y.double()[idx]), slope)
                    o32 = torch.nn.functional.leaky_relu(b32(y[idx]), slope)
                first = (cnt.cumsum(0) - cnt)[cnt > 0]
                case = f"affine={affine} {'counts' if with_counts else 'ones'} call {call}"
                rep.hold(case, "out", "out", out[(cnt > 0).to(DEV)], o64[first], o32[first])
                if track:
                    rep.hold(case, "running_mean", "out", dev.running_mean, b64.running_mean, b32.running_mean)
                    rep.hold(case, "running_var", "out", dev.running_var, b64.running_var, b32.running_var)
                    assert torch.equal(dev.num_batches_tracked.cpu(), b64.num_batches_tracked), case
                    assert int(b64.num_batches_tracked) == (call if train else 0)
                else:
                    assert dev.running_mean is None and dev.num_batches_tracked is None
    rep.check()


@pytest.mark.parametrize("C", [24, 64], ids=["scalar-C24", "vector-C64"])
@pytest.mark.parametrize("momentum", [0.1, None], ids=["momentum0.1", "cumulative"])
def test_rowbn_one_row(momentum, C):
    """A batch of one row (n = 1).  nn.BatchNorm1d refuses it in training mode; the project's rule: the batch variance
    is 0, the unbiased factor n / (n - 1) is taken as 1, so running_var moves towards 0 by the momentum, running_mean
    towards the row, and the output is leaky(beta)."""
    from deepviewagg_amd.modules.multimodal.pooling import batchnorm_act_rows
    rep = P.Report(f"rowbn n = 1, momentum={momentum}")
    slope = 0.2
    for with_counts in (False, True):
        dev, b64, b32 = twin_modules(C, True, True, momentum, 23)
        y = rowbn_case(1, C, F32, 5, False)[0]
        counts = torch.ones(1, dtype=torch.int32, device=DEV) if with_counts else None
        with torch.no_grad():
            out = batchnorm_act_rows(y.to(DEV), dev.train(), slope, counts, 1.0)
        m = 1.0 if momentum is None else momentum          # cumulative average after the first batch: 1 / 1
        case = "counts=[1]" if with_counts else "counts=None"
        # b64 / b32 are never called: they hold the initial buffers and parameters in float64 / fp32
        want = {"out": torch.nn.functional.leaky_relu(b64.bias.detach(), slope).view(1, C),
                "running_mean": (1 - m) * b64.running_mean + m * y.double()[0],
                "running_var": (1 - m) * b64.running_var + m * 0.0 * 1.0}         # variance 0 x factor 1
        w32 = {"out": torch.nn.functional.leaky_relu(b32.bias.detach(), slope).view(1, C),
               "running_mean": (1 - m) * b32.running_mean + m * y[0],
               "running_var": (1 - m) * b32.running_var}
        rep.hold(case, "out", "out", out, want["out"], w32["out"])
        rep.hold(case, "running_mean", "out", dev.running_mean, want["running_mean"], w32["running_mean"])
        rep.hold(case, "running_var", "out", dev.running_var, want["running_var"], w32["running_var"])
        assert int(dev.num_batches_tracked) == 1
    rep.check()
