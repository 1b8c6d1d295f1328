"""Host checks of tests/primitives_ref.py: the float64 references against torch's own operators in double, ``ulp()``
against the neighbours a cast produces, the tie rule on a hand-written case, and the 16-bit gate against a plain fp32
emulation of the kernels (sequential fp32 sum in row order, rounded once): tight and attainable."""
import numpy as np
import pytest
import torch

import primitives_ref as P
import tolerances as T
from oracle import pooling_oracle as O


def ragged(n, max_size, gen, p_empty=0.25, extra=()):
    sizes = torch.randint(1, max_size + 1, (n,), generator=gen)
    sizes[torch.rand(n, generator=gen) < p_empty] = 0
    sizes = torch.cat([sizes, torch.tensor(list(extra), dtype=torch.long)])
    return torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])


@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
def test_segment_ref_against_segment_reduce(reduce):
    gen = torch.Generator().manual_seed(1)
    ptr = ragged(200, 9, gen, extra=(0, 300, 1, 0))
    src = torch.randn(int(ptr[-1]), 5, generator=gen, dtype=torch.float64).requires_grad_()
    out, arg = P.segment_ref(src, ptr, reduce)
    ref = torch.segment_reduce(src, reduce, offsets=ptr, axis=0, initial=0.0 if reduce in ("max", "min") else None)
    empty = P.group_sizes(ptr) == 0
    ref = ref.masked_fill(empty.view(-1, 1), 0.0)        # empty groups give 0 in torch_scatter
    assert bool(empty.any()) and float(out[empty].abs().max()) == 0.0
    if reduce in ("max", "min"):
        # (initial = 0 would clip an all-negative max; take the extremum directly where the group is not empty)
        for g in (~empty).nonzero().flatten().tolist():
            seg = src[int(ptr[g]):int(ptr[g + 1])]
            assert torch.equal(out[g], seg.max(0).values if reduce == "max" else seg.min(0).values)
        assert torch.equal(arg, O.segment_arg(src, ptr, reduce))
    else:
        torch.testing.assert_close(out, ref, rtol=1e-13, atol=1e-13)
    w = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    o2 = O.segment_csr(src, ptr, reduce)
    (g_auto,) = torch.autograd.grad((o2 * w).sum(), src)
    torch.testing.assert_close(P.segment_grad_ref(w, ptr, reduce, arg, src.shape[0]), g_auto, rtol=1e-13, atol=1e-13)
    assert torch.equal(P.gather_ref(w, ptr), w[O.dense_index(ptr)])


def test_tie_rule_by_hand():
    """Two groups of ties: the FIRST row attaining the extremum wins, and only it receives the gradient."""
    ptr = torch.tensor([0, 4, 4, 7])
    src = torch.tensor([[1., -2.], [3., -2.], [3., 5.], [0., 5.],
                        [7., 7.], [7., 7.], [7., 6.]], dtype=torch.float64)
    out, arg = P.segment_ref(src, ptr, "max")
    assert arg.tolist() == [[1, 2], [-1, -1], [4, 4]]
    assert out.tolist() == [[3., 5.], [0., 0.], [7., 7.]]
    out, arg = P.segment_ref(src, ptr, "min")
    assert arg.tolist() == [[3, 0], [-1, -1], [4, 6]]
    assert out.tolist() == [[0., -2.], [0., 0.], [7., 6.]]
    g = P.segment_grad_ref(torch.tensor([[10., 20.], [30., 40.], [50., 60.]]), ptr, "min", arg, 7)
    assert g.tolist() == [[0., 20.], [0., 0.], [0., 0.], [10., 0.], [50., 0.], [0., 0.], [0., 60.]]
    # all -inf: the first row; a group holding +inf sums to +inf
    inf = float("inf")
    src = torch.tensor([[-inf], [-inf], [inf], [1.]], dtype=torch.float64)
    ptr = torch.tensor([0, 2, 4])
    assert P.segment_ref(src, ptr, "max")[1].tolist() == [[0], [2]]
    assert P.segment_ref(src, ptr, "sum")[0].tolist() == [[-inf], [inf]]


@pytest.mark.parametrize("scaling", [False, True])
def test_softmax_ref_against_torch_softmax(scaling):
    gen = torch.Generator().manual_seed(2)
    ptr = ragged(60, 12, gen, extra=(300, 0, 1))
    src = torch.randn(int(ptr[-1]), 3, generator=gen, dtype=torch.float64)
    w = torch.randn(src.shape, generator=gen, dtype=torch.float64)
    out, grad = P.softmax_ref(src, ptr, eps=0.0, scaling=scaling, gout=w)
    x = src.clone().requires_grad_()
    pieces = []
    for g in range(ptr.shape[0] - 1):
        b, e = int(ptr[g]), int(ptr[g + 1])
        if e > b:
            pieces.append(torch.softmax(x[b:e] / ((e - b) ** 0.5 if scaling else 1.0), 0))
    ref = torch.cat(pieces)
    torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(grad, torch.autograd.grad((ref * w).sum(), x)[0], rtol=1e-10, atol=1e-14)
    # the oracle's own expression and its autograd gradient (through the group max), at an eps large enough to matter
    xo = src.clone().requires_grad_()
    oo = O.segment_softmax_csr(xo, ptr, eps=1e-2, scaling=scaling)
    o2, g2 = P.softmax_ref(src, ptr, eps=1e-2, scaling=scaling, gout=w)
    torch.testing.assert_close(o2, oo.detach(), rtol=1e-7, atol=1e-12)
    torch.testing.assert_close(g2, torch.autograd.grad((oo * w).sum(), xo)[0], rtol=1e-6, atol=1e-9)
    # ... which is not the gradient with the max held constant: the eps term is some per cent of it
    x = src.clone().requires_grad_()
    c = x - P.segment_ref(src, ptr, "max")[0][O.dense_index(ptr)]
    if scaling:
        c = c / P.group_sizes(ptr).double().sqrt()[O.dense_index(ptr)].view(-1, 1)
    e = c.exp()
    den = torch.zeros((ptr.shape[0] - 1, 3), dtype=torch.float64).index_add(0, O.dense_index(ptr), e)
    g_const = torch.autograd.grad(((e / (den + 1e-2)[O.dense_index(ptr)]) * w).sum(), x)[0]
    assert float((g_const - g2).abs().max() / g2.abs().max()) > 1e-2
    torch.testing.assert_close(P.softmax_ref(src, ptr, eps=1e-3, scaling=scaling)[0],
                               O.segment_softmax_csr(src, ptr, eps=1e-3, scaling=scaling), rtol=1e-7, atol=1e-12)


@pytest.mark.parametrize("with_counts,given", [(True, False), (False, False), (True, True)])
def test_rowbn_ref_against_batchnorm1d(with_counts, given):
    gen = torch.Generator().manual_seed(3)
    R, C, slope = 40, 6, 0.2
    counts = torch.randint(0, 5, (R,), generator=gen, dtype=torch.int32) if with_counts else None
    y = torch.randn(R, C, generator=gen, dtype=torch.float64) * 2 + 1
    gamma, beta = torch.rand(C, generator=gen, dtype=torch.float64) + 0.5, torch.randn(C, generator=gen, dtype=torch.float64)
    gv = torch.randn(R, C, generator=gen, dtype=torch.float64)
    running = (torch.randn(C, dtype=torch.float64, generator=gen), torch.rand(C, dtype=torch.float64, generator=gen) + 0.5) \
        if given else None
    res = P.rowbn_ref(y, counts, gamma, beta, slope, gv, running)
    idx, cnt = P.view_index(R, counts)
    yr, gr, br = [t.clone().requires_grad_() for t in (y, gamma, beta)]
    yv = yr[idx]
    if given:
        zv = (yv - running[0]) / (running[1] + 1e-5).sqrt() * gr + br
    else:
        zv = (yv - yv.mean(0)) / (yv.var(0, unbiased=False) + 1e-5).sqrt() * gr + br
    ov = torch.nn.functional.leaky_relu(zv, slope)
    dy, dg, db = torch.autograd.grad((ov * gv[idx]).sum(), [yr, gr, br])
    first = (cnt.cumsum(0) - cnt)[cnt > 0]
    torch.testing.assert_close(res["out"][cnt > 0], ov.detach()[first], rtol=1e-12, atol=1e-12)
    for a, b in ((res["dy"], dy), (res["dgamma"], dg), (res["dbeta"], db)):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-11)
    if with_counts:
        assert bool((cnt == 0).any()) and float(res["dy"][cnt == 0].abs().max()) == 0.0
    # the side mask reproduces the plain derivative when it is the float64 side
    res2 = P.rowbn_ref(y, counts, gamma, beta, slope, gv, running, side=res["z"] > 0)
    torch.testing.assert_close(res2["dy"], res["dy"], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ulp_against_cast_neighbours(dtype):
    gen = torch.Generator().manual_seed(4)
    x = (torch.randn(20000, generator=gen, dtype=torch.float64) * 3).exp()
    x = torch.cat([x, -x, torch.tensor([1.0, 2.0, 0.5, 1e-6, 3e-8, 6.0e-5, 6.2e-5], dtype=torch.float64)])
    x = x[x.abs() < 6e4].float().double()          # fp32 values: the cast below is then ONE rounding, as on the device
    lo = x.float().to(dtype).double()              # the stored neighbour nearest to x
    u = P.ulp(x, dtype)
    assert bool(((x - lo).abs() <= 0.5 * u).all())
    # the next stored number away from zero is exactly one spacing further (checked where x is stored exactly)
    up = torch.nextafter(lo.to(dtype), torch.full_like(lo, float("inf")).to(dtype) * lo.sign().to(dtype)).double()
    assert torch.equal((up - lo).abs(), P.ulp(lo, dtype))
    assert float(P.ulp(torch.zeros(1, dtype=torch.float64), torch.float16)) == 2.0 ** -24


def fp32_rowwise_sum(src, ptr):
    """The kernels' arithmetic on the host: per (group, channel) a sequential fp32 sum in row order."""
    x = src.float().numpy()
    p = ptr.numpy()
    out = np.zeros((len(p) - 1, x.shape[1]), dtype=np.float32)
    sizes = p[1:] - p[:-1]
    short = sizes <= 64
    for j in range(int(sizes[short].max(initial=0))):      # row j of every short group at once
        live = short & (sizes > j)
        out[live] = out[live] + x[p[:-1][live] + j]
    for g in np.nonzero(~short)[0]:
        acc = np.zeros(x.shape[1], dtype=np.float32)
        for r in range(p[g], p[g + 1]):
            acc = acc + x[r]
        out[g] = acc
    return torch.from_numpy(out)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_ulp_gate_is_met_and_attained_by_fp32_emulation(dtype):
    """3000 groups of 0-39 rows plus one of 5000 and one of 1, C = 16, seeds 0-4, sum and mean: a correct kernel (fp32
    sum in row order, one rounding) never violates the 16-bit gate and comes within a few per cent of it; a truncating
    store violates it."""
    worst, n_elem, worst_trunc = 0.0, 0, 0.0
    for seed in range(5):
        gen = torch.Generator().manual_seed(seed)
        sizes = torch.cat([torch.randint(0, 40, (3000,), generator=gen), torch.tensor([5000, 1])])
        ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
        src = torch.randn(int(ptr[-1]), 16, generator=gen).to(dtype)
        acc = fp32_rowwise_sum(src, ptr)
        for reduce in ("sum", "mean"):
            a = acc if reduce == "sum" else acc / sizes.clamp(min=1).float().view(-1, 1)
            ref64, _ = P.segment_ref(src, ptr, reduce)
            ref32, _ = P.segment_ref(src, ptr, reduce, torch.float32)
            g = T.gate("out", T.rel_err(ref32, ref64))
            worst = max(worst, P.half_ulp_ratio(a.to(dtype), ref64, dtype, g))
            n_elem += ref64.numel()
            # truncation: clear the low 16 bits of the fp32 pattern (bf16) / round toward zero (fp16)
            if dtype == torch.bfloat16:
                tr = (a.view(torch.int32) & -65536).view(torch.float32).to(dtype)
            else:
                r = a.to(dtype)
                over = r.float().abs() > a.abs()
                tr = torch.where(over, torch.nextafter(r, torch.zeros_like(r)), r)
            worst_trunc = max(worst_trunc, P.half_ulp_ratio(tr, ref64, dtype, g))
    print(f"\n{dtype}: {n_elem} elements, worst err / bound {worst:.3f}, truncating store {worst_trunc:.3f}")
    assert n_elem >= 480000
    assert worst <= 1.0            # met
    assert worst > 0.9             # and attained: the bound has no slack to hide a second rounding in
    assert worst_trunc > 1.5       # a truncating store is caught
