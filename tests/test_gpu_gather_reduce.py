"""-m gpu: the fused gather + max / mean / sum / min pool (csrc/gather_reduce.hip, ``ops.gather_segment_reduce``) against the
materialised composition ``ops.segment_csr(x_mod.materialize(), ptr, reduce)`` -- forward bit for bit, backward against
float64 with the materialised route's own error as the yardstick -- and through ``BimodalCSRPool``.

Gates (tests/tolerances.py; nothing typed in):
  * forward: ``torch.equal`` (the same fp32 additions in the same order, one division, one rounding);
  * backward, fp32: ``rel_err`` against float64 <= ``gate("grad_in", fp32_err)``, fp32_err = the materialised route's
    error on the same case;
  * backward, bf16 / fp16: error against float64 <= AUTOCAST_ROW_HEADROOM x the materialised route's error on the same
    case (the fused route rounds once per map row, the materialised one per view and again per row).
"""
import numpy as np
import pytest
import torch

import gather_reduce_ref as GR
import tolerances as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REDUCES = ["max", "mean", "sum", "min"]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CHANNELS = [1, 13, 16, 24, 64, 200]


def lazy_of(ops, rows, row_idx, plan=None):
    return ops.GatheredFeatures(rows, row_idx, None, False, plan)


def device_case(C, dtype, seed=0):
    case = GR.make_case(C, dtype, seed)
    dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case.items()}
    return case, dev


def one_route(ops, fused, rows, row_idx, ptr, gout, reduce, plan=None):
    """(out, grad w.r.t. the map rows) of the fused op or of the materialised composition."""
    leaf = rows.detach().clone().requires_grad_()
    feats = lazy_of(ops, leaf, row_idx, plan)
    out = ops.gather_segment_reduce(feats, ptr, reduce) if fused else \
        ops.segment_csr(feats.materialize(), ptr, reduce=reduce)
    (g,) = torch.autograd.grad(out, leaf, grad_outputs=gout)
    return out.detach(), g


def both_routes(ops, rows, row_idx, ptr, gout, reduce):
    return [one_route(ops, fused, rows, row_idx, ptr, gout, reduce) for fused in (True, False)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", CHANNELS)
def test_fused_pool_against_the_materialised_composition(C, dtype):
    from deepviewagg_amd import ops
    case, dev = device_case(C, dtype)
    rows, row_idx, ptr, gout = dev["rows"], dev["row_idx"], dev["ptr"], dev["gout"]
    assert ops.gather_segment_reduce_applicable(lazy_of(ops, rows, row_idx), ptr, "min")
    plan = ops.row_plan(row_idx, case["R"], with_counts=False, split=False)[0]
    for reduce in REDUCES:
        (out, g), (out_m, g_m) = both_routes(ops, rows, row_idx, ptr, gout, reduce)
        # forward: bit for bit the composition, and the numpy restatement of the contract
        assert out.dtype == dtype and out.shape == (case["S"], C)
        assert torch.equal(out, out_m), (reduce, "forward differs from segment_csr on the materialised gather")
        want, _ = GR.forward_ref(GR.stored(case["rows"]), case["row_idx"].numpy(), case["ptr"].numpy(), reduce, dtype)
        assert np.array_equal(GR.stored(out), want), reduce
        atom = ops.gather_segment_reduce(lazy_of(ops, rows, row_idx), ptr, reduce, level="atom")
        assert isinstance(atom, ops.GatheredFeatures) and atom.exact and atom.shape == (case["S"], C)
        assert torch.equal(atom.rows, out) and torch.equal(atom.materialize(), out)
        assert torch.equal(atom.row_idx.cpu(), torch.arange(case["S"], dtype=torch.int32))
        # backward against float64
        _, arg64 = GR.forward_f64(GR.stored(case["rows"]), case["row_idx"].numpy(), case["ptr"].numpy(), reduce)
        g64 = torch.from_numpy(GR.backward_f64(GR.stored(case["gout"]), case["row_idx"].numpy(), case["ptr"].numpy(),
                                               reduce, arg64, case["R"]))
        assert g.dtype == dtype and g.shape == rows.shape
        err, err_m = T.rel_err(g, g64), T.rel_err(g_m, g64)
        bound = T.gate("grad_in", err_m) if dtype == torch.float32 else T.AUTOCAST_ROW_HEADROOM * err_m
        ratio = err / err_m if err_m > 0 else float("nan")
        print(f"gather_segment_reduce bwd C={C} {str(dtype)[6:]} {reduce}: fused {err:.3e} materialised {err_m:.3e} "
              f"ratio {ratio:.3f} bound {bound:.3e}")
        assert err <= bound, (reduce, err, err_m, bound)
        for r in GR.COLD_ROWS:
            assert float(g[r].float().abs().max()) == 0.0, "a map row no item gathers keeps a zero gradient"
        # determinism, and the plan handed in / a split plan (its permutation built on first use) give the same bits
        for p in (None, plan, ops.SplitPlan(row_idx, case["R"], None, None)):
            _, g2 = one_route(ops, True, rows, row_idx, ptr, gout, reduce, plan=p)
            assert torch.equal(g2, g), (reduce, type(p))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_max_pool_of_rows_whose_chunks_are_no_power_of_two(dtype):
    """C = 136: 17 chunks on 32 lanes in bf16 / fp16, 34 chunks on 64 lanes in fp32 -- the rows whose max gradient went
    through fp32 atomics before the plan reduction walked column passes.  Forward bit for bit, backward at the gates of
    ``test_fused_pool_against_the_materialised_composition``, and two runs give equal bits."""
    from deepviewagg_amd import ops
    C = 136
    case, dev = device_case(C, dtype)
    rows, row_idx, ptr, gout = dev["rows"], dev["row_idx"], dev["ptr"], dev["gout"]
    (out, g), (out_m, g_m) = both_routes(ops, rows, row_idx, ptr, gout, "max")
    assert torch.equal(out, out_m)
    want, _ = GR.forward_ref(GR.stored(case["rows"]), case["row_idx"].numpy(), case["ptr"].numpy(), "max", dtype)
    assert np.array_equal(GR.stored(out), want)
    _, arg64 = GR.forward_f64(GR.stored(case["rows"]), case["row_idx"].numpy(), case["ptr"].numpy(), "max")
    g64 = torch.from_numpy(GR.backward_f64(GR.stored(case["gout"]), case["row_idx"].numpy(), case["ptr"].numpy(), "max",
                                           arg64, case["R"]))
    err, err_m = T.rel_err(g, g64), T.rel_err(g_m, g64)
    bound = T.gate("grad_in", err_m) if dtype == torch.float32 else T.AUTOCAST_ROW_HEADROOM * err_m
    print(f"gather_segment_reduce bwd C={C} {str(dtype)[6:]} max: fused {err:.3e} materialised {err_m:.3e} bound {bound:.3e}")
    assert err <= bound, (err, err_m, bound)
    for r in GR.COLD_ROWS:
        assert float(g[r].float().abs().max()) == 0.0
    _, g2 = one_route(ops, True, rows, row_idx, ptr, gout, "max")
    assert torch.equal(g2, g), "two runs of the max gradient differ"


@pytest.mark.parametrize("reduce", REDUCES)
def test_min_ties_go_to_the_first_item(reduce):
    """Duplicated values in every segment: all items of a segment read one of two map rows that hold the same values."""
    from deepviewagg_amd import ops
    C = 16
    rows = torch.randn(4, C, device=DEV)
    rows[2] = rows[1]
    row_idx = torch.tensor([1, 2, 1, 2, 2, 1, 0, 3, 2, 1], dtype=torch.int32, device=DEV)
    ptr = torch.tensor([0, 3, 6, 6, 8, 10], device=DEV)
    gout = torch.randn(5, C, device=DEV)
    (out, g), (out_m, g_m) = both_routes(ops, rows, row_idx, ptr, gout, reduce)
    assert torch.equal(out, out_m)
    if reduce in GR.EXTREMA:
        assert torch.equal(g, g_m)          # every gradient element is a copy or a sum of two terms
        assert torch.equal(g[1], gout[0]) and torch.equal(g[2], gout[1] + gout[4])
    else:
        torch.testing.assert_close(g, g_m, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_nan_and_inf_are_treated_as_segment_csr_treats_them(dtype):
    """A NaN wins the max and the min only as the first item of its segment (``v > acc`` and ``v < acc`` are false for it
    afterwards), sums and means carry it; infinities order as usual.  Same bits as the materialised composition, NaN payloads included."""
    from deepviewagg_amd import ops
    C = 16
    rows = torch.randn(6, C, device=DEV)
    rows[1, ::2] = float("nan")
    rows[2, 1::3] = float("inf")
    rows[3, ::5] = float("-inf")
    rows = rows.to(dtype)
    row_idx = torch.tensor([1, 0, 4, 0, 1, 5, 2, 3, 0, 3, 1, 2], dtype=torch.int32, device=DEV)
    ptr = torch.tensor([0, 3, 6, 9, 12], device=DEV)
    bits = lambda t: t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)
    for reduce in REDUCES:
        out = ops.gather_segment_reduce(lazy_of(ops, rows, row_idx), ptr, reduce)
        want = ops.segment_csr(rows[row_idx.long()], ptr, reduce=reduce)
        assert torch.equal(bits(out), bits(want)), reduce
    for reduce in GR.EXTREMA:
        out = ops.gather_segment_reduce(lazy_of(ops, rows, row_idx), ptr, reduce).float()
        assert bool(torch.isnan(out[0, ::2]).all()) and not bool(torch.isnan(out[1]).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_empty_inputs(dtype):
    from deepviewagg_amd import ops
    C, R = 16, 8
    rows = torch.randn(R, C, device=DEV).to(dtype)
    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    for reduce in REDUCES:
        # S = 0
        leaf = rows.clone().requires_grad_()
        out = ops.gather_segment_reduce(lazy_of(ops, leaf, none), torch.zeros(1, dtype=torch.int64, device=DEV), reduce)
        assert out.shape == (0, C) and out.dtype == dtype
        (g,) = torch.autograd.grad(out.sum(), leaf)
        assert g.shape == (R, C) and float(g.float().abs().max()) == 0.0
        # P = 0: every segment is empty
        leaf = rows.clone().requires_grad_()
        ptr = torch.zeros(6, dtype=torch.int64, device=DEV)
        out = ops.gather_segment_reduce(lazy_of(ops, leaf, none), ptr, reduce)
        assert out.shape == (5, C) and float(out.detach().float().abs().max()) == 0.0
        assert torch.equal(out, ops.segment_csr(torch.zeros(0, C, device=DEV, dtype=dtype), ptr, reduce=reduce))
        (g,) = torch.autograd.grad(out, leaf, grad_outputs=torch.ones_like(out))
        assert g.shape == (R, C) and float(g.float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("layout", ["offset", "strided"])
def test_rows_off_the_16_byte_grid_and_non_contiguous_rows(layout, dtype):
    """``offset``: a contiguous slice whose storage offset is one element (C = 16 would take the 16-byte path, the base
    address sends it down the element path); ``strided``: every second column of a wider map (the op copies).  The op
    serves both under every mode; a module sends the max pool of the ``offset`` rows down the materialised route."""
    from deepviewagg_amd import ops
    case, dev = device_case(16, dtype, seed=2)
    R, C = case["R"], 16
    if layout == "offset":
        store = torch.zeros(R * C + 8, dtype=dtype, device=DEV)
        rows = store[1:1 + R * C].view(R, C)
        rows.copy_(dev["rows"])
        assert rows.is_contiguous() and rows.data_ptr() % 16 != 0
    else:
        wide = torch.zeros(R, 2 * C, dtype=dtype, device=DEV)
        wide[:, ::2] = dev["rows"]
        rows = wide[:, ::2]
        assert not rows.is_contiguous()
    for reduce in REDUCES:
        assert ops.gather_segment_reduce_applicable(lazy_of(ops, rows, dev["row_idx"]), dev["ptr"], reduce) \
            == (reduce != "max" or layout == "strided")
        leaf = rows.detach().requires_grad_()
        assert leaf.data_ptr() == rows.data_ptr()
        out = ops.gather_segment_reduce(lazy_of(ops, leaf, dev["row_idx"]), dev["ptr"], reduce)
        (g,) = torch.autograd.grad(out, leaf, grad_outputs=dev["gout"])
        (want, g_want), _ = both_routes(ops, dev["rows"], dev["row_idx"], dev["ptr"], dev["gout"], reduce)
        assert torch.equal(out, want) and torch.equal(g, g_want), reduce


class Counter:
    """Counts ``GatheredFeatures.materialize`` calls while active."""

    def __init__(self, ops, monkeypatch):
        self.calls = 0
        real = ops.GatheredFeatures.materialize

        def counting(feats):
            self.calls += 1
            return real(feats)
        monkeypatch.setattr(ops.GatheredFeatures, "materialize", counting)


def nearest_case(seed, B, C, H, W, N, max_views, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    k = torch.randint(0, max_views + 1, (N,), generator=gen)
    csr = torch.cat([torch.zeros(1, dtype=torch.long), k.cumsum(0)]).to(DEV)
    V = int(csr[-1])
    images = torch.randint(0, B, (V,), generator=gen).to(DEV)
    pixels = torch.stack([torch.randint(0, W, (V,), generator=gen), torch.randint(0, H, (V,), generator=gen)], 1) \
        .to(torch.int16).to(DEV)
    x0 = torch.randn(B, C, H, W, generator=gen).to(dtype)
    return csr, V, images, pixels, x0, gen


def test_view_level_mean_pool_never_materialises(monkeypatch):
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    B, C, H, W, N = 3, 24, 8, 12, 500
    csr, V, images, pixels, x0, gen = nearest_case(3, B, C, H, W, N, 6)
    x_map = torch.rand(V, 8, generator=gen).to(DEV)
    w = torch.randn(N, C, generator=gen).to(DEV)
    counter = Counter(ops, monkeypatch)
    pool = P.BimodalCSRPool(mode='mean')
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "LAZY_REDUCE", fused)
        x = x0.to(DEV).to(memory_format=torch.channels_last).requires_grad_()
        packed = ops.pack_gather_index(images, torch.arange(V + 1, device=DEV), pixels)
        feats = ops.lazy_gather_nearest(x, packed, exact=True)
        before = counter.calls
        out = pool(None, feats, x_map, csr)
        (g,) = torch.autograd.grad((out * w).sum(), x)
        res.append((out.detach(), g, counter.calls - before))
    (out, g, n_fused), (out_m, g_m, n_mat) = res
    assert n_fused == 0 and n_mat == 1
    assert torch.is_tensor(out) and out.shape == (N, C) and torch.equal(out, out_m)
    torch.testing.assert_close(g, g_m, rtol=1e-5, atol=1e-6)
    # save_last keeps the materialised route (the saved x_mod is the [V, C] tensor)
    monkeypatch.setattr(ops, "LAZY_REDUCE", True)
    keep = P.BimodalCSRPool(mode='mean', save_last=True)
    before = counter.calls
    assert torch.equal(keep(None, feats, x_map, csr), out) and counter.calls > before
    assert keep._last_x_mod.shape == (V, C)


def test_non_exact_mapping_stays_lazy_through_the_atomic_mean_pool(monkeypatch):
    """Several pixels per view through ``BimodalCSRPool('mean')`` at the atomic level + ``GroupBimodalCSRPool`` at the view
    level, against the ``LAZY_REDUCE = False`` run, at the gates of
    ``test_gpu_pool_modules.py::test_non_exact_mapping_stays_lazy_through_the_atomic_max_pool``."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    gen = torch.Generator().manual_seed(11)
    B, C, H, W, N = 4, 64, 16, 24, 1500
    k = torch.randint(0, 7, (N,), generator=gen)
    csr = torch.cat([torch.zeros(1, dtype=torch.long), k.cumsum(0)])
    V = int(csr[-1])
    atoms = torch.randint(1, 10, (V,), generator=gen)
    atom_ptr = torch.cat([torch.zeros(1, dtype=torch.long), atoms.cumsum(0)])
    Pn = int(atom_ptr[-1])
    images = torch.randint(0, B, (V,), generator=gen)
    pixels = torch.stack([torch.randint(0, W, (Pn,), generator=gen), torch.randint(0, H, (Pn,), generator=gen)], 1)
    x0 = torch.randn(B, C, H, W, generator=gen)
    x_map = torch.rand(V, 8, generator=gen).to(DEV)
    wout = torch.randn(N, C, generator=gen).to(DEV)
    torch.manual_seed(5)
    view_pool = P.GroupBimodalCSRPool(in_map=8, in_mod=C, num_groups=4, use_mod=False, map_encoder='DeepSetFeat',
                                      use_num=True).to(DEV).train()
    sd = {k_: v.clone() for k_, v in view_pool.state_dict().items()}
    atomic = P.BimodalCSRPool(mode='mean')

    def run(fused):
        monkeypatch.setattr(ops, "LAZY_REDUCE", fused)
        view_pool.load_state_dict(sd)
        for p_ in view_pool.parameters():
            p_.grad = None
        x = x0.to(DEV).to(memory_format=torch.channels_last).requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            xb = x.to(torch.bfloat16)
            lazy = ops.lazy_gather_nearest_mapping(xb, images.to(DEV), atom_ptr.to(DEV), pixels.to(DEV).to(torch.int16),
                                                   1.0, exact=False)
            pooled = atomic(None, lazy, None, atom_ptr.to(DEV))
            out = view_pool(None, pooled, x_map, csr.to(DEV))
        (out.float() * wout).sum().backward()
        return pooled, out.detach().float(), x.grad.detach().float(), \
            [p.grad.detach().float().clone() for p in view_pool.parameters()]
    pooled_l, out_l, gx_l, gp_l = run(True)
    pooled_m, out_m, gx_m, gp_m = run(False)
    assert isinstance(pooled_l, ops.GatheredFeatures) and isinstance(pooled_m, torch.Tensor)
    assert torch.equal(pooled_l.materialize().detach(), pooled_m.detach())          # the mean pool itself: bit-exact
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-20))
    assert rel(out_l, out_m) < 2e-2, rel(out_l, out_m)
    assert rel(gx_l, gx_m) < 6e-2, rel(gx_l, gx_m)
    for (n, _), a, b in zip(view_pool.named_parameters(), gp_l, gp_m):
        assert torch.isfinite(a).all(), n
        assert rel(a, b) < 2.5e-1, (n, rel(a, b))


def test_min_pool_of_a_65535_item_segment_takes_the_materialised_route(monkeypatch):
    """Max and min keep uint16 arg offsets: a segment of 65535 items materialises, one of 65534 does not."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    C, R = 4, 50
    gen = torch.Generator().manual_seed(4)
    sizes = torch.tensor([3, 65535, 0, 2])
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).to(DEV)
    Pn = int(ptr[-1])
    rows = torch.randn(R, C, generator=gen).to(DEV)
    row_idx = torch.randint(0, R, (Pn,), generator=gen).to(torch.int32).to(DEV)
    x_map = torch.rand(Pn, 8, device=DEV)
    feats = lazy_of(ops, rows, row_idx)
    assert ops.gather_segment_reduce_applicable(feats, ptr, "mean")           # only max and min keep uint16 offsets
    short = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor([3, 65534, 0, 3]).cumsum(0)]).to(DEV)
    counter = Counter(ops, monkeypatch)
    for mode in GR.EXTREMA:
        before = counter.calls
        assert not ops.gather_segment_reduce_applicable(feats, ptr, mode)
        out = P.BimodalCSRPool(mode=mode)(None, feats, x_map, ptr)
        assert counter.calls == before + 1
        assert torch.equal(out, ops.segment_csr(rows[row_idx.long()], ptr, reduce=mode))
        assert ops.gather_segment_reduce_applicable(feats, short, mode)
        assert torch.equal(P.BimodalCSRPool(mode=mode)(None, feats, x_map, short),
                           ops.segment_csr(rows[row_idx.long()], short, reduce=mode))
        assert counter.calls == before + 1


def test_no3d_tail_with_a_mean_view_pool_on_lazy_features(monkeypatch):
    """The image-only model's dataflow: lazy gather -> ``BimodalCSRPool('mean')`` over the views -> head, log-softmax and
    the view-level loss on the same lazy features (``models.no3d.no3d_tail``): logits and loss of the materialised run."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.models import no3d
    from deepviewagg_amd.modules.multimodal import pooling as P
    B, C, H, W, N, K = 2, 32, 8, 10, 300, 13
    csr, V, images, pixels, x0, gen = nearest_case(9, B, C, H, W, N, 5)
    x_map = torch.rand(V, 8, generator=gen).to(DEV)
    pos = torch.rand(N, 3, generator=gen).to(DEV)
    labels = torch.randint(0, K, (N,), generator=gen).to(DEV)
    seen = (csr[1:] > csr[:-1])
    torch.manual_seed(2)
    head = torch.nn.Sequential(torch.nn.Linear(C, K)).to(DEV)
    pool = P.BimodalCSRPool(mode='mean')
    counter = Counter(ops, monkeypatch)
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "LAZY_REDUCE", fused)
        x = x0.to(DEV).to(memory_format=torch.channels_last).requires_grad_()
        packed = ops.pack_gather_index(images, torch.arange(V + 1, device=DEV), pixels)
        feats = ops.lazy_gather_nearest(x, packed, exact=True)
        before = counter.calls
        features = pool(None, feats, x_map, csr)
        output, loss = no3d.no3d_tail(features, seen, pos, labels, head, True, (feats, csr))
        (g,) = torch.autograd.grad(loss + output.square().mean(), x)
        res.append((output.detach(), loss.detach(), g, counter.calls - before))
    (o, l, g, n_fused), (o_m, l_m, g_m, n_mat) = res
    assert n_fused == 0 and n_mat == 1
    assert torch.equal(o, o_m) and torch.equal(l, l_m)
    torch.testing.assert_close(g, g_m, rtol=1e-5, atol=1e-7)


def test_fused_route_saves_the_gathered_tensor():
    """V = 4096 views, C = 64, fp32: the peak of the pool's forward + backward lies at least V C 4 bytes below that of
    the ``LAZY_REDUCE = False`` route.  The output gradient is handed in (``grad_outputs``), so the peaks hold the pool's
    own tensors only.  Materialised: the [V, C] gather lives through the forward, its [V, C] gradient through the backward
    (never both), next to the output, the fp32 [R, C] sum and the int64 copy of the row index (8 V).  Fused: the output,
    the [R, C] gradient and the int32 segment of every item (4 V).  The difference is V C 4 + 4 V bytes."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    B, C, H, W, N = 2, 64, 16, 16, 1024
    gen = torch.Generator().manual_seed(6)
    csr = (torch.arange(N + 1) * 4).to(DEV)
    V = 4 * N
    images = torch.randint(0, B, (V,), generator=gen).to(DEV)
    pixels = torch.stack([torch.randint(0, W, (V,), generator=gen), torch.randint(0, H, (V,), generator=gen)], 1) \
        .to(torch.int16).to(DEV)
    x = torch.randn(B, C, H, W, generator=gen).to(DEV).to(memory_format=torch.channels_last).requires_grad_()
    x_map = torch.rand(V, 8, device=DEV)
    w = torch.randn(N, C, device=DEV)
    packed = ops.pack_gather_index(images, torch.arange(V + 1, device=DEV), pixels)
    feats = ops.lazy_gather_nearest(x, packed, exact=True)
    pool = P.BimodalCSRPool(mode='mean')

    def peak(fused):
        ops.LAZY_REDUCE = fused
        try:
            for measured in (False, True):        # the first pass warms the one-off allocations up
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                out = pool(None, feats, x_map, csr)
                (g,) = torch.autograd.grad(out, x, grad_outputs=w)
                torch.cuda.synchronize()
                top = torch.cuda.max_memory_allocated() - base
                del out, g
            return top
        finally:
            ops.LAZY_REDUCE = True
    fused, mat = peak(True), peak(False)
    print(f"peak allocated over forward + backward: fused {fused} B, materialised {mat} B, V C 4 = {V * C * 4} B")
    assert mat - fused >= V * C * 4, (fused, mat)
