"""-m gpu: the fused bilinear gather + max / mean / sum / min pool (csrc/interp_reduce.hip, ``ops.interp_segment_reduce``)
against the materialised composition ``ops.segment_csr(x_mod.materialize(), ptr, reduce)`` -- forward bit for bit, backward
against float64 with the materialised route's own error as the yardstick -- and through the pooling modules.

Gates (tests/tolerances.py; nothing typed in):
  * forward: ``torch.equal`` (the interpolation's products and sums, the rounding of the item, the fp32 additions in item
    order, one division, one rounding -- all the composition's);
  * backward, fp32: ``rel_err`` against float64 <= ``gate("grad_in", err_m)``, err_m = the materialised route's error on
    the same case;
  * backward, bf16 / fp16: error against float64 <= AUTOCAST_ROW_HEADROOM x err_m (the fused route rounds once per map
    row, the materialised one per item and again per row).
The backward has two branches -- the anchor plan where ``ops._anchor_ok`` serves the shape (fp32 / bf16, C = 16 and 64
here), the plan over the 4 P taps elsewhere -- and both are held to the same gates on the same cases
(``ops.INTERP_REDUCE_ANCHOR = False`` forces the tap plan).
The float64 gradient of max / min is taken at the winners of the forward that is differentiated (the restatement's, which
the kernel's equal): an item value rounded to bf16 may tie with, or pass, one that float64 ranks differently.
"""
import numpy as np
import pytest
import torch

import interp_reduce_ref as IR
import tolerances as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REDUCES = ["max", "mean", "sum", "min"]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CHANNELS = [1, 13, 16, 24, 64, 200]


def lazy_of(ops, xs, images, coords, parts=None, order=None, exact=False):
    """The bilinear lazy gather of items (``images``, ``coords``) on the maps ``xs``: one setting, or the ``cat`` of the
    settings' gathers (``parts`` = the items of every setting) in the given order."""
    items = []
    for x, pos in zip(xs, parts if parts is not None else [torch.arange(images.shape[0])]):
        n = pos.shape[0]
        packed = ops.pack_gather_index(images[pos].to(DEV), torch.arange(n + 1, device=DEV),
                                       torch.zeros(n, 2, dtype=torch.int16, device=DEV))
        items.append(ops.lazy_gather_bilinear(x, packed, coords[pos].to(DEV), exact))
    return items[0] if len(items) == 1 and order is None else ops.InterpolatedFeatures.cat(items, order=order)


def case_lazy(ops, case, xs):
    if len(case["settings"]) == 1:
        return lazy_of(ops, xs, case["images"], case["coords"])
    return lazy_of(ops, xs, case["images"], case["coords"], case["parts"], case["order"].to(DEV))


def leaves(case):
    return [x.to(DEV).to(memory_format=torch.channels_last).requires_grad_() for x in case["x"]]


def rows_of(grads):
    """Gradients of the maps [B, C, H, W] in the numbering of the stacked map rows."""
    return torch.cat([g.permute(0, 2, 3, 1).reshape(-1, g.shape[1]) for g in grads], 0)


def one_route(ops, fused, case, reduce, anchor=True, ws_bytes=None):
    """(out, gradient w.r.t. the stacked map rows, the lazy gather) of the fused op or of the materialised composition.
    ``anchor=False`` keeps the fused backward on the tap plan, ``ws_bytes`` bounds the anchor workspace (image chunks)."""
    xs = leaves(case)
    lazy = case_lazy(ops, case, xs)
    ptr = case["ptr"].to(DEV)
    keep = ops.INTERP_REDUCE_ANCHOR, ops.ANCHOR_WS_BYTES
    ops.INTERP_REDUCE_ANCHOR, ops.ANCHOR_WS_BYTES = anchor, ws_bytes
    try:
        out = ops.interp_segment_reduce(lazy, ptr, reduce) if fused else \
            ops.segment_csr(lazy.materialize(), ptr, reduce=reduce)
        grads = torch.autograd.grad(out, xs, grad_outputs=case["gout"].to(DEV))
    finally:
        ops.INTERP_REDUCE_ANCHOR, ops.ANCHOR_WS_BYTES = keep
    return out.detach(), rows_of(grads), lazy


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", CHANNELS)
def test_fused_pool_against_the_materialised_composition(C, dtype):
    from deepviewagg_amd import ops
    for settings in ((0,), (0, 1)):
        case = IR.make_case(C, dtype, settings=settings)
        ptr = case["ptr"].numpy()
        for reduce in REDUCES:
            out, g, lazy = one_route(ops, True, case, reduce)
            out_m, g_m, _ = one_route(ops, False, case, reduce)
            if reduce == REDUCES[0]:
                # the case generator's taps are the device's, and the planted views have no 2 x 2 structure
                assert torch.equal(lazy.tap_rows.cpu().long(), torch.from_numpy(case["tap_rows"]))
                assert torch.equal(lazy.tap_weights.cpu(), torch.from_numpy(case["tap_weights"]))
                dummy = ops.n_anchors(lazy.geometry)
                is_dummy = (lazy.anchors == dummy).cpu()
                assert sorted(torch.nonzero(is_dummy).reshape(-1).tolist()) == sorted(case["irregular"].tolist())
                assert ops.interp_segment_reduce_applicable(lazy, case["ptr"].to(DEV), "max")
            # forward: bit for bit the composition, and the numpy restatement of the contract
            assert out.dtype == dtype and out.shape == (case["S"], C)
            assert torch.equal(out, out_m), (settings, reduce, "forward differs from segment_csr on the materialised gather")
            want, arg = IR.forward_ref(IR.stored(case["rows"]), case["tap_rows"], case["tap_weights"], ptr, reduce, dtype)
            assert np.array_equal(IR.stored(out), want), (settings, reduce)
            atom = ops.interp_segment_reduce(lazy, case["ptr"].to(DEV), reduce, level="atom")
            assert isinstance(atom, ops.GatheredFeatures) and atom.exact and atom.shape == (case["S"], C)
            assert torch.equal(atom.rows, out) and torch.equal(atom.materialize(), out)
            assert torch.equal(atom.row_idx.cpu(), torch.arange(case["S"], dtype=torch.int32))
            # backward against float64
            won = IR.winners(arg, ptr) if arg is not None else None
            g64 = torch.from_numpy(IR.backward_f64(IR.stored(case["gout"]), case["tap_rows"], case["tap_weights"], ptr,
                                                   reduce, won, case["R"]))
            assert g.dtype == dtype and g.shape == (case["R"], C)
            err, err_m = T.rel_err(g, g64), T.rel_err(g_m, g64)
            bound = T.gate("grad_in", err_m) if dtype == torch.float32 else T.AUTOCAST_ROW_HEADROOM * err_m
            ratio = err / err_m if err_m > 0 else float("nan")
            print(f"interp_segment_reduce bwd {len(settings)} setting(s) C={C} {str(dtype)[6:]} {reduce}: fused {err:.3e} "
                  f"materialised {err_m:.3e} ratio {ratio:.3f} bound {bound:.3e}")
            assert err <= bound, (settings, reduce, err, err_m, bound)
            for r in case["cold"]:
                assert float(g[r].float().abs().max()) == 0.0, "a map row no tap touches keeps a zero gradient"
            if reduce in ("sum", "mean"):
                # the irregular views' taps are in the gradient: its component along their float64 contribution d
                w0 = case["tap_weights"].copy()
                w0[case["irregular"].numpy()] = 0
                less = torch.from_numpy(IR.backward_f64(IR.stored(case["gout"]), case["tap_rows"], w0, ptr, reduce, won,
                                                        case["R"]))
                d = g64 - less
                share = float(((g.double().cpu() - less) * d).sum() / (d * d).sum())      # 1: present, 0: missing
                assert share > 0.5, (settings, reduce, share, "the taps of the irregular views are missing")
            _, g2, _ = one_route(ops, True, case, reduce)
            assert torch.equal(g2, g), (reduce, "two runs differ")
            if ops._anchor_ok(C, dtype):
                # g came over the anchor plan: the tap plan on the same case at the same gates, and the anchor plan with
                # its workspace bounded to one image per pass (same sums, same bits)
                _, g_tap, _ = one_route(ops, True, case, reduce, anchor=False)
                err_t = T.rel_err(g_tap, g64)
                print(f"  tap plan {err_t:.3e}")
                assert err_t <= bound, (settings, reduce, err_t, err_m, bound)
                for r in case["cold"]:
                    assert float(g_tap[r].float().abs().max()) == 0.0
                _, g3, _ = one_route(ops, True, case, reduce, anchor=False)
                assert torch.equal(g3, g_tap)
                _, g4, _ = one_route(ops, True, case, reduce, ws_bytes=1)
                assert torch.equal(g4, g)
                # which kernels ran: the launches' names
                for anchor, name in ((True, "interp_anchor_sum"), (False, "interp_segment_reduce_bwd")):
                    ops.TIMER = ops.KernelTimer()
                    try:
                        one_route(ops, True, case, reduce, anchor=anchor)
                        ran = set(ops.TIMER.summary())
                    finally:
                        ops.TIMER = None
                    assert name in ran and len(ran & {"interp_anchor_sum", "interp_segment_reduce_bwd"}) == 1, (anchor, ran)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_nan_and_inf_are_treated_as_the_composition_treats_them(dtype):
    """NaN and +-Inf in the map rows: the same bits as the materialised composition, NaN payloads included, for the four
    reduces (a NaN item wins max / min only as the first item of its segment; 0 x Inf of a zero-weight tap is a NaN)."""
    from deepviewagg_amd import ops
    C, H, W = 16, 3, 4
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, C, H, W, generator=gen)
    x[0, ::2, 1, 1] = float("nan")
    x[0, 1::3, 0, 2] = float("inf")
    x[1, ::5, 2, 3] = float("-inf")
    x[1, 3::4, 1, 0] = float("nan")
    x = x.to(dtype).to(DEV).to(memory_format=torch.channels_last)
    P = 96
    images = torch.randint(0, 2, (P,), generator=gen)
    coords = torch.rand(P, 2, generator=gen)
    coords[::7] = torch.tensor([0.5, 0.375])          # exact pixel centres of the 3 x 4 map: weights 0 and 1
    ptr = torch.tensor([0, 5, 5, 37, 40, 96]).to(DEV)
    lazy = lazy_of(ops, [x], images, coords)
    assert bool(torch.isnan(lazy.materialize().float()).any()) and bool(torch.isinf(lazy.materialize().float()).any())
    for reduce in REDUCES:
        out = ops.interp_segment_reduce(lazy, ptr, reduce)
        want = ops.segment_csr(lazy.materialize(), ptr, reduce=reduce)
        assert torch.equal(bits(out), bits(want)), reduce


@pytest.mark.parametrize("reduce", REDUCES)
def test_ties_go_to_the_first_item(reduce):
    """Every item of a segment interpolates to the same value: two maps hold equal contents and the items of a segment
    share their coordinates.  Max and min give their gradient to the first item only."""
    from deepviewagg_amd import ops
    C, H, W = 16, 4, 6
    gen = torch.Generator().manual_seed(8)
    one = torch.randn(1, C, H, W, generator=gen)
    x = torch.cat([one, one, torch.randn(1, C, H, W, generator=gen)]).to(DEV).to(memory_format=torch.channels_last) \
        .requires_grad_()
    images = torch.tensor([1, 0, 1, 0, 0, 1, 2, 2, 0, 1])
    at = torch.tensor([[0.3, 0.6], [0.7, 0.2], [0.1, 0.1], [0.5, 0.9]])
    coords = at[torch.tensor([0, 0, 0, 1, 1, 1, 2, 2, 3, 3])]
    ptr = torch.tensor([0, 3, 6, 6, 8, 10]).to(DEV)
    gout = torch.randn(5, C, generator=gen).to(DEV)
    res = []
    for fused in (True, False):
        lazy = lazy_of(ops, [x], images, coords)
        out = ops.interp_segment_reduce(lazy, ptr, reduce) if fused else \
            ops.segment_csr(lazy.materialize(), ptr, reduce=reduce)
        (g,) = torch.autograd.grad(out, x, grad_outputs=gout)
        res.append((out.detach(), g))
    (out, g), (out_m, g_m) = res
    assert torch.equal(out, out_m)
    torch.testing.assert_close(g, g_m, rtol=1e-5, atol=1e-6)
    if reduce in ("max", "min"):
        # segment 0: first item on map 1; segment 1: first item on map 0; segment 4: first item on map 0
        first_only = lazy_of(ops, [x], images[[0, 3, 6, 8]], coords[[0, 3, 6, 8]])
        solo = ops.interp_segment_reduce(first_only, torch.tensor([0, 1, 2, 2, 3, 4]).to(DEV), "sum")
        (g_first,) = torch.autograd.grad(solo, x, grad_outputs=gout)
        torch.testing.assert_close(g, g_first, rtol=1e-6, atol=1e-7)
        # map 0 gets nothing from segment 0, whose later items alone lie on it
        lone = lazy_of(ops, [x], images[[3, 8]], coords[[3, 8]])
        (g_lone,) = torch.autograd.grad(ops.interp_segment_reduce(lone, torch.tensor([0, 1, 2]).to(DEV), "sum"), x,
                                        grad_outputs=gout[[1, 4]])
        torch.testing.assert_close(g[0], g_lone[0], rtol=1e-6, atol=1e-7)


def taps_features(ops, rows, tap_rows, tap_weights):
    """An ``InterpolatedFeatures`` from taps alone (no coordinates: ``materialize`` is not available)."""
    f = ops.InterpolatedFeatures.__new__(ops.InterpolatedFeatures)
    f.x = f.packed_idx = f.coords = f.parts = f.order = f.anchors = None
    f.rows, f.tap_rows, f.tap_weights, f.exact = rows, tap_rows, tap_weights, False
    f.geometry = [(1, 1, rows.shape[0])]
    return f


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_empty_inputs(dtype):
    from deepviewagg_amd import ops
    C, R = 16, 8
    rows = torch.randn(R, C, device=DEV).to(dtype)
    no_rows = torch.zeros((0, 4), dtype=torch.int32, device=DEV)
    no_w = torch.zeros((0, 4), dtype=torch.float32, device=DEV)
    for reduce in REDUCES:
        # S = 0
        leaf = rows.clone().requires_grad_()
        out = ops.interp_segment_reduce(taps_features(ops, leaf, no_rows, no_w), torch.zeros(1, dtype=torch.int64, device=DEV),
                                        reduce)
        assert out.shape == (0, C) and out.dtype == dtype
        (g,) = torch.autograd.grad(out.sum(), leaf)
        assert g.shape == (R, C) and float(g.float().abs().max()) == 0.0
        # P = 0 with S > 0: every segment is empty
        leaf = rows.clone().requires_grad_()
        ptr = torch.zeros(6, dtype=torch.int64, device=DEV)
        out = ops.interp_segment_reduce(taps_features(ops, leaf, no_rows, no_w), ptr, reduce)
        assert out.shape == (5, C) and float(out.detach().float().abs().max()) == 0.0
        assert torch.equal(out, ops.segment_csr(torch.zeros(0, C, device=DEV, dtype=dtype), ptr, reduce=reduce))
        (g,) = torch.autograd.grad(out, leaf, grad_outputs=torch.ones_like(out))
        assert g.shape == (R, C) and float(g.float().abs().max()) == 0.0
        # R = 0: no map row, no item
        leaf = rows[:0].clone().requires_grad_()
        out = ops.interp_segment_reduce(taps_features(ops, leaf, no_rows, no_w), ptr, reduce)
        assert out.shape == (5, C) and float(out.detach().float().abs().max()) == 0.0
        (g,) = torch.autograd.grad(out, leaf, grad_outputs=torch.ones_like(out))
        assert g.shape == (0, C)
        # items, but all of them behind empty leading segments and before empty trailing ones
        leaf = rows.clone().requires_grad_()
        t = torch.tensor([[0, 1, 2, 3], [4, 4, 5, 5]], dtype=torch.int32, device=DEV)
        w = torch.tensor([[0.25, 0.25, 0.25, 0.25], [0.5, 0.0, 0.5, 0.0]], device=DEV)
        ptr = torch.tensor([0, 0, 0, 2, 2, 2], device=DEV)
        out = ops.interp_segment_reduce(taps_features(ops, leaf, t, w), ptr, reduce)
        assert float(out[[0, 1, 3, 4]].detach().float().abs().max()) == 0.0
        (g,) = torch.autograd.grad(out, leaf, grad_outputs=torch.ones_like(out))
        assert float(g[6:].float().abs().max()) == 0.0
        if reduce == "sum":
            assert g[:, 0].float().tolist() == [0.25, 0.25, 0.25, 0.25, 0.5, 0.5, 0.0, 0.0]


class Counter:
    """Counts ``InterpolatedFeatures.materialize`` calls while active (a ``cat`` counts once: the parts' calls go through
    the same method and are not counted again)."""

    def __init__(self, ops, monkeypatch):
        self.calls, self.depth = 0, 0
        real = ops.InterpolatedFeatures.materialize

        def counting(feats, *a, **k):
            if self.depth == 0:
                self.calls += 1
            self.depth += 1
            try:
                return real(feats, *a, **k)
            finally:
                self.depth -= 1
        monkeypatch.setattr(ops.InterpolatedFeatures, "materialize", counting)


def module_gates(g, g_m, g64, dtype):
    err, err_m = T.rel_err(g, g64), T.rel_err(g_m, g64)
    bound = T.gate("grad_in", err_m) if dtype == torch.float32 else T.AUTOCAST_ROW_HEADROOM * err_m
    assert err <= bound, (err, err_m, bound)


@pytest.mark.parametrize("mode", REDUCES)
@pytest.mark.parametrize("settings", [(0,), (0, 1)], ids=["single", "cat"])
def test_view_level_pool_of_the_module_never_materialises(settings, mode, monkeypatch):
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    C, dtype = 24, torch.float32
    case = IR.make_case(C, dtype, seed=2, settings=settings)
    ptr = case["ptr"].to(DEV)
    x_map = torch.rand(case["P"], 8, device=DEV)
    counter = Counter(ops, monkeypatch)
    pool = P.BimodalCSRPool(mode=mode)
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "LAZY_INTERP_REDUCE", fused)
        xs = leaves(case)
        feats = case_lazy(ops, case, xs)
        before = counter.calls
        out = pool(None, feats, x_map, ptr)
        grads = torch.autograd.grad(out, xs, grad_outputs=case["gout"].to(DEV))
        res.append((out.detach(), rows_of(grads), counter.calls - before))
    (out, g, n_fused), (out_m, g_m, n_mat) = res
    assert n_fused == 0 and n_mat == 1
    assert torch.is_tensor(out) and out.shape == (case["S"], C) and torch.equal(out, out_m)
    _, arg = IR.forward_ref(IR.stored(case["rows"]), case["tap_rows"], case["tap_weights"], case["ptr"].numpy(), mode, dtype)
    won = IR.winners(arg, case["ptr"].numpy()) if arg is not None else None
    g64 = torch.from_numpy(IR.backward_f64(IR.stored(case["gout"]), case["tap_rows"], case["tap_weights"],
                                           case["ptr"].numpy(), mode, won, case["R"]))
    module_gates(g, g_m, g64, dtype)
    # save_last keeps the materialised route (the saved x_mod is the [V, C] tensor)
    monkeypatch.setattr(ops, "LAZY_INTERP_REDUCE", True)
    keep = P.BimodalCSRPool(mode=mode, save_last=True)
    before = counter.calls
    assert torch.equal(keep(None, feats, x_map, ptr), out) and counter.calls == before + 1
    assert keep._last_x_mod.shape == (case["P"], C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", REDUCES)
def test_atomic_level_pool_of_a_non_exact_mapping(mode, dtype, monkeypatch):
    """``x_map`` is None (the atomic pool of ``UnimodalBranch``) and the segments are the views' atoms: the plain [V, C]
    tensor comes out on both routes."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    C = 16
    case = IR.make_case(C, dtype, seed=3, settings=(0,))
    ptr = case["ptr"].to(DEV)
    counter = Counter(ops, monkeypatch)
    pool = P.BimodalCSRPool(mode=mode)
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "LAZY_INTERP_REDUCE", fused)
        xs = leaves(case)
        feats = case_lazy(ops, case, xs)
        assert not feats.exact and case["S"] < case["P"]
        before = counter.calls
        out = pool(None, feats, None, ptr)
        grads = torch.autograd.grad(out, xs, grad_outputs=case["gout"].to(DEV))
        res.append((out.detach(), rows_of(grads), counter.calls - before))
    (out, g, n_fused), (out_m, g_m, n_mat) = res
    assert n_fused == 0 and n_mat == 1
    assert torch.is_tensor(out) and torch.is_tensor(out_m) and torch.equal(out, out_m)
    _, arg = IR.forward_ref(IR.stored(case["rows"]), case["tap_rows"], case["tap_weights"], case["ptr"].numpy(), mode, dtype)
    won = IR.winners(arg, case["ptr"].numpy()) if arg is not None else None
    g64 = torch.from_numpy(IR.backward_f64(IR.stored(case["gout"]), case["tap_rows"], case["tap_weights"],
                                           case["ptr"].numpy(), mode, won, case["R"]))
    module_gates(g, g_m, g64, dtype)


def test_unimodal_branch_with_a_mean_view_pool_and_one_optimiser_step(monkeypatch):
    """``UnimodalBranch(interpolate=True)`` with ``BimodalCSRPool('mean')`` over the views (the mean-pool baseline) on the
    two-setting fixture of ``test_gpu_data.py``: no [V, C] tensor on the fused route, the output of the materialised run bit
    for bit, and after one SGD step on the encoder the same output again at fp32 rounding."""
    from conftest import load_golden, t, state_dict_from
    from test_gpu_data import make_image_data, Conv
    from deepviewagg_amd import ops
    from deepviewagg_amd.core.multimodal.image import ImageData
    from deepviewagg_amd.modules.multimodal import UnimodalBranch, BimodalCSRPool, BimodalFusion
    g = load_golden("branch_bilinear")
    n_set = int(g["n_settings"])
    counter = Counter(ops, monkeypatch)

    def run(fused):
        monkeypatch.setattr(ops, "LAZY_INTERP_REDUCE", fused)
        xs = [t(g[f"s{i}_x_img"], DEV) for i in range(n_set)]
        conv = Conv(6, 8)
        conv.load_state_dict(state_dict_from(g, "sd_conv/"))
        branch = UnimodalBranch(conv, BimodalCSRPool(mode="max"), BimodalCSRPool(mode="mean"),
                                BimodalFusion(mode="concatenation"), interpolate=True).to(DEV).train()
        opt = torch.optim.SGD(branch.parameters(), lr=0.1)
        outs = []
        before = counter.calls
        for _ in range(2):
            sds = [make_image_data(g, f"s{i}_", xs[i], g[f"s{i}_ref_size"], DEV) for i in range(n_set)]
            mm = {"x_3d": t(g["x_3d"], DEV), "x_seen": None, "modalities": {"image": ImageData(sds)}}
            y = branch(mm, "image")["x_3d"]
            outs.append(y.detach().clone())
            opt.zero_grad()
            (y * t(g["w"], DEV)).sum().backward()
            opt.step()
        grad = branch.conv.conv.weight.grad.detach().clone()
        return outs, grad, counter.calls - before
    (y0, y1), gw, n_fused = run(True)
    (y0_m, y1_m), gw_m, n_mat = run(False)
    assert n_fused == 0 and n_mat >= 2
    assert torch.equal(y0, y0_m)
    assert float((y1 - y0).abs().max()) > 0, "the step moved the encoder"
    torch.testing.assert_close(gw, gw_m, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(y1, y1_m, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("mode", ["max", "min"])
def test_heuristic_pool_interpolates_the_selected_views_only(mode, monkeypatch):
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    C = 24
    case = IR.make_case(C, torch.float32, seed=4, settings=(0,))
    ptr = case["ptr"].to(DEV)
    x_map = torch.rand(case["P"], 8, device=DEV)
    counter = Counter(ops, monkeypatch)
    xs = leaves(case)
    feats = case_lazy(ops, case, xs)
    out = P.HeuristicBimodalCSRPool(mode=mode, feat=2)(None, feats, x_map, ptr)
    assert counter.calls == 0
    want = P.HeuristicBimodalCSRPool(mode=mode, feat=2)(None, feats.materialize(), x_map, ptr)
    assert out.shape == (case["S"], C) and torch.equal(out, want)
    empty = (case["ptr"][1:] == case["ptr"][:-1]).to(DEV)
    assert float(out.detach()[empty].abs().max()) == 0.0
    (gx,) = torch.autograd.grad(out, xs, grad_outputs=case["gout"].to(DEV))
    (gx_m,) = torch.autograd.grad(want, xs, grad_outputs=case["gout"].to(DEV))
    torch.testing.assert_close(gx, gx_m, rtol=1e-5, atol=1e-6)
    # save_last and a cat of settings keep materialising
    before = counter.calls
    assert torch.equal(P.HeuristicBimodalCSRPool(mode=mode, feat=2, save_last=True)(None, feats, x_map, ptr), want)
    assert counter.calls == before + 1
    both = IR.make_case(C, torch.float32, seed=4, settings=(0, 1))
    cat = case_lazy(ops, both, leaves(both))
    before = counter.calls
    got = P.HeuristicBimodalCSRPool(mode=mode, feat=2)(None, cat, torch.rand(both["P"], 8, device=DEV), both["ptr"].to(DEV))
    assert counter.calls == before + 1 and got.shape == (both["S"], C)


def test_extremum_of_a_65535_item_segment_takes_the_materialised_route(monkeypatch):
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    C = 4
    gen = torch.Generator().manual_seed(4)
    sizes = torch.tensor([3, 65535, 0, 2])
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).to(DEV)
    Pn = int(ptr[-1])
    x = torch.randn(2, C, 5, 5, generator=gen).to(DEV).to(memory_format=torch.channels_last)
    feats = lazy_of(ops, [x], torch.randint(0, 2, (Pn,), generator=gen), torch.rand(Pn, 2, generator=gen))
    x_map = torch.rand(Pn, 8, device=DEV)
    counter = Counter(ops, monkeypatch)
    mat = feats.materialize()
    assert counter.calls == 1
    for mode in ("max", "min"):
        assert not ops.interp_segment_reduce_applicable(feats, ptr, mode)
        before = counter.calls
        out = P.BimodalCSRPool(mode=mode)(None, feats, x_map, ptr)
        assert counter.calls == before + 1
        assert torch.equal(out, ops.segment_csr(mat, ptr, reduce=mode))
    assert ops.interp_segment_reduce_applicable(feats, ptr, "mean")           # only max and min keep uint16 offsets
    before = counter.calls
    assert torch.equal(P.BimodalCSRPool(mode="mean")(None, feats, x_map, ptr), ops.segment_csr(mat, ptr, reduce="mean"))
    assert counter.calls == before
    short = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor([3, 65534, 0, 3]).cumsum(0)]).to(DEV)
    for mode in ("max", "min"):
        assert ops.interp_segment_reduce_applicable(feats, short, mode)
        assert torch.equal(P.BimodalCSRPool(mode=mode)(None, feats, x_map, short), ops.segment_csr(mat, short, reduce=mode))
    assert counter.calls == before


def test_fused_route_stays_below_the_gathered_tensor():
    """P = 2^17 items in 4096 segments of 32, 4 maps of 32 x 64, C = 64, fp32, mean, forward + backward with the output
    gradient handed in: the fused route's peak of allocated memory above its inputs stays below P C 4 bytes -- the tensor
    it exists to avoid; the tap plan and its sort are about a quarter of it -- and the materialised route's is at least
    that."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    B, C, H, W, N = 4, 64, 32, 64, 4096
    gen = torch.Generator().manual_seed(6)
    V = 32 * N
    csr = (torch.arange(N + 1) * 32).to(DEV)
    x = torch.randn(B, C, H, W, generator=gen).to(DEV).to(memory_format=torch.channels_last).requires_grad_()
    feats = lazy_of(ops, [x], torch.randint(0, B, (V,), generator=gen), torch.rand(V, 2, generator=gen), exact=True)
    x_map = torch.rand(V, 8, device=DEV)
    w = torch.randn(N, C, device=DEV)
    pool = P.BimodalCSRPool(mode='mean')

    def peak(fused):
        ops.LAZY_INTERP_REDUCE = fused
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
            ops.LAZY_INTERP_REDUCE = True
    fused, mat = peak(True), peak(False)
    print(f"peak allocated over forward + backward: fused {fused} B, materialised {mat} B, P C 4 = {V * C * 4} B")
    assert fused < V * C * 4, (fused, V * C * 4)
    assert mat >= V * C * 4, (mat, V * C * 4)
