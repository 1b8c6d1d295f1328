"""CPU tests of the fused bilinear gather + max / mean / sum / min pool: the shared case holds what it promises, the numpy
restatement of the forward against float64, the float64 gradient against autograd, the argument checks of the two C
entries, the switch and the applicability rules, and the fall-through of ``BimodalCSRPool`` to the materialised route
(no GPU needed)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import interp_reduce_ref as IR
from deepviewagg_amd import _lib, ops
from deepviewagg_amd.modules.multimodal import pooling as P

REDUCES = ["max", "mean", "sum", "min"]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.mark.parametrize("settings", [(0,), (0, 1)], ids=["single", "cat"])
def test_case_holds_every_kind_of_tap_block(settings):
    case = IR.make_case(13, torch.float32, settings=settings)
    sizes = (case["ptr"][1:] - case["ptr"][:-1]).tolist()
    assert sizes[0] == 0 and sizes[-1] == 0 and {1, 2, 70, 300} <= set(sizes)
    assert 700 <= case["P"] <= 900
    t, w = case["tap_rows"], case["tap_weights"]
    assert case["R"] == (IR.R_ROWS if len(settings) == 2 else 48) and t.min() >= 0 and t.max() < case["R"]
    irr = case["irregular"].numpy()
    regular = np.ones(case["P"], dtype=bool)
    regular[irr] = False
    assert np.allclose(w[regular].sum(1), 1.0, atol=1e-6)
    assert np.allclose(w[irr].sum(1), 2.0, atol=1e-6), "floor(q + 1) = floor(q) + 2: both rows weigh about 1"
    hits = np.bincount(t.reshape(-1), minlength=case["R"])
    assert len(case["cold"]) == (3 if len(settings) == 2 else 2) and all(hits[r] == 0 for r in case["cold"])
    distinct = np.array([len(set(r)) for r in t.tolist()])
    assert (distinct == 1).sum() >= 8 and (distinct == 2).sum() >= 20 and (distinct == 4).sum() >= 300
    assert ((w == 1.0).any(1)).sum() >= 20, "exact pixel centres: one weight 1, three weights 0"
    cells, counts = np.unique(t, axis=0, return_counts=True)
    assert counts.max() >= 300, "one cell owns at least 300 items"
    assert len(irr) >= 2
    for p in irr:           # floor(q) = 0 -> clamped row 0, floor(q + 1) = 2 -> row 1 of the map: no 2 x 2 block of a
        rows = (t[p] - (t[p] // 24) * 24) // 6          # padded grid starts at padded row 0 and ends at padded row 2
        assert rows[0] == 0 and rows[2] == 1 and float(np.float32(case["coords"][p, 0]) * np.float32(4)
                                                       + np.float32(0.5)) == 1 - 2.0 ** -24
    if len(settings) == 2:
        assert sorted(case["order"].tolist()) == list(range(case["P"])) and \
            case["order"].tolist() != list(range(case["P"]))
        concat = torch.cat(case["parts"])
        assert torch.equal(concat[case["order"]], torch.arange(case["P"]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [1, 13, 16])
def test_forward_restatement_lies_within_one_rounding_of_float64(C, dtype):
    """Per element, against float64 on the stored map values.  With u = half an ulp of the storage type at 1 and A the
    magnitude sum_k |w_k x_k| summed (mean: averaged) over the segment's n items: every item is rounded once to the storage
    type (<= u A in the sum), the result once more (<= u |out| <= u A), and the fp32 evaluation adds at most
    (n + 8) 2^-24 A (four products and three sums per item, n - 1 sums, one division).  max / min return one item's
    stored value: u A_max + 8 2^-24 A_max with A_max the largest item magnitude of the segment."""
    case = IR.make_case(C, dtype)
    rows, ptr = IR.stored(case["rows"]), case["ptr"].numpy()
    n = (ptr[1:] - ptr[:-1]).astype(np.float64)[:, None]
    u = IR.UNIT[dtype]
    ties = 0
    for reduce in REDUCES:
        out, arg = IR.forward_ref(rows, case["tap_rows"], case["tap_weights"], ptr, reduce, dtype)
        want, arg64, scale = IR.forward_f64(rows, case["tap_rows"], case["tap_weights"], ptr, reduce)
        if reduce in ("sum", "mean"):
            assert arg is None
            bound = (2 * u + (n + 8) * 2.0 ** -24) * scale
        else:
            bound = (u + 8 * 2.0 ** -24) * scale
            won = IR.winners(arg, ptr)
            assert ((won >= 0) == (n > 0)).all() and (won[n[:, 0] == 0] == -1).all()
            v = IR.item_values(rows, case["tap_rows"], case["tap_weights"], dtype)
            for s in np.nonzero(n[:, 0] >= 2)[0]:
                seg = v[ptr[s]:ptr[s + 1]]
                best = seg.max(0) if reduce == "max" else seg.min(0)
                ties += int(((seg == best).sum(0) > 1).sum())
                first = (seg == best).argmax(0)
                assert np.array_equal(first, won[s] - ptr[s]), "the first of equal items wins"
        assert (np.abs(out.astype(np.float64) - want) <= bound).all(), reduce
        assert (out[n[:, 0] == 0] == 0).all()
    assert ties > 0, "the case holds no duplicated extremum: the first-item rule is not exercised"


@pytest.mark.parametrize("reduce", REDUCES)
def test_float64_references_agree_with_autograd(reduce):
    case = IR.make_case(13, torch.float32, seed=1)
    rows = case["rows"].double().requires_grad_()
    t, w, ptr = torch.from_numpy(case["tap_rows"]), torch.from_numpy(case["tap_weights"]).double(), case["ptr"]
    x = (rows[t] * w.unsqueeze(-1)).sum(1)
    out64, arg, _ = IR.forward_f64(IR.stored(case["rows"]), case["tap_rows"], case["tap_weights"], ptr.numpy(), reduce)
    outs = []
    for s, (b, e) in enumerate(zip(ptr[:-1].tolist(), ptr[1:].tolist())):
        seg = x[b:e]
        if e == b:
            outs.append(torch.zeros(x.shape[1], dtype=torch.float64))
        elif reduce in ("sum", "mean"):
            outs.append(seg.sum(0) if reduce == "sum" else seg.mean(0))
        else:       # the winners of the float64 forward: amax / amin would spread the gradient over ties
            outs.append(x[torch.from_numpy(arg[s]), torch.arange(x.shape[1])])
    out = torch.stack(outs)
    assert np.allclose(out64, out.detach().numpy(), rtol=1e-13, atol=1e-13)
    (g,) = torch.autograd.grad((out * case["gout"].double()).sum(), rows)
    g64 = IR.backward_f64(IR.stored(case["gout"]), case["tap_rows"], case["tap_weights"], ptr.numpy(), reduce, arg,
                          case["R"])
    assert np.allclose(g64, g.numpy(), rtol=1e-12, atol=1e-12)
    assert all(float(np.abs(g64[r]).max()) == 0.0 for r in case["cold"])
    irr = case["irregular"].numpy()
    if reduce in ("sum", "mean"):       # the irregular views' taps are in the float64 gradient
        w0 = case["tap_weights"].copy()
        w0[irr] = 0
        without = IR.backward_f64(IR.stored(case["gout"]), case["tap_rows"], w0, ptr.numpy(), reduce, arg, case["R"])
        assert float(np.abs(g64 - without).max()) > 1e-3


def test_entries_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.dva_version() >= 330
    fwd, bwd = lib.dva_interp_segment_reduce_fwd, lib.dva_interp_segment_reduce_bwd
    buf = ctypes.create_string_buffer(64)      # never dereferenced: every call below returns before a HIP call
    p = ctypes.cast(buf, ctypes.c_void_p)
    SUM, MEAN, MAX, MIN = _lib.DVA_SUM, _lib.DVA_MEAN, _lib.DVA_MAX, _lib.DVA_MIN
    # null pointers with S > 0
    assert fwd(None, None, None, None, None, None, 4, 8, 3, 16, _lib.DVA_F32, MEAN, None) == -1
    assert fwd(p, p, None, p, p, p, 4, 8, 3, 16, _lib.DVA_F32, MEAN, None) == -1          # no tap weights
    assert bwd(None, None, None, None, None, None, None, None, 4, 8, 3, 16, _lib.DVA_F32, SUM, None) == -1
    assert bwd(p, p, p, p, p, None, p, p, 4, 8, 3, 16, _lib.DVA_F32, SUM, None) == -1      # no tap weights
    for code in (MAX, MIN):                                                                # max / min without arg
        assert fwd(p, p, p, p, p, None, 4, 8, 3, 16, _lib.DVA_F32, code, None) == -1
        assert bwd(p, None, p, p, p, p, p, p, 4, 8, 3, 16, _lib.DVA_BF16, code, None) == -1
    # negative sizes
    for S, Pn, R, C in [(-1, 8, 3, 16), (4, -8, 3, 16), (4, 8, -3, 16), (4, 8, 3, -16)]:
        assert fwd(p, p, p, p, p, p, S, Pn, R, C, _lib.DVA_F32, SUM, None) == -1
        assert bwd(p, p, p, p, p, p, p, p, S, Pn, R, C, _lib.DVA_F32, SUM, None) == -1
    # unknown dtype / reduce code
    assert fwd(p, p, p, p, p, p, 4, 8, 3, 16, 7, SUM, None) == -1
    assert bwd(p, p, p, p, p, p, p, p, 4, 8, 3, 16, 7, SUM, None) == -1
    assert fwd(p, p, p, p, p, p, 4, 8, 3, 16, _lib.DVA_F32, 9, None) == -1
    assert bwd(p, p, p, p, p, p, p, p, 4, 8, 3, 16, _lib.DVA_F16, -1, None) == -1
    # 4 P, R or S of 2^31 or more
    for S, Pn, R in [(1 << 31, 8, 3), (4, 1 << 29, 3), (4, 8, 1 << 31)]:
        for code in (SUM, MAX):
            assert fwd(p, p, p, p, p, p, S, Pn, R, 16, _lib.DVA_F32, code, None) == -2
            assert bwd(p, p, p, p, p, p, p, p, S, Pn, R, 16, _lib.DVA_F32, code, None) == -2
    # nothing to do
    assert fwd(None, None, None, None, None, None, 0, 0, 3, 16, _lib.DVA_F32, SUM, None) == 0
    assert fwd(None, None, None, None, None, None, 4, 8, 3, 0, _lib.DVA_F32, MAX, None) == 0
    assert bwd(None, None, None, None, None, None, None, None, 4, 8, 0, 16, _lib.DVA_F32, SUM, None) == 0
    assert bwd(None, None, None, None, None, None, None, None, 4, 8, 3, 0, _lib.DVA_F32, MIN, None) == 0


def test_anchor_entries_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    asum, fix = lib.dva_interp_anchor_rows_sum, lib.dva_interp_anchor_fixup
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    SUM, MAX = _lib.DVA_SUM, _lib.DVA_MAX
    assert asum(None, None, None, None, None, None, None, None, 4, 8, 16, _lib.DVA_F32, SUM, None) == -1
    assert asum(p, None, p, p, p, p, p, p, 4, 8, 16, _lib.DVA_F32, MAX, None) == -1        # max without arg
    assert fix(None, None, None, None, None, None, None, None, None, 4, 8, 16, _lib.DVA_F32, SUM, None) == -1
    assert fix(p, None, p, p, p, p, p, p, p, 4, 8, 16, _lib.DVA_BF16, MAX, None) == -1     # max without arg
    for A, Pn, C in [(-1, 8, 16), (4, -8, 16), (4, 8, -16)]:
        assert asum(p, p, p, p, p, p, p, p, A, Pn, C, _lib.DVA_F32, SUM, None) == -1
        assert fix(p, p, p, p, p, p, p, p, p, A, Pn, C, _lib.DVA_F32, SUM, None) == -1
    assert asum(p, p, p, p, p, p, p, p, 4, 8, 16, 7, SUM, None) == -1
    assert fix(p, p, p, p, p, p, p, p, p, 4, 8, 16, _lib.DVA_F32, 9, None) == -1
    # fp16, sizes of 2^31 or more, and shapes the anchor kernel does not cover: the caller takes the tap plan
    assert asum(p, p, p, p, p, p, p, p, 4, 8, 16, _lib.DVA_F16, SUM, None) == -2
    assert fix(p, p, p, p, p, p, p, p, p, 4, 8, 16, _lib.DVA_F16, SUM, None) == -2
    assert asum(p, p, p, p, p, p, p, p, 1 << 31, 8, 16, _lib.DVA_F32, SUM, None) == -2
    assert asum(p, p, p, p, p, p, p, p, 4, 1 << 31, 16, _lib.DVA_F32, SUM, None) == -2
    for C, dt in [(13, _lib.DVA_F32), (24, _lib.DVA_F32), (24, _lib.DVA_BF16), (1024, _lib.DVA_BF16)]:
        assert asum(p, p, p, p, p, p, p, p, 4, 8, C, dt, SUM, None) == -2
    # nothing to do
    assert asum(None, None, None, None, None, None, None, None, 0, 8, 16, _lib.DVA_F32, SUM, None) == 0
    assert fix(None, None, None, None, None, None, None, None, None, 4, 0, 16, _lib.DVA_F32, SUM, None) == 0
    assert ops.INTERP_REDUCE_ANCHOR is True


def cpu_features(case, cls=ops.InterpolatedFeatures):
    """An ``InterpolatedFeatures`` over CPU tensors (no kernel ran: the taps are the numpy ones)."""
    feats = cls.__new__(cls)
    feats.x = feats.packed_idx = feats.coords = feats.parts = feats.order = feats.anchors = None
    feats.rows, feats.exact = case["rows"], False
    feats.tap_rows = torch.from_numpy(case["tap_rows"]).to(torch.int32)
    feats.tap_weights = torch.from_numpy(case["tap_weights"])
    feats.geometry = [IR.GEOMETRY[s] for s in case["settings"]]
    return feats


class CountingFeatures(ops.InterpolatedFeatures):
    """``InterpolatedFeatures`` that counts ``materialize`` calls (and interpolates with torch, so it works on the CPU)."""
    calls = 0

    def materialize(self, rows=None):
        CountingFeatures.calls += 1
        return (self.rows[self.tap_rows.long()].float() * self.tap_weights.unsqueeze(-1)).sum(1).to(self.rows.dtype)


@pytest.mark.parametrize("mode", REDUCES)
@pytest.mark.parametrize("level", ["view", "atom"])
def test_cpu_features_take_the_materialised_route(mode, level, monkeypatch):
    """A CPU ``x_mod`` is not served by the fused op: the module materialises and hands the tensor to ``segment_csr``
    (which, as every op of the package, then refuses the CPU tensor -- there is no CPU fallback)."""
    case = IR.make_case(16, torch.float32)
    feats = cpu_features(case, CountingFeatures)
    assert not ops.interp_segment_reduce_applicable(feats, case["ptr"], mode)
    monkeypatch.setattr(ops, "interp_segment_reduce", lambda *a, **k: pytest.fail("the fused op was called"))
    CountingFeatures.calls = 0
    x_map = torch.rand(case["P"], 8) if level == "view" else None
    with pytest.raises(_lib.DvaError):
        P.BimodalCSRPool(mode=mode)(None, feats, x_map, case["ptr"])
    assert CountingFeatures.calls == 1


def test_switch_and_what_the_op_serves(monkeypatch):
    """``ops.LAZY_INTERP_REDUCE`` is a plain module attribute; applicability is decided from type, device, dtype and
    sizes, and for max / min from the segment sizes through ``_atoms_per_view_ok``."""
    assert ops.LAZY_INTERP_REDUCE is True
    dev = lambda dtype, shape: types.SimpleNamespace(is_cuda=True, dtype=dtype, shape=torch.Size(shape),
                                                     dim=lambda: len(shape))

    def feats_of(dtype, R, C, n_items, cls=ops.InterpolatedFeatures):
        f = cls.__new__(cls)
        f.rows, f.tap_rows, f.tap_weights = dev(dtype, (R, C)), dev(torch.int32, (n_items, 4)), dev(torch.float32,
                                                                                                     (n_items, 4))
        f.parts = f.order = None
        return f
    asked = []
    monkeypatch.setattr(ops, "_atoms_per_view_ok", lambda ptr: asked.append(ptr) or True)
    ptr_ = dev(torch.int64, (11,))
    for dtype in DTYPES:
        for C in (1, 13, 64):
            feats = feats_of(dtype, 63, C, 40)
            for reduce in REDUCES:
                assert ops.interp_segment_reduce_applicable(feats, ptr_, reduce)
    assert len(asked) == 18 and all(a is ptr_ for a in asked), "max and min ask for the segment sizes, mean and sum do not"
    feats = feats_of(torch.float32, 63, 16, 40)
    cat = feats_of(torch.float32, 63, 16, 40)
    cat.parts, cat.order = [feats, feats], None
    assert ops.interp_segment_reduce_applicable(cat, ptr_, "mean")                          # a cat of settings
    assert not ops.interp_segment_reduce_applicable(feats, ptr_, "prod")
    assert not ops.interp_segment_reduce_applicable(feats_of(torch.float64, 63, 16, 40), ptr_, "mean")
    assert not ops.interp_segment_reduce_applicable(dev(torch.float32, (40, 16)), ptr_, "mean")      # a plain tensor
    assert not ops.interp_segment_reduce_applicable(ops.GatheredFeatures(dev(torch.float32, (63, 16)),
                                                                         dev(torch.int32, (40,)), None, False), ptr_, "mean")
    assert not ops.gather_segment_reduce_applicable(feats, ptr_, "mean")        # the nearest ops answer for their own type
    assert not ops.gather_segment_reduce_applicable(feats, ptr_, "max")
    # the limits: 4 P, R, S below 2^31
    assert ops.interp_segment_reduce_applicable(feats_of(torch.float32, 63, 16, (1 << 29) - 1), ptr_, "sum")
    assert not ops.interp_segment_reduce_applicable(feats_of(torch.float32, 63, 16, 1 << 29), ptr_, "sum")
    assert not ops.interp_segment_reduce_applicable(feats_of(torch.float32, 1 << 31, 16, 40), ptr_, "sum")
    assert not ops.interp_segment_reduce_applicable(feats, dev(torch.int64, ((1 << 31) + 1,)), "sum")
    # segments above 65534 items: max and min only
    monkeypatch.setattr(ops, "_atoms_per_view_ok", lambda ptr: False)
    assert not ops.interp_segment_reduce_applicable(feats, ptr_, "max")
    assert not ops.interp_segment_reduce_applicable(feats, ptr_, "min")
    assert ops.interp_segment_reduce_applicable(feats, ptr_, "mean") and ops.interp_segment_reduce_applicable(feats, ptr_, "sum")
    monkeypatch.setattr(ops, "LAZY_INTERP_REDUCE", False)
    assert not ops.interp_segment_reduce_applicable(feats, ptr_, "mean")
    with pytest.raises(ValueError):
        ops.interp_segment_reduce(feats, ptr_, "prod")
    with pytest.raises(ValueError):
        ops.interp_segment_reduce(feats, ptr_, "mean", level="point")
    with pytest.raises(TypeError):
        ops.interp_segment_reduce(dev(torch.float32, (40, 16)), ptr_, "mean")
