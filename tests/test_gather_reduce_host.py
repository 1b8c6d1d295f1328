"""CPU tests of the fused gather + max / mean / sum / min pool: the numpy restatement of the forward against the torch
composition, the float64 gradient against autograd, the argument checks of the two C entries, and the fall-through of
``BimodalCSRPool`` to the materialised route (no GPU needed)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import gather_reduce_ref as GR
from deepviewagg_amd import _lib, ops
from deepviewagg_amd.modules.multimodal import pooling as P

REDUCES = ["max", "mean", "sum", "min"]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def torch_composition(rows, row_idx, ptr, reduce):
    """``segment_csr(rows[row_idx], ptr, reduce)`` segment by segment and item by item in torch: fp32 accumulation in item
    order, one rounding by torch's own cast."""
    x = rows[row_idx.long()].float()
    S, C = ptr.shape[0] - 1, x.shape[1]
    out = torch.zeros(S, C)
    arg = torch.full((S, C), 0xffff, dtype=torch.int64)
    for s in range(S):
        beg, end = int(ptr[s]), int(ptr[s + 1])
        acc = torch.zeros(C)
        for a in range(beg, end):
            if reduce in GR.EXTREMA:
                better = (x[a] > acc if reduce == "max" else x[a] < acc) if a > beg else torch.ones(C, dtype=torch.bool)
                acc = torch.where(better, x[a], acc)
                arg[s] = torch.where(better, torch.full_like(arg[s], a - beg), arg[s])
            else:
                acc = acc + x[a]
        if reduce == "mean" and end > beg:
            acc = acc / torch.tensor(float(end - beg), dtype=torch.float32)
        out[s] = acc
    return out.to(rows.dtype), arg


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [1, 13, 16])
def test_forward_restatement_equals_the_torch_composition(C, dtype):
    case = GR.make_case(C, dtype)
    sizes = (case["ptr"][1:] - case["ptr"][:-1]).tolist()
    assert sizes[0] == 0 and sizes[-1] == 0 and {1, 2, 70, 300} <= set(sizes)
    hits = torch.bincount(case["row_idx"].long(), minlength=GR.R_ROWS)
    assert int(hits[GR.HOT_ROW]) >= 300 and all(int(hits[r]) == 0 for r in GR.COLD_ROWS)
    for reduce in REDUCES:
        out, arg = GR.forward_ref(GR.stored(case["rows"]), case["row_idx"].numpy(), case["ptr"].numpy(), reduce, dtype)
        want, want_arg = torch_composition(case["rows"], case["row_idx"], case["ptr"], reduce)
        assert np.array_equal(out, GR.stored(want)), reduce
        if reduce in GR.EXTREMA:
            assert np.array_equal(arg.astype(np.int64), want_arg.numpy())
            ties = sum(int((case["rows"][case["row_idx"][b:e].long()].float().sort(0, descending=reduce == "max")
                            .values[:2].diff(dim=0) == 0).sum())
                       for b, e in zip(case["ptr"][:-1].tolist(), case["ptr"][1:].tolist()) if e - b >= 2)
            assert ties > 0, "the case holds no duplicated extremum: the first-item rule is not exercised"
        else:
            assert arg is None


def test_bf16_rounding_of_the_restatement_is_torchs():
    gen = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=gen) * 10 ** torch.randint(-6, 6, (4096,), generator=gen).float(),
                   torch.tensor([0.0, -0.0, 1.00390625, 1.01171875, 3.3895314e38, float("inf"), 1e-40])])
    assert np.array_equal(GR.round_to(x.numpy(), torch.bfloat16), x.bfloat16().float().numpy())
    assert np.array_equal(GR.round_to(x.numpy(), torch.float16), x.half().float().numpy())


@pytest.mark.parametrize("reduce", REDUCES)
def test_float64_references_agree_with_autograd(reduce):
    case = GR.make_case(13, torch.float32, seed=1)
    rows, idx, ptr = case["rows"].double().requires_grad_(), case["row_idx"].long(), case["ptr"]
    x = rows[idx]
    outs = []
    for b, e in zip(ptr[:-1].tolist(), ptr[1:].tolist()):
        seg = x[b:e]
        if e == b:
            outs.append(torch.zeros(x.shape[1], dtype=torch.float64))
        else:
            outs.append({"sum": lambda: seg.sum(0), "mean": lambda: seg.mean(0), "min": lambda: seg.amin(0),
                         "max": lambda: seg.amax(0)}[reduce]())
    out = torch.stack(outs)
    out64, arg = GR.forward_f64(GR.stored(case["rows"]), idx.numpy(), ptr.numpy(), reduce)
    assert np.allclose(out64, out.detach().numpy(), rtol=1e-14, atol=0)
    if reduce not in GR.EXTREMA:      # amax / amin spread the gradient over ties; the kernels (and segment_csr) give it to the first
        (g,) = torch.autograd.grad((out * case["gout"].double()).sum(), rows)
        g64 = GR.backward_f64(GR.stored(case["gout"]), idx.numpy(), ptr.numpy(), reduce, arg, GR.R_ROWS)
        assert np.allclose(g64, g.numpy(), rtol=1e-13, atol=1e-13)
    else:
        g64 = GR.backward_f64(GR.stored(case["gout"]), idx.numpy(), ptr.numpy(), reduce, arg, GR.R_ROWS)
        live = (ptr[1:] > ptr[:-1]).numpy()
        assert np.allclose(g64.sum(0), GR.stored(case["gout"]).astype(np.float64)[live].sum(0), rtol=1e-12, atol=1e-12)
        assert all(float(np.abs(g64[r]).max()) == 0.0 for r in GR.COLD_ROWS)


def test_entries_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.dva_version() >= 331
    fwd, bwd = lib.dva_gather_segment_reduce_fwd, lib.dva_gather_segment_reduce_bwd
    buf = ctypes.create_string_buffer(64)      # never dereferenced: every call below returns before a HIP call
    p = ctypes.cast(buf, ctypes.c_void_p)
    SUM, MEAN, MAX, MIN = _lib.DVA_SUM, _lib.DVA_MEAN, _lib.DVA_MAX, _lib.DVA_MIN
    # null pointers with S > 0
    assert fwd(None, None, None, None, None, 4, 8, 3, 16, _lib.DVA_F32, MEAN, None) == -1
    assert fwd(p, p, p, p, None, 4, 8, 3, 16, _lib.DVA_F32, MIN, None) == -1           # min without arg
    assert fwd(p, p, p, p, None, 4, 8, 3, 16, _lib.DVA_F32, MAX, None) == -1           # max without arg
    assert bwd(None, None, None, None, None, None, None, 4, 8, 3, 16, _lib.DVA_F32, SUM, None) == -1
    assert bwd(p, None, p, p, p, p, p, 4, 8, 3, 16, _lib.DVA_BF16, MIN, None) == -1     # min without arg
    assert bwd(p, None, p, p, p, p, p, 4, 8, 3, 16, _lib.DVA_BF16, MAX, None) == -1     # max without arg
    # negative sizes
    for S, Pn, R, C in [(-1, 8, 3, 16), (4, -8, 3, 16), (4, 8, -3, 16), (4, 8, 3, -16)]:
        assert fwd(p, p, p, p, p, S, Pn, R, C, _lib.DVA_F32, SUM, None) == -1
        assert bwd(p, p, p, p, p, p, p, S, Pn, R, C, _lib.DVA_F32, SUM, None) == -1
    # unknown dtype / reduce code
    assert fwd(p, p, p, p, p, 4, 8, 3, 16, 7, SUM, None) == -1
    assert bwd(p, p, p, p, p, p, p, 4, 8, 3, 16, 7, SUM, None) == -1
    assert fwd(p, p, p, p, p, 4, 8, 3, 16, _lib.DVA_F32, 9, None) == -1
    assert bwd(p, p, p, p, p, p, p, 4, 8, 3, 16, _lib.DVA_F16, -1, None) == -1
    # sizes of 2^31 or more, under every mode (the max pool is served by these entries: nothing to do is 0, not -2)
    for S, Pn, R in [(1 << 31, 8, 3), (4, 1 << 31, 3), (4, 8, 1 << 31)]:
        for code in (SUM, MAX):
            assert fwd(p, p, p, p, p, S, Pn, R, 16, _lib.DVA_F32, code, None) == -2
            assert bwd(p, p, p, p, p, p, p, S, Pn, R, 16, _lib.DVA_F32, code, None) == -2
    assert fwd(p, p, p, p, p, 0, 8, 3, 16, _lib.DVA_F32, MAX, None) == 0
    assert bwd(p, p, p, p, p, p, p, 4, 8, 0, 16, _lib.DVA_F32, MAX, None) == 0
    # nothing to do
    assert fwd(None, None, None, None, None, 0, 0, 3, 16, _lib.DVA_F32, SUM, None) == 0
    assert bwd(None, None, None, None, None, None, None, 4, 8, 0, 16, _lib.DVA_F32, SUM, None) == 0


class CountingFeatures(ops.GatheredFeatures):
    """``GatheredFeatures`` that counts ``materialize`` calls (and gathers with torch, so that it works on the CPU)."""
    calls = 0

    def materialize(self):
        CountingFeatures.calls += 1
        return self.rows[self.row_idx.long()]


@pytest.mark.parametrize("mode", REDUCES)
@pytest.mark.parametrize("level", ["view", "atom"])
def test_cpu_features_take_the_materialised_route(mode, level, monkeypatch):
    """A CPU ``x_mod`` is not served by the fused op: the module materialises and hands the tensor to ``segment_csr``
    (which, as every op of the package, then refuses the CPU tensor -- there is no CPU fallback)."""
    case = GR.make_case(16, torch.float32)
    feats = CountingFeatures(case["rows"], case["row_idx"], None, False)
    assert not ops.gather_segment_reduce_applicable(feats, case["ptr"], mode)
    monkeypatch.setattr(ops, "gather_segment_reduce", lambda *a, **k: pytest.fail("the fused op was called"))
    CountingFeatures.calls = 0
    x_map = torch.rand(case["P"], 8) if level == "view" else None
    with pytest.raises(_lib.DvaError):
        P.BimodalCSRPool(mode=mode)(None, feats, x_map, case["ptr"])
    assert CountingFeatures.calls == 1


def test_lazy_reduce_switch_and_what_the_op_serves(monkeypatch):
    """``ops.LAZY_REDUCE`` and ``ops.LAZY_NONEXACT`` are plain module attributes; applicability is decided from device,
    dtype, shape and alignment alone, and ``lazy_pool_applicable`` adds the level: CPU stand-ins for device tensors."""
    assert ops.LAZY_REDUCE is True and ops.LAZY_NONEXACT is True

    def dev(dtype, shape, contiguous=True, address=4096):
        return types.SimpleNamespace(is_cuda=True, dtype=dtype, shape=torch.Size(shape), dim=lambda: len(shape),
                                     element_size=lambda: torch.empty(0, dtype=dtype).element_size(),
                                     is_contiguous=lambda: contiguous, data_ptr=lambda: address)

    def ptr_of(n_segments, ok=True):     # the verdict of ``_atoms_per_view_ok`` as a measured pointer tensor carries it
        t = dev(torch.int64, (n_segments + 1,))
        t._version, t._dva_atoms_ok = 0, (0, ok)
        return t

    feats_of = lambda dtype, C, **kw: ops.GatheredFeatures(dev(dtype, (96, C), **kw), dev(torch.int32, (40,)), None, False)
    ptr_ = ptr_of(10)
    for dtype in DTYPES:
        es = torch.empty(0, dtype=dtype).element_size()
        for C in (1, 13, 24, 64, 136):
            feats = feats_of(dtype, C)
            for mode in ("mean", "sum", "min"):
                assert ops.gather_segment_reduce_applicable(feats, ptr_, mode)
            # max keeps its narrower gate: rows of whole 16-byte chunks
            assert ops.gather_segment_reduce_applicable(feats, ptr_, "max") == (C * es % 16 == 0), (dtype, C)
    # max: a contiguous slice off the 16-byte grid materialises, non-contiguous rows (copied by the op) do not
    assert not ops.gather_segment_reduce_applicable(feats_of(torch.float32, 16, address=4100), ptr_, "max")
    assert ops.gather_segment_reduce_applicable(feats_of(torch.float32, 16, address=4100), ptr_, "min")
    assert ops.gather_segment_reduce_applicable(feats_of(torch.float32, 16, contiguous=False, address=4100), ptr_, "max")
    # uint16 arg offsets: a segment of more than 65534 items is not served under max and min
    feats = feats_of(torch.float32, 16)
    long_ = ptr_of(10, ok=False)
    assert [ops.gather_segment_reduce_applicable(feats, long_, m) for m in REDUCES] == [False, True, True, False]
    # sizes of 2^31 or more, under every mode
    huge = ops.GatheredFeatures(dev(torch.float32, (96, 16)), dev(torch.int32, (1 << 31,)), None, False)
    assert not any(ops.gather_segment_reduce_applicable(huge, ptr_, m) for m in REDUCES)
    assert not ops.gather_segment_reduce_applicable(ops.GatheredFeatures(dev(torch.float64, (96, 16)), None, None, False),
                                                    ptr_, "mean")
    assert not ops.gather_segment_reduce_applicable(dev(torch.float32, (40, 16)), ptr_, "mean")      # a plain tensor
    # the level: an atomic pool of a nearest gather is fused only where it shrinks it (S < P = 40); a view pool always
    for mode in REDUCES:
        assert ops.lazy_pool_applicable(feats, ptr_of(39), mode, atomic=True)
        assert not ops.lazy_pool_applicable(feats, ptr_of(40), mode, atomic=True)
        assert ops.lazy_pool_applicable(feats, ptr_of(40), mode, atomic=False)
        assert ops.lazy_pool_applicable(feats, ptr_of(400), mode, atomic=False)
    # what comes out: lazy rows under the identity gather at the atomic level, the plain tensor at the view level
    seen = []
    monkeypatch.setattr(ops, "gather_segment_reduce", lambda x, p, reduce, level="view": seen.append((reduce, level)))
    monkeypatch.setattr(ops, "interp_segment_reduce", lambda x, p, reduce, level="view": seen.append(("interp", level)))
    ops.lazy_pool(feats, ptr_, "max", atomic=True)
    ops.lazy_pool(feats, ptr_, "max", atomic=False)
    ops.lazy_pool(feats, ptr_, "min", atomic=True)
    taps = ops.InterpolatedFeatures.__new__(ops.InterpolatedFeatures)
    ops.lazy_pool(taps, ptr_, "max", atomic=True)
    ops.lazy_pool(taps, ptr_, "mean", atomic=False)
    assert seen == [("max", "atom"), ("max", "view"), ("min", "atom"), ("interp", "view"), ("interp", "view")]
    monkeypatch.undo()
    # the two switches: LAZY_NONEXACT the max pool, LAZY_REDUCE the others
    monkeypatch.setattr(ops, "LAZY_REDUCE", False)
    assert [ops.gather_segment_reduce_applicable(feats, ptr_, m) for m in REDUCES] == [True, False, False, False]
    monkeypatch.setattr(ops, "LAZY_REDUCE", True)
    monkeypatch.setattr(ops, "LAZY_NONEXACT", False)
    assert [ops.gather_segment_reduce_applicable(feats, ptr_, m) for m in REDUCES] == [False, True, True, True]
    assert not ops.lazy_pool_applicable(feats, ptr_, "max", atomic=False)
    with pytest.raises(ValueError):
        ops.gather_segment_reduce(feats, ptr_, "prod")
    with pytest.raises(ValueError):
        ops.gather_segment_reduce(feats, ptr_, "mean", level="point")
