"""CPU tests of the multi-part sparse-convolution entries (``dva_sparse_conv_apply_parts``, ``_apply_packed_parts``,
``_wgrad_parts``): every refusal comes before any HIP call, in the order of the single-tensor entries; and of the lazy
``snn.cat`` that carries the parts (pure tensor bookkeeping, no kernel)."""
import ctypes

import pytest
import torch

from deepviewagg_amd import _lib, ops
from deepviewagg_amd.modules.SparseConv3d import ResNetUp
from deepviewagg_amd.modules.SparseConv3d import nn as snn

_BUF = ctypes.create_string_buffer(512)
_P = (ctypes.addressof(_BUF) + 15) & ~15    # a 16-byte aligned non-null pointer: the host side never dereferences it
_BIG = 1 << 40                              # a size that passes every size check
F32, BF16, F16 = _lib.DVA_F32, _lib.DVA_BF16, _lib.DVA_F16
_DEFAULT = object()


def _table(parts, widths):
    """The two host arrays of an entry; ``parts`` = None passes a null table."""
    w = None if widths is None else (ctypes.c_int32 * max(1, len(widths)))(*widths)
    p = None if parts is None else (ctypes.c_void_p * max(1, len(parts)))(*parts)
    return p, w


def _apply(parts=_DEFAULT, widths=(16, 32), P=None, nbr=_P, W=_P, bias=None, out=_P + 64, n_src=4, n_dst=4, K=27, cout=16,
           dtype=F32, ws=_P + 128, nbytes=_BIG):
    parts = [_P + 32 * i for i in range(len(widths or ()))] if parts is _DEFAULT else parts
    p, w = _table(parts, widths)
    return _lib.load().dva_sparse_conv_apply_parts(p, w, len(widths) if P is None else P, nbr, W, bias, out, n_src, n_dst,
                                                   K, cout, dtype, ws, nbytes, None)


def _packed(parts=_DEFAULT, widths=(16, 32), P=None, nbr=_P, packed=_P + 128, nbytes=_BIG, bias=None, residual=None,
            slope=0.0, out=_P + 64, n_src=4, n_dst=4, K=27, cout=16, dtype=F32):
    parts = [_P + 32 * i for i in range(len(widths or ()))] if parts is _DEFAULT else parts
    p, w = _table(parts, widths)
    return _lib.load().dva_sparse_conv_apply_packed_parts(p, w, len(widths) if P is None else P, nbr, packed, nbytes, bias,
                                                          residual, slope, out, n_src, n_dst, K, cout, dtype, None)


def _wgrad(parts=_DEFAULT, widths=(16, 32), P=None, nbr=_P, gout=_P + 64, gW=_P + 128, n_src=4, n_dst=4, K=27, cout=16,
           dtype=F32):
    parts = [_P + 32 * i for i in range(len(widths or ()))] if parts is _DEFAULT else parts
    p, w = _table(parts, widths)
    return _lib.load().dva_sparse_conv_wgrad_parts(p, w, len(widths) if P is None else P, nbr, gout, gW, n_src, n_dst, K,
                                                   cout, dtype, None)


def test_version_has_the_parts_entries():
    assert _lib.load().dva_version() >= 333


@pytest.mark.parametrize("call", [_apply, _packed, _wgrad], ids=["apply_parts", "apply_packed_parts", "wgrad_parts"])
def test_parts_entries_refuse_before_any_device_call(call):
    assert call(dtype=F16) == -2                                    # no fp16 sparse convolution
    assert call(dtype=F16, widths=(8, 32), parts=None) == -2        # dtype before widths before pointers
    for code in (3, -1):
        assert call(dtype=code) == -1
    assert call(widths=(), P=0) == -1                               # P = 0
    assert call(widths=(16,) * 5) == -2                             # P = 5
    assert call(widths=(16,) * 5, dtype=F16) == -2
    assert call(widths=None, P=2) == -1                             # no widths to read
    assert call(widths=(16, 8)) == -2 and call(widths=(8,)) == -2   # a width of 8: the host pads a narrow part
    assert call(widths=(16, 0)) == -1 and call(widths=(-16, 32)) == -1
    assert call(cout=24) == -2 and call(cout=0) == -1 and call(K=0) == -1
    assert call(n_src=-1) == -1 and call(n_dst=-1) == -1
    assert call(n_src=1 << 31) == -2 and call(n_dst=(0x7fffffff // 27) + 1) == -2    # 32-bit row indices
    for P in (1, 2, 3, 4):                                          # every supported count reaches the later checks
        assert call(widths=(16,) * P, n_src=1 << 31) == -2 and call(widths=(16,) * (P - 1) + (24,)) == -2


@pytest.mark.parametrize("call", [_apply, _packed], ids=["apply_parts", "apply_packed_parts"])
def test_apply_entries_refuse_bad_pointers_and_sizes(call):
    assert call(n_dst=0, parts=None, nbr=None, out=None) == 0       # nothing to write: DVA_OK before any pointer is read
    assert call(parts=None) == -1                                   # null table
    assert call(parts=[_P, None]) == -1 and call(parts=[None, _P]) == -1            # a null part
    assert call(parts=[_P, _P + 8]) == -1 and call(parts=[_P + 4, _P]) == -1        # a misaligned part
    assert call(parts=[_P, _P + 32, _P + 2], widths=(16, 16, 16)) == -1
    assert call(nbr=None) == -1 and call(out=None) == -1 and call(out=_P + 4) == -1
    assert call(n_src=0) == -1                                      # masked lanes read row 0 of every part: it must exist
    need = _lib.load().dva_sparse_conv_workspace_bytes(27, 48, 16, F32)
    assert need > 0 and call(nbytes=need - 1) == -1                 # too small a packed buffer / workspace
    assert call(nbytes=_lib.load().dva_sparse_conv_workspace_bytes(27, 48, 16, BF16), dtype=F32) == -1
    assert call(widths=(16, 32, 64), nbytes=need) == -1             # sized for 48 input channels, not 112


def test_apply_packed_parts_keeps_the_rules_of_the_fused_epilogue():
    assert _packed(slope=float("nan")) == -1 and _packed(slope=float("inf")) == -1
    assert _packed(residual=_P + 64) == -1                          # residual aliases out
    assert _packed(residual=_P + 8) == -1 and _packed(packed=None) == -1 and _packed(packed=_P + 8) == -1


def test_apply_parts_needs_weights_and_a_workspace():
    assert _apply(W=None) == -1 and _apply(ws=None) == -1 and _apply(ws=_P + 8) == -1


def test_wgrad_parts_refuses_a_null_gradient_before_the_first_launch():
    assert _wgrad(gW=None) == -1
    assert _wgrad(gW=None, n_dst=0) == -1 and _wgrad(gW=None, dtype=F16) == -2


# ---- ops: argument checks that need no device ----------------------------------------------------------------------

def test_ops_refuse_a_cpu_list_and_more_parts_than_the_kernels_take():
    assert ops.SPARSE_CONV_MAX_PARTS == 4
    nbr = torch.zeros(27, 3, dtype=torch.int32)
    with pytest.raises(_lib.DvaError):                              # no CPU path, for a list as for a tensor
        ops.sparse_conv([torch.zeros(3, 16), torch.zeros(3, 16)], torch.zeros(27, 32, 16), None, nbr, nbr)
    with pytest.raises(ValueError):
        ops.sparse_conv([torch.zeros(3, 16)] * 5, torch.zeros(27, 80, 16), None, nbr, nbr)
    with pytest.raises(ValueError):
        ops.sparse_conv([torch.zeros(3, 16), torch.zeros(4, 16)], torch.zeros(27, 32, 16), None, nbr, nbr)
    with pytest.raises(ValueError):
        ops.sparse_conv([], torch.zeros(27, 32, 16), None, nbr, nbr)


# ---- the lazy cat ----------------------------------------------------------------------------------------------------

def _voxels(n, c, seed):
    gen = torch.Generator().manual_seed(seed)
    coords = torch.cat([torch.arange(n).reshape(-1, 1).repeat(1, 3), torch.zeros(n, 1, dtype=torch.long)], 1).int()
    return snn.SparseVoxelTensor(torch.randn(n, c, generator=gen), coords)


def test_lazy_cat_is_the_cat_on_first_read_and_only_then():
    a = _voxels(9, 4, 0)
    b = a.like(torch.randn(9, 7, generator=torch.Generator().manual_seed(1)))
    eager = snn.cat(a, b)
    assert type(eager) is snn.SparseVoxelTensor and snn.LAZY_CAT is False      # the default route is today's
    lazy = snn.cat(a, b, lazy=True)
    assert isinstance(lazy, snn.LazyCatTensor) and isinstance(lazy, snn.SparseVoxelTensor)
    assert lazy.parts[0] is a.F and lazy.parts[1] is b.F and lazy._feats is None and lazy.num_channels == 11
    assert lazy.C is a.C and lazy.s == a.s and lazy.coord_maps is a.coord_maps and lazy.kernel_maps is a.kernel_maps
    f = lazy.F
    assert torch.equal(f, eager.F) and lazy.F is f                  # bit for bit, cached
    assert snn.feature_parts(lazy) is lazy.parts and snn.feature_parts(eager) is None
    lazy.F = f * 2                                                  # assigning F drops the parts
    assert lazy.parts is None and snn.feature_parts(lazy) is None and torch.equal(lazy.F, f * 2) and lazy.num_channels == 11
    # consumers that know nothing of parts: like, +, ReLU
    lazy = snn.cat(a, b, lazy=True)
    assert type(lazy.like(f)) is snn.SparseVoxelTensor
    assert torch.equal((lazy + eager).F, eager.F + eager.F)
    assert torch.equal(snn.ReLU()(lazy).F, torch.relu(eager.F))


def test_lazy_cat_flattens_nested_parts_and_obeys_the_module_switch(monkeypatch):
    a, = (_voxels(5, 3, 2),)
    b, c = a.like(torch.ones(5, 2)), a.like(torch.full((5, 1), 2.0))
    inner = snn.cat(a, b, lazy=True)
    outer = snn.cat(inner, c, lazy=True)
    assert len(outer.parts) == 3 and torch.equal(outer.F, torch.cat([a.F, b.F, c.F], 1))
    five = snn.cat(a, b, c, a, b, lazy=True)                        # more parts than the kernels take: read through F
    assert len(five.parts) == 5 and snn.feature_parts(five) is None
    assert torch.equal(five.F, torch.cat([a.F, b.F, c.F, a.F, b.F], 1))
    monkeypatch.setattr(snn, "LAZY_CAT", True)
    assert isinstance(snn.cat(a, b), snn.LazyCatTensor) and type(snn.cat(a, b, lazy=False)) is snn.SparseVoxelTensor


def test_1x1x1_convolution_on_parts_is_the_sum_of_per_part_gemms():
    a = _voxels(33, 6, 3)
    b = a.like(torch.randn(33, 10, generator=torch.Generator().manual_seed(4)))
    conv = snn.Conv3d(16, 12, kernel_size=1, bias=True)
    eager, lazy = conv(snn.cat(a, b)), conv(snn.cat(a, b, lazy=True))
    assert type(lazy) is snn.SparseVoxelTensor and lazy.F.shape == (33, 12)
    torch.testing.assert_close(lazy.F, eager.F, rtol=1e-5, atol=1e-5)     # two fp32 GEMMs summed against one
    eager.F.sum().backward()
    g = conv.kernel.grad.clone()
    conv.kernel.grad = None
    lazy.F.sum().backward()
    torch.testing.assert_close(conv.kernel.grad, g, rtol=1e-5, atol=1e-5)


def test_the_switch_moves_no_state_dict_key(monkeypatch):
    keys = list(ResNetUp(up_conv_nn=[32, 16, 24], N=1).state_dict())
    monkeypatch.setattr(snn, "LAZY_CAT", True)
    assert list(ResNetUp(up_conv_nn=[32, 16, 24], N=1).state_dict()) == keys


def test_the_cat_benchmark_is_built_on_measure(capsys):
    import importlib
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    text = open(os.path.join(ROOT, "tools", "sparse_cat_bench.py")).read()
    for word in ("torch.cuda.Event(", "perf_counter", "set_sync_debug_mode", "reset_peak_memory_stats",
                 "TorchDispatchMode"):
        assert word not in text
    assert "measure.alternate(" in text and "measure.profile_once(" in text and "measure.emit(" in text
    device_in_use = torch.cuda.is_initialized()                     # by an earlier test of the same process, if at all
    module = importlib.import_module("sparse_cat_bench")
    with pytest.raises(SystemExit) as stop:
        module.main(["--help"])
    assert stop.value.code == 0 and "--reps" in capsys.readouterr().out
    assert torch.cuda.is_initialized() == device_in_use             # importing the tool and its help need no device
    assert set(module.arms()) == {"fusion_4_512_128_fwd", "fusion_4_512_128_fwd_bwd", "decoder_join_resblock",
                                  "decoder_join_folded", "resnet_down_up_pair"}
    assert snn.LAZY_CAT is False                                    # importing the tool flips nothing
