"""CPU tests of the folded sparse-convolution inference path: the two packed C-ABI entries validate their arguments
before any HIP call, ``folded_weights`` is the float64 formula rounded to fp32 once, and ``fold_for_inference``
rewrites the tree where stated and nowhere else."""
import copy
import ctypes

import pytest
import torch

from deepviewagg_amd import _lib
from deepviewagg_amd.modules.SparseConv3d import (BottleneckBlock, FoldedConv, FoldedResidual, ResBlock, ResNetDown,
                                                  ResNetUp, fold_for_inference, folded_weights)
from deepviewagg_amd.modules.SparseConv3d import nn as snn

_BUF = ctypes.create_string_buffer(256)
_P = (ctypes.addressof(_BUF) + 15) & ~15    # a 16-byte aligned non-null pointer: the host side never dereferences it
_BIG = 1 << 40                              # a size that passes every size check
F32, BF16, F16 = _lib.DVA_F32, _lib.DVA_BF16, _lib.DVA_F16


def _pack(W=_P, K=27, cin=16, cout=16, mode=0, dtype=F32, packed=_P, nbytes=_BIG):
    return _lib.load().dva_sparse_conv_pack_weights(W, K, cin, cout, mode, dtype, packed, nbytes, None)


def _apply(x=_P, nbr=_P, packed=_P, nbytes=_BIG, bias=_P, residual=None, slope=0.0, out=_P + 64, n_src=4, n_dst=4,
           K=27, cin=16, cout=16, dtype=F32):
    return _lib.load().dva_sparse_conv_apply_packed(x, nbr, packed, nbytes, bias, residual, slope, out, n_src, n_dst,
                                                    K, cin, cout, dtype, None)


def test_version_has_the_packed_entries():
    assert _lib.load().dva_version() >= 332


@pytest.mark.parametrize("call", [_pack, _apply], ids=["pack_weights", "apply_packed"])
def test_packed_entries_validate_without_a_device(call):
    need = _lib.load().dva_sparse_conv_workspace_bytes(27, 16, 16, F32)
    assert need == 442368
    for code in (3, -1):
        assert call(dtype=code) == -1                               # unknown dtype code
    assert call(dtype=F16) == -2                                    # a known code without kernels
    assert call(cin=8) == -2 and call(cout=24) == -2                # the host pads the channel counts to 16
    assert call(dtype=F16, cin=8, packed=None) == -2                # dtype before channels before pointers
    assert call(dtype=3, cin=8) == -1
    assert call(K=0) == -1 and call(cin=0) == -1 and call(cout=-16) == -1
    assert call(packed=None) == -1                                  # null packed buffer
    assert call(packed=_P + 8) == -1                                # misaligned packed buffer
    assert call(nbytes=need - 1) == -1                              # short packed_bytes
    assert call(nbytes=_lib.load().dva_sparse_conv_workspace_bytes(27, 16, 16, BF16), dtype=F32) == -1


def test_pack_weights_rejects_a_bad_mode_and_a_null_source():
    assert _pack(mode=2) == -1 and _pack(mode=-1) == -1
    assert _pack(W=None) == -1


def test_apply_packed_rejects_bad_rows_without_a_device():
    assert _apply(residual=_P + 4) == -1 and _apply(residual=_P + 8, dtype=BF16) == -1   # misaligned residual
    assert _apply(residual=_P + 64) == -1                           # residual aliases out
    assert _apply(out=_P + 4) == -1 and _apply(x=_P + 2) == -1      # misaligned out / x
    assert _apply(out=None) == -1 and _apply(nbr=None) == -1 and _apply(x=None) == -1
    assert _apply(n_src=-1) == -1 and _apply(n_dst=-1) == -1
    assert _apply(slope=float("nan")) == -1 and _apply(slope=float("inf")) == -1
    assert _apply(n_src=1 << 31) == -2 and _apply(n_dst=(0x7fffffff // 27) + 1) == -2    # 32-bit row indices
    assert _apply(n_src=0) == -1                                    # masked lanes read row 0: it must exist
    assert _apply(n_dst=0, packed=None) == 0                        # nothing to write: as dva_sparse_conv_apply


def test_the_fold_benchmark_is_built_on_measure(capsys):
    """tools/sparse_fold_bench.py meets what tests/test_measure_host.py asks of the side benchmarks: clocks and counters
    are measure.py's, the two routes go through ``alternate``, and ``--help`` needs no device."""
    import importlib
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    text = open(os.path.join(ROOT, "tools", "sparse_fold_bench.py")).read()
    for word in ("torch.cuda.Event(", "perf_counter", "set_sync_debug_mode", "reset_peak_memory_stats",
                 "TorchDispatchMode"):
        assert word not in text
    assert "measure.alternate(" in text and "measure.profile_once(" in text and "measure.emit(" in text
    module = importlib.import_module("sparse_fold_bench")
    with pytest.raises(SystemExit) as stop:
        module.main(["--help"])
    assert stop.value.code == 0 and "--reps" in capsys.readouterr().out
    assert not torch.cuda.is_initialized()
    assert set(module.arms()) == {"resblock_64_64", "resblock_64_128_shortcut", "resnet_down_up_pair"}


# ---- folded_weights ----------------------------------------------------------------------------------------------

def _random_bn(c, affine=True, seed=0):
    gen = torch.Generator().manual_seed(seed)
    bn = snn.BatchNorm(c)
    if not affine:
        bn.bn = snn._RowBatchNorm(num_features=c, affine=False)
    with torch.no_grad():
        bn.bn.running_mean.copy_(torch.randn(c, generator=gen))
        bn.bn.running_var.copy_(torch.rand(c, generator=gen) * 3 + 0.05)
        if affine:
            bn.bn.weight.copy_(torch.randn(c, generator=gen))
            bn.bn.bias.copy_(torch.randn(c, generator=gen))
    return bn.eval()


@pytest.mark.parametrize("conv_cls,k,bias,affine", [
    (snn.Conv3d, 3, True, True), (snn.Conv3d, 3, False, True), (snn.Conv3d, 1, True, False),
    (snn.Conv3d, 2, False, False), (snn.Conv3dTranspose, 2, True, True), (snn.Conv3dTranspose, 3, False, False)])
def test_folded_weights_are_the_float64_formula_rounded_once(conv_cls, k, bias, affine):
    torch.manual_seed(k + bias + 2 * affine)
    conv = conv_cls(12, 20, kernel_size=k, stride=2 if k == 2 else 1, bias=bias)
    bn = _random_bn(20, affine, seed=k)
    W, b = folded_weights(conv, bn)
    inner = bn.bn
    weight = inner.weight.double() if affine else torch.ones(20, dtype=torch.float64)
    g = weight / torch.sqrt(inner.running_var.double() + inner.eps)
    cb = conv.bias.double() if bias else torch.zeros(20, dtype=torch.float64)
    bb = inner.bias.double() if affine else torch.zeros(20, dtype=torch.float64)
    W_ref = (conv.kernel.double() * g).float()                      # the output channels are the last axis
    b_ref = ((cb - inner.running_mean.double()) * g + bb).float()
    assert W.dtype == torch.float32 and W.shape == conv.kernel.shape and torch.equal(W, W_ref)
    assert b.dtype == torch.float32 and b.shape == (20,) and torch.equal(b, b_ref)
    assert torch.equal(folded_weights(conv, inner)[0], W)           # the inner BatchNorm1d is accepted too
    assert not W.requires_grad and not b.requires_grad


def test_folded_weights_need_running_statistics():
    bn = snn.BatchNorm(8)
    bn.bn = snn._RowBatchNorm(num_features=8, track_running_stats=False)
    with pytest.raises(ValueError):
        folded_weights(snn.Conv3d(4, 8), bn.eval())
    stage = ResNetDown(down_conv_nn=[4, 8], N=0).eval()
    stage.conv_in[1].bn = snn._RowBatchNorm(num_features=8, track_running_stats=False).eval()
    with pytest.raises(ValueError):
        fold_for_inference(stage)


# ---- fold_for_inference ------------------------------------------------------------------------------------------

class _Other(torch.nn.Module):
    """A branch that is not a sparse-convolution run: it must come through unchanged."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 4)
        self.norm = torch.nn.BatchNorm1d(4)


class _Net(torch.nn.Module):
    def __init__(self, block):
        super().__init__()
        self.down = ResNetDown(down_conv_nn=[16, 32], N=2, block=block)
        self.up = ResNetUp(up_conv_nn=[32, 16, 24], N=1, block=block)
        self.head = snn.Seq().append(snn.Conv3d(24, 8, kernel_size=1, bias=True)).append(snn.ReLU())   # no BatchNorm
        self.other = _Other()


def _kinds(seq):
    return [type(m).__name__ for m in seq]


@pytest.mark.parametrize("block", ["ResBlock", "BottleneckBlock"])
def test_fold_rewrites_the_tree_where_stated_and_leaves_the_argument_alone(block):
    torch.manual_seed(0)
    net = _Net(block).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_()
            m.running_var.uniform_(0.5, 2.0)
    before = copy.deepcopy(net.state_dict())
    folded = fold_for_inference(net)
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not any(isinstance(m, (FoldedConv, FoldedResidual)) for m in net.modules())
    assert not net.training and not any(m.training for m in folded.modules())

    assert type(folded.down) is ResNetDown and type(folded.up) is ResNetUp
    assert _kinds(folded.down.conv_in) == ["FoldedConv"] and _kinds(folded.up.conv_in) == ["FoldedConv"]
    assert folded.down.conv_in[0].slope == 0.0 and not folded.down.conv_in[0].t and folded.up.conv_in[0].t
    assert folded.up.conv_in[0].stride == 2 and folded.up.conv_in[0].weight.shape == (8, 32, 32)
    assert _kinds(folded.down.blocks) == ["FoldedResidual"] * 2 and _kinds(folded.up.blocks) == ["FoldedResidual"]
    n_convs = 2 if block == "ResBlock" else 3
    for twin, has_shortcut in ((folded.down.blocks[0], True), (folded.down.blocks[1], False),
                               (folded.up.blocks[0], True)):
        assert twin.kind == block and _kinds(twin.block) == ["FoldedConv"] * n_convs
        assert all(c.slope == 0.0 for c in twin.block)              # the ReLU sits inside the block, before the sum
        assert (twin.downsample is not None) == has_shortcut
        if has_shortcut:
            assert _kinds(twin.downsample) == ["FoldedConv"] and twin.downsample[0].slope == 1.0
            assert twin.downsample[0].kernel_volume == 1 and twin.downsample[0].weight.dim() == 3
    # the folded buffers are folded_weights of the argument's layers
    W, b = folded_weights(net.down.conv_in[0], net.down.conv_in[1])
    assert torch.equal(folded.down.conv_in[0].weight, W) and torch.equal(folded.down.conv_in[0].bias, b)
    W, b = folded_weights(net.down.blocks[0].downsample[0], net.down.blocks[0].downsample[1])
    assert torch.equal(folded.down.blocks[0].downsample[0].weight, W.unsqueeze(0))
    assert torch.equal(folded.down.blocks[0].downsample[0].bias, b)
    # unchanged elsewhere: a convolution without a BatchNorm behind it, and modules that are no sparse convolution
    assert _kinds(folded.head) == ["Conv3d", "ReLU"] and type(folded.other) is _Other
    assert folded.head[0] is not net.head[0] and torch.equal(folded.head[0].kernel, net.head[0].kernel)
    assert {k: v for k, v in folded.other.state_dict().items()}.keys() == net.other.state_dict().keys()
    assert all(torch.equal(v, net.other.state_dict()[k]) for k, v in folded.other.state_dict().items())


def test_fold_refuses_training_mode_and_the_result_refuses_train():
    net = _Net("ResBlock")
    with pytest.raises(ValueError):
        fold_for_inference(net)                                     # a fresh module is in training mode
    net.eval()
    net.down.blocks[0].train()
    with pytest.raises(ValueError):
        fold_for_inference(net)                                     # so is a part of it
    folded = fold_for_inference(net.eval())
    for module in (folded, folded.down, folded.down.conv_in[0], folded.down.blocks[0]):
        with pytest.raises(RuntimeError):
            module.train()
        with pytest.raises(RuntimeError):
            module.train(True)
    assert folded.eval() is folded and not any(m.training for m in folded.modules())
    assert fold_for_inference(net.down.blocks[0]).kind == "ResBlock"          # a block or a Seq may be the root
    assert _kinds(fold_for_inference(net.down.conv_in)) == ["FoldedConv"]
