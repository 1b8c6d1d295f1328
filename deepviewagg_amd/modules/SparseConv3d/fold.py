"""Inference form of the residual sparse-convolution stages: ``fold_for_inference(module)`` returns a copy in which
every convolution carries its BatchNorm (an affine map with constant coefficients in eval mode), its ReLU and, at the
end of a residual block, the shortcut sum in the epilogue of the convolution kernel
(``ops.sparse_conv_fused`` over weights packed once, ``csrc/sparseconv.hip``).  A ``ResBlock`` becomes two launches
(three with a ``downsample``) that write every output row once; the unfolded eval path runs the weight re-pack, the
convolution, the BatchNorm table and the BatchNorm row pass per layer, then a torch ``add``.

Folding arithmetic, in float64 and rounded to fp32 once: ``g = weight / sqrt(running_var + eps)``,
``W' = fp32(W * g)`` over the output-channel axis, ``b' = fp32((bias - running_mean) * g + bn.bias)``; a missing
convolution bias counts as 0, a non-affine BatchNorm as weight 1 and bias 0.

The folded modules have no training mode and no autograd; the argument of ``fold_for_inference`` is left as it is.
"""
import copy

import torch
from torch import nn

from ... import ops
from . import nn as snn
from .modules import _Residual

__all__ = ["FoldedConv", "FoldedResidual", "fold_for_inference", "folded_weights"]


def folded_weights(conv, bn):
    """``(W', b')`` of ``bn(conv(x))`` in eval mode: fp32 tensors shaped as ``conv.kernel`` and ``[Cout]``, on the
    device of the parameters (CPU tensors work).  ``bn``: ``snn.BatchNorm`` or the ``BatchNorm1d`` inside it."""
    bn = bn.bn if isinstance(bn, snn.BatchNorm) else bn
    if bn.running_mean is None or bn.running_var is None:
        raise ValueError("fold_for_inference needs the running statistics of every BatchNorm "
                         "(track_running_stats=False leaves none to fold)")
    weight = torch.ones_like(bn.running_var, dtype=torch.float64) if bn.weight is None else bn.weight.detach().double()
    g = weight / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    W = (conv.kernel.detach().double() * g).float()
    b = -bn.running_mean.detach().double() if conv.bias is None else \
        conv.bias.detach().double() - bn.running_mean.detach().double()
    b = b * g
    if bn.bias is not None:
        b = b + bn.bias.detach().double()
    return W, b.float()


class _Frozen(nn.Module):
    """A module without a training mode."""

    def __init__(self):
        super().__init__()
        self.training = False

    def train(self, mode=True):
        if mode:
            raise RuntimeError(f"{type(self).__name__} is an inference-only module (fold_for_inference): "
                               "train the unfolded modules and fold again")
        return super().train(False)


class FoldedConv(_Frozen):
    """``Conv3d`` / ``Conv3dTranspose`` -> ``BatchNorm`` [-> ``ReLU``] as one launch:
    ``out = leaky(conv(x; W') + b', slope) [+ residual]``.  ``weight`` [K, Cin, Cout] and ``bias`` [Cout] are buffers;
    the packed operand of the kernel is built on the first forward on a device and kept per (device, feature dtype,
    part widths of a lazy concatenation or None).
    A 1x1x1 stride-1 layer runs the same kernel with K = 1 over the identity map, cached in ``x.kernel_maps`` under the
    key such a convolution has."""

    _maps = snn.Conv3d._maps
    _build = staticmethod(snn.Conv3d._build)

    def __init__(self, conv, bn, relu):
        super().__init__()
        self.in_channels, self.out_channels = conv.in_channels, conv.out_channels
        self.kernel_size, self.stride, self.dilation, self.t = conv.kernel_size, conv.stride, conv.dilation, conv.t
        self.kernel_volume = conv.kernel_volume
        self.slope = 0.0 if relu else 1.0
        W, b = folded_weights(conv, bn)
        self.register_buffer("weight", W.reshape(self.kernel_volume, self.in_channels, self.out_channels).contiguous())
        self.register_buffer("bias", b)
        self._packed = {}

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}"
                + (", transpose=True" if self.t else "") + f", slope={self.slope}")

    def _apply(self, fn, *args, **kwargs):
        self._packed = {}                       # the buffers move or change type: pack again
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._packed = {}
        return super()._load_from_state_dict(*args, **kwargs)

    def _operand(self, dtype, widths=None):
        key = (self.weight.device, dtype, widths)
        if key not in self._packed:
            self._packed[key] = ops.sparse_conv_pack(self.weight, dtype, parts=widths)
        return self._packed[key]

    def forward(self, x, residual=None):
        if self.kernel_volume == 1 and self.stride == 1:
            key = (x.s, 1, 1, 1)
            if key not in x.kernel_maps:
                ident = torch.arange(x.C.shape[0], dtype=torch.int32, device=x.C.device).unsqueeze(0)
                x.kernel_maps[key] = (ident, ident)
            nbr, out_coords, out_stride = x.kernel_maps[key][0], x.C, x.s
        else:
            nbr, _, out_coords, out_stride = self._maps(x)
        parts = snn.feature_parts(x)     # a lazy concatenation (snn.cat(..., lazy=True)): the kernel reads the parts
        if parts is None:
            f = ops.sparse_conv_fused(x.F, self._operand(ops.sparse_conv_feature_dtype(x.F)), self.bias, nbr,
                                      residual=residual, slope=self.slope)
        else:
            dtype = ops.sparse_conv_parts_dtype(parts)
            widths = tuple(p.shape[1] for p in parts)
            f = ops.sparse_conv_fused(list(parts), self._operand(dtype, widths), self.bias, nbr, residual=residual,
                                      slope=self.slope)
        return snn.SparseVoxelTensor(f, out_coords, out_stride, x.coord_maps, x.kernel_maps)


class FoldedResidual(_Frozen):
    """Folded twin of ``ResBlock`` / ``BottleneckBlock``: the last convolution of ``block`` takes the shortcut
    (``x.F``, or the output of the folded ``downsample``) as its residual operand, after its ReLU."""

    def __init__(self, block):
        super().__init__()
        self.kind = type(block).__name__
        self.block = _fold_seq(block.block)
        self.downsample = None if block.downsample is None else _fold_seq(block.downsample)
        layers = list(self.block) + list(self.downsample or [])
        if not all(isinstance(m, FoldedConv) for m in layers):
            raise ValueError(f"{self.kind}: only conv - BatchNorm [- ReLU] runs fold into a residual block")

    def extra_repr(self):
        return f"twin of {self.kind}"

    def forward(self, x):
        short = x.F if self.downsample is None else self.downsample(x).F
        layers = list(self.block)
        for conv in layers[:-1]:
            x = conv(x)
        return layers[-1](x, residual=short)


def _fold_seq(seq):
    """A ``Seq`` with every Conv3d -> BatchNorm [-> ReLU] run as one ``FoldedConv``, the rest folded in place."""
    mods, out, i = list(seq), snn.Seq(), 0
    while i < len(mods):
        if isinstance(mods[i], snn.Conv3d) and i + 1 < len(mods) and isinstance(mods[i + 1], snn.BatchNorm):
            relu = i + 2 < len(mods) and isinstance(mods[i + 2], snn.ReLU)
            out.append(FoldedConv(mods[i], mods[i + 1], relu))
            i += 3 if relu else 2
        else:
            out.append(_fold(mods[i]))
            i += 1
    out.training = False
    return out


def _fold(module):
    if isinstance(module, _Residual):
        return FoldedResidual(module)
    if isinstance(module, snn.Seq):
        return _fold_seq(module)
    for name, child in list(module.named_children()):
        module._modules[name] = _fold(child)
    return module


def fold_for_inference(module):
    """A deep copy of ``module`` (in eval mode) with every Conv3d / Conv3dTranspose -> BatchNorm [-> ReLU] run of a
    ``Seq`` as one ``FoldedConv`` and every ``ResBlock`` / ``BottleneckBlock`` as a ``FoldedResidual``; everything else
    (the pooling branches of a ``MultimodalBlockDown`` included) is copied as it is.  ``module`` is not modified."""
    if any(m.training for m in module.modules()):
        raise ValueError("fold_for_inference folds the running statistics of eval mode: call module.eval() first")
    return _fold(copy.deepcopy(module))
