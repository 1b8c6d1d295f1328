"""Autograd-aware Python entry points of the HIP kernels (through the C ABI, see ``_lib.py``).

Each op mirrors a primitive the reference obtains from ``torch_scatter`` or composes from torch
ops; names and argument meaning follow the reference call sites:

=========================  ==========================================================
``segment_csr``            torch_scatter.segment_csr  (pooling.py:63,289,295,628,787,807)
``gather_csr``             pooling.py:813-841
``segment_gather_csr``     pooling.py:844-856
``segment_softmax_csr``    pooling.py:758-810
``view_attention``         pooling.py:284-300 / :514-530 (softmax + weighted sum + gating)
``gather_nearest``         core/multimodal/image.py:1285 (``x[feature_map_indexing]``)
``gather_bilinear``        core/multimodal/image.py:105-170 (``sparse_interpolation``)
``gather_segment_reduce``  pooling.py:14-71 (``BimodalCSRPool`` mean / sum / min) on image.py:1285, without the gather
``interp_segment_reduce``  pooling.py:14-71 (``BimodalCSRPool`` max / mean / sum / min) on image.py:105-170, without the gather
``grid_cluster``           core/data_transform/grid_transform.py:143-148 (grid_cluster / voxel_grid)
``grid_mean``              grid_transform.py:81 (``scatter_mean``)
``grid_majority``          grid_transform.py:76-79 (one_hot + ``scatter_add`` + argmax)
``radius_query``           core/data_transform/transforms.py:147,215,332,386 (KDTree.query_radius)
``elastic_smooth``         grid_transform.py:231-234 (six ``scipy.ndimage.convolve`` calls)
``elastic_displace``       grid_transform.py:241-242 (``RegularGridInterpolator``)
``elastic_distortion``     grid_transform.py:218-243 (one level of ElasticDistortion)
``image_tail``             core/data_transform/multimodal/image.py:1195-1282 (ColorJitter, flip, ToFloatImage, Normalize)
``image_window``           the same tail over deferred windows: core/multimodal/image.py:578-722 (rolls, crops) folded in
``image_resample``         PIL ``Image.resize`` (8-bit BICUBIC) of decoded RGB batches, as core/multimodal/image.py:1061,1093 call it
``read_images_u8``         core/multimodal/image.py:1059-1099 (resize, roll, crop or box resize) after the decode
``image_nonstatic_mask``   core/data_transform/multimodal/image.py:139-154 (NonStaticMask's comparison)
``cloud_augment``          core/data_transform/transforms.py:463-563, features.py:30-81 (noise, rotation, scale, symmetry, centre)
``log_softmax_nll``        models/segmentation/sparseconv3d.py:45-51 (``F.log_softmax`` + ``F.nll_loss``)
``lovasz_softmax_flat``    metrics/lovasz_loss.py:174-215 (``flatten_probas`` + ``lovasz_softmax_flat``)
``confusion_counts``       metrics/segmentation_tracker.py:72-83 (mask + ``np.argmax`` + ``np.bincount``)
``merge_mapping``          core/multimodal/image.py:2211-2273 (``select_points(mode='merge')`` + ``from_dense``)
``select_mapping``         core/multimodal/image.py:2029-2210, :2279-2342 (``select_images / _views / _points('pick')``, ``crop``)
``voxel_level``            a strided torchsparse ``Conv3d``'s coordinates and maps + modules/multimodal/modules.py:176-198, one sort
=========================  ==========================================================

All ops require tensors on a HIP device and raise otherwise (no CPU fallback).
"""
import collections
import ctypes
import os

import threading

import numpy as np
import torch

from . import _lib
from ._lib import check, dtype_code, ptr, require_device, stream_of

# 0 = auto, 1 = generic kernels, 2 = fused wavefront-team kernels (tests flip this)
ROWS_GRAD_ALGO = 0    # 0: segmented reduction over the row plan; 1: fp32 atomics
ATTENTION_ALGO = 0


class KernelTimer:
    """Optional per-kernel timing with HIP events on the launch stream (bench.py sets
    ``ops.TIMER = KernelTimer()``): records an event pair around every C-ABI launch together with the
    algorithmic bytes of that launch; ``summary()`` synchronises once and aggregates."""

    def __init__(self, only=None):
        # ``only``: names to time; every other launch goes out without events.  An event pair costs the stream ~6 us of
        # bubble per launch on this part (rocprofv3 trace, round 5: 43 pairs = 0.27 ms of an 11.2 ms step), so a region
        # whose WALL time matters times only the kernel(s) it reports on
        self.records = []
        self.only = None if only is None else set(only)

    def launch(self, name, nbytes):
        if self.only is not None and name not in self.only:
            return _NO_TIMER
        return _TimedLaunch(self, name, nbytes)

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, nbytes, e0, e1 in self.records:
            a = agg.setdefault(name, dict(launches=0, ms=0.0, bytes=0))
            a["launches"] += 1
            a["ms"] += e0.elapsed_time(e1)
            a["bytes"] += nbytes
        return agg


class _TimedLaunch:
    def __init__(self, timer, name, nbytes):
        self.timer, self.name, self.nbytes = timer, name, nbytes

    def __enter__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e1 = torch.cuda.Event(enable_timing=True)
        self.e0.record()

    def __exit__(self, *exc):
        self.e1.record()
        self.timer.records.append((self.name, self.nbytes, self.e0, self.e1))
        return False


class _NoTimer:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_TIMER = _NoTimer()
TIMER = None

# ---------------------------------------------------------------------------------------------
# small zero-filled tensors (statistics accumulators, gradient arenas) without a fill launch each
# ---------------------------------------------------------------------------------------------
_ZERO_POOLS = {}
_ZERO_LOCK = threading.Lock()
_ZERO_POOL_BYTES = 32 << 20
_ZERO_SMALL_BYTES = 1 << 20


def zeros_small(shape, dtype, device):
    """``torch.zeros(shape, dtype=dtype, device=device)`` for the small accumulators of a step (fp64 statistics of a
    BatchNorm layer, the fp32 arena of a backward): a piece of a 32 MiB zero-filled pool per (device, stream) that only
    moves forward -- a piece is handed out once, so it is zero when the kernel that accumulates into it runs, and the
    pool is replaced (one fill) when it is used up.  A step of the pooling path asks for ~10 such tensors; each used to
    be its own 4-5 us fill kernel (round 5).  Large requests and requests during a HIP-graph capture (a captured fill is
    replayed, the pool's fill is not) take the plain ``torch.zeros``."""
    device = torch.device(device)
    n = 1
    for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)):
        n *= int(d)
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    if (device.type != "cuda" or nbytes == 0 or nbytes > _ZERO_SMALL_BYTES
            or torch.cuda.is_current_stream_capturing()):
        return torch.zeros(shape, dtype=dtype, device=device)
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    step = (nbytes + 255) & ~255
    with _ZERO_LOCK:        # the autograd thread and the caller's thread may both ask (never the same piece twice)
        return _zero_piece(key, step, nbytes, shape, dtype, device)


def _zero_piece(key, step, nbytes, shape, dtype, device):
    pool = _ZERO_POOLS.get(key)
    if pool is None or pool[1] + step > _ZERO_POOL_BYTES:
        # the pieces of a used-up pool are still alive when its successor is allocated: the first pool reserves the
        # second block as well (held while the first is allocated, then handed back to the caching allocator), so that
        # no hipMalloc lands in a later step (a pool lasts ~200 steps of the headline workload)
        spare = torch.empty(_ZERO_POOL_BYTES, dtype=torch.uint8, device=device) if pool is None else None
        pool = [torch.zeros(_ZERO_POOL_BYTES, dtype=torch.uint8, device=device), 0]
        del spare
        _ZERO_POOLS[key] = pool
    off = pool[1]
    pool[1] = off + step
    # NOT a view of the pool tensor: views share the base's autograd version counter, so an in-place update of one piece
    # (AccumulateGrad's `grad += new` on a parameter gradient that lives in a piece) would invalidate every other piece
    # saved for backward ("modified by an inplace operation").  A fresh tensor set_ onto the pool's storage
    # has its own counter; `off` is a multiple of 256 bytes, so it is a whole number of elements of any dtype.
    piece = torch.empty(0, dtype=dtype, device=device)
    size = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (int(shape),)
    return piece.set_(pool[0].untyped_storage(), off // piece.element_size(), size)


def _timed(name, nbytes):
    return TIMER.launch(name, int(nbytes)) if TIMER is not None else _NO_TIMER


def _as_2d(src):
    if src.dim() == 1:
        return src.reshape(-1, 1), True
    if src.dim() != 2:
        raise NotImplementedError("CSR ops take 1D or 2D source tensors")  # pooling.py:774-777
    return src, False


def _check_ptr(csr_idx):
    if csr_idx.dim() != 1:
        raise ValueError("CSR ops can only be computed over 1D CSR indices")  # pooling.py:771-773
    if csr_idx.dtype != torch.int64:
        raise TypeError(f"CSR pointers must be int64 (LongTensor), got {csr_idx.dtype}")
    return csr_idx.contiguous()


class _SegmentCSR(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, csr_idx, reduce):
        lib = _lib.load()
        require_device(src, csr_idx)
        src = src.contiguous()
        n, C = csr_idx.shape[0] - 1, src.shape[1]
        out = torch.empty((n, C), dtype=src.dtype, device=src.device)
        arg = None
        code = _lib.REDUCE_CODE[reduce]
        if code in (_lib.DVA_MAX, _lib.DVA_MIN):
            arg = torch.empty((n, C), dtype=torch.int32, device=src.device)
        with _timed("segment_csr_fwd", (src.shape[0] + n) * C * src.element_size() + n * 8
                    + (n * C * 4 if arg is not None else 0)):
            check(lib.dva_segment_csr_fwd(ptr(src), ptr(csr_idx), ptr(out), ptr(arg), n, C,
                                          dtype_code(src), code, stream_of(src)), "dva_segment_csr_fwd")
        ctx.save_for_backward(csr_idx, arg if arg is not None else csr_idx)
        ctx.meta = (code, src.shape[0], C, arg is not None)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        csr_idx, arg = ctx.saved_tensors
        code, M, C, has_arg = ctx.meta
        gout = gout.contiguous()
        n = csr_idx.shape[0] - 1
        # rows not covered by the pointers (none for a well-formed CSR) keep zero gradient
        gsrc = torch.zeros((M, C), dtype=gout.dtype, device=gout.device)
        with _timed("segment_csr_bwd", (M + n) * C * gout.element_size() + n * 8
                    + (n * C * 4 if has_arg else 0)):
            check(lib.dva_segment_csr_bwd(ptr(gout), ptr(csr_idx), ptr(arg) if has_arg else None,
                                          ptr(gsrc), n, C, dtype_code(gout), code, stream_of(gout)),
                  "dva_segment_csr_bwd")
        return gsrc, None, None


def segment_csr(src, csr_idx, out=None, reduce="sum"):
    """``torch_scatter.segment_csr`` for 1D/2D ``src`` reduced along dim 0. Empty groups give 0."""
    assert out is None, "out= is not supported"
    if reduce not in _lib.REDUCE_CODE:
        raise ValueError(f"Unknown reduce '{reduce}'")
    csr_idx = _check_ptr(csr_idx)
    src2, was_1d = _as_2d(src)
    res = _SegmentCSR.apply(src2, csr_idx, reduce)
    return res.reshape(-1) if was_1d else res


def segment_csr_arg(src, csr_idx, reduce="max"):
    """(values, arg) of a max/min CSR reduction; arg = winning row (int32, -1 for empty groups,
    first row on ties). Not differentiable (used for index selection, pooling.py:135-143)."""
    if reduce not in ("max", "min"):
        raise ValueError("segment_csr_arg supports 'max' and 'min'")
    lib = _lib.load()
    csr_idx = _check_ptr(csr_idx)
    src2, was_1d = _as_2d(src.detach())
    require_device(src2, csr_idx)
    src2 = src2.contiguous()
    n, C = csr_idx.shape[0] - 1, src2.shape[1]
    out = torch.empty((n, C), dtype=src2.dtype, device=src2.device)
    arg = torch.empty((n, C), dtype=torch.int32, device=src2.device)
    check(lib.dva_segment_csr_fwd(ptr(src2), ptr(csr_idx), ptr(out), ptr(arg), n, C,
                                  dtype_code(src2), _lib.REDUCE_CODE[reduce], stream_of(src2)),
          "dva_segment_csr_fwd")
    if was_1d:
        return out.reshape(-1), arg.reshape(-1)
    return out, arg


class _GatherCSR(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, csr_idx, n_rows):
        lib = _lib.load()
        require_device(src, csr_idx)
        src = src.contiguous()
        n, C = csr_idx.shape[0] - 1, src.shape[1]
        out = torch.empty((n_rows, C), dtype=src.dtype, device=src.device)
        with _timed("gather_csr", (n_rows + n) * C * src.element_size() + n * 8):
            check(lib.dva_gather_csr(ptr(src), ptr(csr_idx), ptr(out), n, C, dtype_code(src),
                                     stream_of(src)), "dva_gather_csr")
        ctx.save_for_backward(csr_idx)
        return out

    @staticmethod
    def backward(ctx, gout):
        (csr_idx,) = ctx.saved_tensors
        return _SegmentCSR.apply(gout.contiguous(), csr_idx, "sum"), None, None


def num_items(csr_idx):
    """Number of rows a CSR pointer tensor covers (one host sync, like csr.py:140)."""
    return int(csr_idx[-1].item()) if csr_idx.numel() > 0 else 0


def gather_csr(src, csr_idx, n_rows=None):
    """pooling.py:813-841: redistribute group-level rows to the group's elements."""
    if not torch.is_floating_point(src):
        raise ValueError("`gather_csr` can only be computed over tensors with floating point data types.")
    csr_idx = _check_ptr(csr_idx)
    src2, was_1d = _as_2d(src)
    if n_rows is None:
        n_rows = num_items(csr_idx)
    res = _GatherCSR.apply(src2, csr_idx, n_rows)
    return res.reshape(-1) if was_1d else res


def segment_gather_csr(src, csr_idx, reduce="sum"):
    """pooling.py:844-856."""
    n_rows = src.shape[0]
    return gather_csr(segment_csr(src, csr_idx, reduce=reduce), csr_idx, n_rows=n_rows)


class _SegmentSoftmaxCSR(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, csr_idx, eps, scaling):
        lib = _lib.load()
        require_device(src, csr_idx)
        src = src.contiguous()
        n, G = csr_idx.shape[0] - 1, src.shape[1]
        out = torch.zeros_like(src)
        check(lib.dva_segment_softmax_csr_fwd(ptr(src), ptr(csr_idx), ptr(out), n, G, int(scaling),
                                              float(eps), stream_of(src)),
              "dva_segment_softmax_csr_fwd")
        ctx.save_for_backward(out, csr_idx)
        ctx.scaling = int(scaling)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        out, csr_idx = ctx.saved_tensors
        gout = gout.contiguous()
        n, G = csr_idx.shape[0] - 1, out.shape[1]
        gsrc = torch.zeros_like(out)
        check(lib.dva_segment_softmax_csr_bwd(ptr(gout), ptr(out), ptr(csr_idx), ptr(gsrc), n, G,
                                              ctx.scaling, stream_of(gout)),
              "dva_segment_softmax_csr_bwd")
        return gsrc, None, None, None


def segment_softmax_csr(src, csr_idx, eps=1e-12, scaling=False):
    """pooling.py:758-810 (same error behaviour)."""
    if not torch.is_floating_point(src):
        raise ValueError(
            "`segment_csr_softmax` can only be computed over tensors with floating point data types.")
    if csr_idx.dim() != 1:
        raise ValueError("`segment_csr_softmax` can only be computed over 1D CSR indices.")
    if src.dim() > 2:
        raise NotImplementedError(
            "`segment_csr_softmax` can only be computed over 1D or 2D source tensors.")
    csr_idx = _check_ptr(csr_idx)
    src2, was_1d = _as_2d(src)
    res = _SegmentSoftmaxCSR.apply(src2.float(), csr_idx, eps, scaling).to(src.dtype)
    return res.reshape(-1) if was_1d else res


class _ViewAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, compat, csr_idx, gate_w, gate_b, scaling, eps):
        lib = _lib.load()
        require_device(val, compat, csr_idx, gate_w, gate_b)
        val = val.contiguous()
        compat = compat.contiguous()
        N, (V, C), G = csr_idx.shape[0] - 1, val.shape, compat.shape[1]
        gw = gate_w.detach().reshape(-1).float().contiguous() if gate_w is not None else None
        gb = gate_b.detach().reshape(-1).float().contiguous() if gate_b is not None else None
        if (gw is None) != (gb is None):
            # Gating(weight=.., bias=..) with one of them disabled: neutral element for the other
            gw = gw if gw is not None else torch.ones(G, device=val.device)
            gb = gb if gb is not None else torch.zeros(G, device=val.device)
        out = torch.empty((N, C), dtype=val.dtype, device=val.device)
        att = torch.zeros((V, G), dtype=torch.float32, device=val.device)
        gate = torch.empty((N, G), dtype=torch.float32, device=val.device)
        amax = torch.empty((N, G), dtype=torch.int32, device=val.device)
        es = val.element_size()
        with _timed("view_attention_fwd", V * (C * es + 2 * G * 4) + N * (C * es + 8 + 2 * G * 4)):
            check(lib.dva_view_attention_fwd(ptr(val), ptr(compat), ptr(csr_idx), ptr(gw), ptr(gb),
                                             ptr(out), ptr(att), ptr(gate), ptr(amax), N, V, C, G,
                                             int(scaling), float(eps), dtype_code(val), ATTENTION_ALGO,
                                             stream_of(val)), "dva_view_attention_fwd")
        ctx.save_for_backward(val, compat, csr_idx, att, gate, amax,
                              gw if gw is not None else csr_idx, gb if gb is not None else csr_idx)
        ctx.meta = (int(scaling), gw is not None,
                    None if gate_w is None else gate_w.shape, None if gate_b is None else gate_b.shape)
        ctx.mark_non_differentiable(att, gate)
        return out, att, gate

    @staticmethod
    def backward(ctx, gout, _gatt, _ggate):
        lib = _lib.load()
        val, compat, csr_idx, att, gate, amax, gw, gb = ctx.saved_tensors
        scaling, has_gate, w_shape, b_shape = ctx.meta
        gout = gout.contiguous()
        N, (V, C), G = csr_idx.shape[0] - 1, val.shape, compat.shape[1]
        gval = torch.zeros_like(val)
        gcompat = torch.zeros_like(compat)
        gwb = torch.zeros(2 * G, dtype=torch.float32, device=val.device) if has_gate else None
        es = val.element_size()
        with _timed("view_attention_bwd", V * (2 * C * es + 2 * G * 4) + N * (C * es + 8 + 3 * G * 4)):
            check(lib.dva_view_attention_bwd(ptr(gout), ptr(val), ptr(compat), ptr(att), ptr(gate),
                                             ptr(amax), ptr(csr_idx), ptr(gw) if has_gate else None,
                                             ptr(gb) if has_gate else None, ptr(gval), ptr(gcompat),
                                             ptr(gwb), N, V, C, G, scaling, dtype_code(val),
                                             ATTENTION_ALGO, stream_of(val)), "dva_view_attention_bwd")
        g_w, g_b = _gate_grads(gwb, G, has_gate, w_shape, b_shape)
        return gval, gcompat, None, g_w, g_b, None, None


def view_attention(val, compat, csr_idx, gate_w=None, gate_b=None, scaling=False, eps=1e-12):
    """Fused tail of GroupBimodalCSRPool / QKVBimodalCSRPool (pooling.py:284-300).

    :param val: [V, C] values (fp32 or bf16)
    :param compat: [V, G] compatibilities (computed in fp32)
    :param csr_idx: LongTensor [N+1]
    :param gate_w, gate_b: Gating parameters of shape [1, G] (both None -> no gating)
    :return: (x_pool [N, C], attentions [V, G], gating [N, G])
    """
    csr_idx = _check_ptr(csr_idx)
    if compat.dim() == 1:
        compat = compat.reshape(-1, 1)
    return _ViewAttention.apply(val, compat.float(), csr_idx, gate_w, gate_b, scaling, eps)


# ---------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------

def pack_gather_index(images, atom_ptr, pixels, ratio=1.0):
    """8-byte packed (image, x, y) index of every atom, at feature-map resolution.

    images LongTensor [V], atom_ptr LongTensor [V+1], pixels int16/int32/int64 [P, 2] (w, h);
    ``ratio`` is the mapping -> feature-map downscale (image.py:1916-1980).
    """
    lib = _lib.load()
    require_device(images, atom_ptr, pixels)
    images = images.contiguous()
    atom_ptr = _check_ptr(atom_ptr)
    pixels = pixels.contiguous()
    if pixels.dtype not in (torch.int16, torch.int32, torch.int64):
        raise TypeError(f"pixels must be int16/int32/int64, got {pixels.dtype}")
    V, P = images.shape[0], pixels.shape[0]
    packed = torch.empty(P, dtype=torch.int64, device=pixels.device)
    check(lib.dva_pack_gather_index(ptr(images), ptr(atom_ptr), ptr(pixels), pixels.element_size(),
                                    float(ratio), V, P, ptr(packed), stream_of(pixels)),
          "dva_pack_gather_index")
    return packed


def _nhwc(x):
    """[B,C,H,W] tensor -> contiguous [B,H,W,C] storage (free if x is channels_last)."""
    return x.permute(0, 2, 3, 1).contiguous()


class _GatherNearest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, packed):
        lib = _lib.load()
        require_device(x, packed)
        B, C, H, W = x.shape
        xl = _nhwc(x)
        P = packed.shape[0]
        out = torch.empty((P, C), dtype=x.dtype, device=x.device)
        es = x.element_size()
        # P*(g*C*s + idx) + P*C*s with g = 1
        with _timed("gather_nearest_fwd", P * (2 * C * es + 8)):
            check(lib.dva_gather_nearest_fwd(ptr(xl), ptr(packed), ptr(out), P, B, H, W, C,
                                             dtype_code(x), stream_of(x)), "dva_gather_nearest_fwd")
        ctx.save_for_backward(packed)
        ctx.meta = (B, C, H, W, x.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        (packed,) = ctx.saved_tensors
        B, C, H, W, dt = ctx.meta
        gout = gout.contiguous()
        P = packed.shape[0]
        if ROWS_GRAD_ALGO == 0:
            # deterministic segmented reduction over the row plan (sorted atoms) instead of fp32 atomics
            row_idx, _, (perm, row_ptr) = gather_row_index(packed, B, H, W, with_counts=False, with_plan=True, split=False)
            gx = torch.empty((B, H, W, C), dtype=torch.float32, device=gout.device)
            with _timed("gather_nearest_bwd", P * (C * gout.element_size() + 12) + B * H * W * C * 4):
                check(lib.dva_gather_rows_sum(ptr(gout), ptr(perm), ptr(row_ptr), None, 0, ptr(gx), B * H * W, P, C,
                                              dtype_code(gout), stream_of(gout)), "dva_gather_rows_sum")
            return gx.permute(0, 3, 1, 2).to(dt), None
        gx = torch.zeros((B, H, W, C), dtype=torch.float32, device=gout.device)
        # P*(C*s + idx) + P*g*C*4*2 (read-modify-write of the fp32 gradient map)
        with _timed("gather_nearest_bwd", P * (C * gout.element_size() + 8) + P * C * 4 * 2):
            check(lib.dva_gather_nearest_bwd(ptr(gout), ptr(packed), ptr(gx), P, B, H, W,
                                             C, dtype_code(gout), stream_of(gout)),
                  "dva_gather_nearest_bwd")
        return gx.permute(0, 3, 1, 2).to(dt), None


def gather_nearest(x, packed_idx):
    """``x[(batch, ..., h, w)]`` on a [B,C,H,W] map (image.py:1285) -> [P, C]."""
    assert x.dim() == 4
    return _GatherNearest.apply(x, packed_idx)


def _anchor_ok(C, dtype):
    """The anchor route of the bilinear backward (dva_anchor_rows_sum / _fixup: fp32 and bf16 gradients only; an fp16
    gradient takes dva_gather_rows_sum)."""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    vec = 4 if dtype == torch.float32 else 8
    lpr = C // vec
    return C % vec == 0 and lpr > 0 and (lpr & (lpr - 1)) == 0 and lpr <= 64


ANCHOR_WS_BYTES = None     # test hook: workspace budget of bilinear_scatter in bytes (None: from the free device memory)


def _anchor_chunk_images(B, bytes_per_image, device):
    """Images per pass of ``bilinear_scatter`` so that the per-anchor sums stay within the workspace budget."""
    budget = ANCHOR_WS_BYTES
    if budget is None:
        if B * bytes_per_image <= (1 << 30):
            return B                                   # small: no driver query on the common path
        free, _ = torch.cuda.mem_get_info(device)
        budget = max(min(free // 4, 8 << 30), 256 << 20)
    return max(1, min(B, budget // max(bytes_per_image, 1)))


def _geometry(B, H=None, W=None):
    """[(B, H, W), ...] of the feature maps behind a bilinear gather: one triple, or one per SETTING of a multi-setting
    batch (``InterpolatedFeatures.cat``: map rows and anchors of the settings are numbered one after the other)."""
    return [(int(B), int(H), int(W))] if H is not None else [tuple(int(v) for v in g) for g in B]


def n_anchors(geometry):
    """Anchors of a geometry, WITHOUT the dummy anchor (which is the next id)."""
    return sum(b * (h + 1) * (w + 1) for b, h, w in geometry)


def anchor_plan(anchors, B, H=None, W=None):
    """The row plan over the ANCHORS of the views (``dva_gather_bilinear_taps_anchor``): ``(perm, row_ptr)`` with
    sum B (H + 1) (W + 1) + 1 anchors (the last one = views without the 2 x 2 tap structure).  ``B`` may be a list of
    (B, H, W) triples (several settings)."""
    return row_plan(anchors, n_anchors(_geometry(B, H, W)) + 1, with_counts=False, split=False)[0]


def bilinear_scatter(grad, tap_rows, tap_weights, anchors, B, H=None, W=None, bn_backward=None, plan=None):
    """Transpose of the bilinear gather: fp32 [B*H*W, C] = sum over the views and their 4 taps of weight x grad row.
    Views are grouped by ANCHOR (the padded cell of their top-left tap, ``dva_gather_bilinear_taps_anchor``): one
    sort of P keys, every gradient row read once into four per-anchor sums, then a 2 x 2 stencil on the map
    (csrc/attention.hip anchor_rows_sum_kernel, csrc/gather.hip anchor_combine_kernel).  Deterministic.
    ``bn_backward = (z_a, bn_a, sm_a, Y)`` (fused bilinear path): ``grad`` is dy_a (bf16, position order) and the
    BatchNorm_a backward ``G dy_a - K1 - K2 z_a`` is folded into the scatter instead of a pass of its own: with ``Y``
    (the interpolated map rows, position order) at the level of the anchor through the Gram matrix of its tap weights
    (one random row per view), without it from the stored ``z_a`` rows; the dummy-anchor views always use ``z_a``."""
    lib = _lib.load()
    grad = grad.contiguous()
    P, C = grad.shape
    geometry = _geometry(B, H, W)                   # several settings: rows and anchors numbered setting after setting
    n_rows = sum(b * h * w for b, h, w in geometry)
    dummy = n_anchors(geometry)                     # the anchor of views without the 2 x 2 structure
    perm, row_ptr = plan if plan is not None else anchor_plan(anchors, geometry)
    st = stream_of(grad)
    es = grad.element_size()
    if bn_backward is not None:
        z_a, bn_a, sm_a, Y = bn_backward
        if grad.dtype != torch.bfloat16 or z_a.dtype != torch.bfloat16 or z_a.shape != grad.shape or C % 32:
            raise _lib.DvaError("bilinear_scatter(bn_backward): bf16 [V, C] rows, C a multiple of 32", -1)
        z_a = z_a.contiguous()
        if Y is not None:
            if Y.dtype != torch.bfloat16 or Y.shape[1] != C:
                raise _lib.DvaError("bilinear_scatter(bn_backward): Y bf16 [R, C]", -1)
            Y = Y.contiguous()
    two_rows = bn_backward is not None and bn_backward[3] is None
    # The per-anchor sums S [anchors, 4, C] fp32 are 4 x the map gradient: bounded workspace, the images
    # go through in chunks when it would exceed the budget (anchors are image-major, so a chunk of images is a
    # contiguous range of the plan; the dummy anchor's views are added tap by tap by the fix-up below)
    out = torch.empty((n_rows, C), dtype=torch.float32, device=grad.device)
    chunks = [_anchor_chunk_images(b, (h + 1) * (w + 1) * 4 * C * 4, grad.device) for b, h, w in geometry]
    S = torch.empty((max(min(i, b) * (h + 1) * (w + 1) for i, (b, h, w) in zip(chunks, geometry)) + 1, 4, C),
                    dtype=torch.float32, device=grad.device)
    n_views_anchored = max(dummy, 1)
    a_off = r_off = 0
    for imgs, (Bs, Hs, Ws) in zip(chunks, geometry):
        per_image = (Hs + 1) * (Ws + 1)
        for b0 in range(0, Bs, imgs):
            nb = min(imgs, Bs - b0)
            a0, na = a_off + b0 * per_image, nb * per_image
            rp = row_ptr[a0:a0 + na + 1]
            with _timed("bilinear_anchor_sum",
                        P * (C * es * (2 if two_rows else 1) + 20) * na // n_views_anchored + na * 4 * C * 4):
                if bn_backward is None:
                    check(lib.dva_anchor_rows_sum(ptr(grad), ptr(perm), ptr(rp), ptr(tap_weights), ptr(S), na, P, C,
                                                  dtype_code(grad), st), "dva_anchor_rows_sum")
                else:
                    check(lib.dva_anchor_rows_sum_bn(ptr(grad), None if Y is not None else ptr(z_a), ptr(bn_a),
                                                     ptr(sm_a), ptr(perm), ptr(rp), ptr(tap_weights),
                                                     ptr(tap_rows) if Y is not None else None, ptr(Y), ptr(S), na, P, C,
                                                     st), "dva_anchor_rows_sum_bn")
            with _timed("bilinear_anchor_combine", na * 4 * C * 4 + nb * Hs * Ws * C * 4):
                check(lib.dva_anchor_combine(ptr(S), ptr(out[r_off + b0 * Hs * Ws:]), nb, Hs, Ws, C, st),
                      "dva_anchor_combine")
        a_off += Bs * per_image
        r_off += Bs * Hs * Ws
    # views of the dummy anchor, tap by tap: the entries only take the dummy id from (B, H, W) = B (H + 1) (W + 1)
    if bn_backward is None:
        check(lib.dva_anchor_fixup(ptr(grad), ptr(tap_rows), ptr(tap_weights), ptr(anchors), ptr(out), P, dummy, 0, 0, C,
                                   dtype_code(grad), st), "dva_anchor_fixup")
    else:
        check(lib.dva_anchor_fixup_bn(ptr(grad), ptr(z_a), ptr(bn_a), ptr(sm_a), ptr(tap_rows), ptr(tap_weights),
                                      ptr(anchors), ptr(out), P, dummy, 0, 0, C, st), "dva_anchor_fixup_bn")
    return out


class _GatherBilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, packed, coords):
        lib = _lib.load()
        require_device(x, packed, coords)
        B, C, H, W = x.shape
        xl = _nhwc(x)
        coords = coords.float().contiguous()
        P = packed.shape[0]
        out = torch.empty((P, C), dtype=x.dtype, device=x.device)
        check(lib.dva_gather_bilinear_fwd(ptr(xl), ptr(packed), ptr(coords), ptr(out), P, B, H, W, C,
                                          dtype_code(x), stream_of(x)), "dva_gather_bilinear_fwd")
        ctx.save_for_backward(packed, coords)
        ctx.meta = (B, C, H, W, x.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        packed, coords = ctx.saved_tensors
        B, C, H, W, dt = ctx.meta
        gout = gout.contiguous()
        P = packed.shape[0]
        if ROWS_GRAD_ALGO == 0 and 4 * P < 2 ** 31:
            # the 4 corner taps of every atom, grouped by map row (row plan), then a weighted segmented
            # reduction: deterministic, no fp32 atomics
            rows4 = torch.empty(4 * P, dtype=torch.int32, device=gout.device)
            w4 = torch.empty(4 * P, dtype=torch.float32, device=gout.device)
            anchors = torch.empty(P, dtype=torch.int32, device=gout.device) if _anchor_ok(C, gout.dtype) else None
            check(lib.dva_gather_bilinear_taps_anchor(ptr(packed), ptr(coords), P, B, H, W, ptr(rows4), ptr(w4),
                                                      ptr(anchors), stream_of(gout)), "dva_gather_bilinear_taps_anchor")
            if anchors is not None:
                # grouped by anchor instead: P keys to sort, every gradient row read once (bilinear_scatter)
                gx = bilinear_scatter(gout, rows4, w4, anchors, B, H, W).view(B, H, W, C)
                return gx.permute(0, 3, 1, 2).to(dt), None, None
            (perm, row_ptr), _ = row_plan(rows4, B * H * W, with_counts=False, split=False)
            gx = torch.empty((B, H, W, C), dtype=torch.float32, device=gout.device)
            with _timed("gather_bilinear_bwd", 4 * P * (C * gout.element_size() + 12) + B * H * W * C * 4):
                check(lib.dva_gather_rows_sum(ptr(gout), ptr(perm), ptr(row_ptr), ptr(w4), 2, ptr(gx), B * H * W,
                                              4 * P, C, dtype_code(gout), stream_of(gout)), "dva_gather_rows_sum")
            return gx.permute(0, 3, 1, 2).to(dt), None, None
        gx = torch.zeros((B, H, W, C), dtype=torch.float32, device=gout.device)
        check(lib.dva_gather_bilinear_bwd(ptr(gout), ptr(packed), ptr(coords), ptr(gx),
                                          packed.shape[0], B, H, W, C, dtype_code(gout),
                                          stream_of(gout)), "dva_gather_bilinear_bwd")
        return gx.permute(0, 3, 1, 2).to(dt), None, None


def gather_bilinear(x, packed_idx, coords):
    """``sparse_interpolation(x, coords, batch)`` with border padding (image.py:105-170)."""
    assert x.dim() == 4
    assert coords.dim() == 2 and coords.shape[1] == 2
    return _GatherBilinear.apply(x, packed_idx, coords)


# ---------------------------------------------------------------------------------------------
# lazy view gather + fused gather-attention  (DESIGN.md "E_mod hoisting")
# ---------------------------------------------------------------------------------------------

# The split plan (round 5, csrc/plan_split.hip): from 1 - 2 M views on (and 512 < rows <= 2^18) ``row_plan`` builds only the
# offset tables of a two-pass radix partition -- row_ptr and counts come out of them -- and the backward runs the two
# scatter passes on the 16-byte view records themselves, so the rows gradient streams its records in plan order.
# DVA_SPLIT_PLAN=0: the permutation plan everywhere (the A/B).
SPLIT_PLAN = os.environ.get("DVA_SPLIT_PLAN", "1") == "1"
# measured crossover (tools/split_threshold.py, profiles/r05_split_threshold.json: plan + rows gradient at C = 64): the split
# form wins from 2 M views on for any row count (0.13 against 0.17 - 0.23 ms) and from 1 M views on maps of >= 2^17 rows
# (0.10 against 0.19 ms); at 0.5 M views its eight launches cost what the records' lines do
SPLIT_PLAN_MIN_VIEWS = 1 << 20


def split_plan_serves(dtype, C):
    """Does a consumer of [R, C] value rows of this dtype take its rows gradient over a SplitPlan?  bf16 / fp16: the
    16-byte records of the chain (any C: bucket kernel at C in {32, 64}, the two record passes otherwise); fp32: the 32-byte
    records of the lean attention backward at C in {32, 64} (round 6).  Everything else wants the permutation."""
    # (a plan builder that knew its consumer's shapes would ask attention_bwd_route which backward runs: DESIGN.md)
    return dtype in (torch.bfloat16, torch.float16) or (dtype == torch.float32 and C in (32, 64))


def _split_plan_pays(n_views, n_rows):
    return n_views >= SPLIT_PLAN_MIN_VIEWS and (n_views >= 2 * SPLIT_PLAN_MIN_VIEWS or n_rows >= (1 << 17))

# DVA_SPLIT_FUSED=0: pass B + the segmented reduction of attention.hip instead of the bucket kernel (the A/B; also the
# form whose sums equal the permutation plan's bit for bit)
SPLIT_FUSED = os.environ.get("DVA_SPLIT_FUSED", "1") == "1"


def _legacy_row_plan(row_idx, n_rows, with_counts):
    lib = _lib.load()
    V, dev = row_idx.shape[0], row_idx.device
    perm = torch.empty(V, dtype=torch.int32, device=dev)
    row_ptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(n_rows, dtype=torch.int32, device=dev) if with_counts else None
    ws, nbytes = _lib.workspace("dva_row_plan_workspace_bytes", dev, V, n_rows)
    with _timed("row_plan", V * 16):
        check(lib.dva_row_plan(ptr(row_idx), V, n_rows, ptr(perm), ptr(row_ptr), ptr(counts), ptr(ws),
                               int(nbytes), stream_of(row_idx)), "dva_row_plan")
    return (perm, row_ptr), counts


class SplitPlan:
    """The backward of the row gather (reference ``core/multimodal/image.py:1262-1287``: ``x[idx]`` in the forward, an
    ``index_add`` of the views' gradients in the backward) for large mappings.
    A row plan without its permutation: ``row_ptr`` and the offset tables of the two scatter passes
    (``dva_plan_split_build``).  ``sort_records`` brings the 16-byte view records of a backward into plan order;
    callers that want ``(perm, row_ptr)`` (unpacking, ``plan[0]``) get the permutation from ``dva_row_plan`` on first
    use -- correct, but it pays the sort the split plan exists to avoid."""

    def __init__(self, row_idx, n_rows, row_ptr, tables):
        self.row_idx, self.n_rows, self.row_ptr, self.tables = row_idx, int(n_rows), row_ptr, tables
        self._perm = None

    LAZY_PERMS = 0      # how often a consumer asked a split plan for its permutation (each one = a full dva_row_plan sort)

    @property
    def perm(self):
        if self._perm is None:
            if SplitPlan.LAZY_PERMS == 0:
                import warnings
                warnings.warn("SplitPlan.perm: a consumer wants (perm, row_ptr) from a split plan -- the permutation is "
                              "being built by a full dva_row_plan sort on top of the split build (correct, but slower "
                              "than asking row_plan(..., split=False) up front); counted in ops.SplitPlan.LAZY_PERMS",
                              RuntimeWarning, stacklevel=3)
            SplitPlan.LAZY_PERMS += 1
            self._perm, row_ptr = _legacy_row_plan(self.row_idx, self.n_rows, False)[0]
            if self.row_ptr is None:        # a plan made of the row index alone
                self.row_ptr = row_ptr
        return self._perm

    def __iter__(self):
        yield self.perm
        yield self.row_ptr

    def __getitem__(self, i):
        return (self.perm, self.row_ptr)[i] if i in (0, -2) else (None, self.row_ptr)[i]

    def __len__(self):
        return 2

    def sort_records(self, rec, keyed=False, bucket_order=False):
        """rec int32 [V, 4] in view order -> the same storage in plan order (word 3 of a record = its row key).
        ``keyed``: word 3 already holds the row key (the records of ``dva_chain_attn_bwd``).  ``bucket_order``: pass A
        only -- a NEW tensor with the records in bucket order (what ``rows_grad_fused`` consumes)."""
        lib = _lib.load()
        V = self.row_idx.shape[0]
        assert rec.shape == (V, 4) and rec.dtype == torch.int32 and rec.is_contiguous()
        buf = torch.empty_like(rec)
        with _timed("plan_sort_records", V * ((32 if bucket_order else 64) + (0 if keyed else 4))):
            check(lib.dva_plan_split_sort_records(None if keyed else ptr(self.row_idx), ptr(rec), V, self.n_rows,
                                                  ptr(self.row_ptr),
                                                  ptr(self.tables), self.tables.numel(), ptr(buf),
                                                  None if bucket_order else ptr(rec), stream_of(rec)),
                  "dva_plan_split_sort_records")
        return buf if bucket_order else rec

    def rows_grad_f32(self, gout, rec, C, G, stream):
        """fp32 [R, C] rows gradient from the 32-byte view records of ``dva_chain_attn_bwd_f32`` (``rec`` fp32 [V, 8], view
        order) through pass A on those records + the fp32 bucket kernel (round 6), or None where it does not apply."""
        lib = _lib.load()
        V, R = self.row_idx.shape[0], self.n_rows
        if (gout.dtype != torch.float32 or C not in (32, 64) or G not in (1, 2, 4) or (C // 4) % G
                or gout.data_ptr() % 16 or not gout.is_contiguous()):
            return None
        assert rec.shape == (V, 8) and rec.dtype == torch.float32 and rec.is_contiguous()
        brec = torch.empty_like(rec)
        with _timed("plan_sort_records", V * (64 + 4)):
            check(lib.dva_plan_split_sort_records32(ptr(self.row_idx), ptr(rec), V, R, ptr(self.tables),
                                                    self.tables.numel(), ptr(brec), stream), "dva_plan_split_sort_records32")
        g = torch.empty((R, C), dtype=torch.float32, device=gout.device)
        with _timed("view_gather_rows_grad", V * (32 + C * 4) + R * C * 4):
            check(lib.dva_plan_split_rows_grad(ptr(gout), ptr(brec), V, R, ptr(self.tables), self.tables.numel(), ptr(g),
                                               C, G, _lib.DVA_F32, _lib.DVA_F32, stream), "dva_plan_split_rows_grad")
        return g

    def rows_grad_fused(self, gout, rec, C, G, stream):
        """bf16 / fp16 [R, C] rows gradient (gout's dtype) from KEYED view-order records through pass A + the bucket kernel
        (``dva_plan_split_rows_grad``: no pass B, no plan-order records), or None where that kernel does not apply."""
        lib = _lib.load()
        V, R = self.row_idx.shape[0], self.n_rows
        # everything dva_plan_split_rows_grad refuses (DVA_ERR_UNSUPPORTED: dtype, C, G, 16-byte alignment of the
        # gradient rows; the records and the output are fresh allocations) is decided here, BEFORE pass A is launched
        if (gout.dtype not in (torch.bfloat16, torch.float16) or C not in (32, 64) or G not in (1, 2, 4) or (C // 8) % G
                or gout.data_ptr() % 16 or not gout.is_contiguous()):
            return None
        brec = self.sort_records(rec, keyed=True, bucket_order=True)
        g = torch.empty((R, C), dtype=gout.dtype, device=gout.device)
        code = dtype_code(gout)
        with _timed("view_gather_rows_grad", V * (16 + C * 2) + R * C * 2):
            check(lib.dva_plan_split_rows_grad(ptr(gout), ptr(brec), V, R, ptr(self.tables), self.tables.numel(), ptr(g),
                                               C, G, code, code, stream), "dva_plan_split_rows_grad")
        return g


def row_plan(row_idx, n_rows, with_counts=True, split=True):
    """Views grouped by the feature-map row they read: ``(perm, row_ptr)`` int32 (+ ``counts`` int32
    [n_rows]).  Stable, so the order of the views inside a row (and with it every sum over them) is
    deterministic.  Large plans come back as a ``SplitPlan`` (same ``row_ptr`` / ``counts``, no permutation) unless the
    caller knows its consumer wants the permutation (``split=False``: fp32 maps, several atoms per view)."""
    lib = _lib.load()
    require_device(row_idx)
    V, dev = row_idx.shape[0], row_idx.device
    if split and SPLIT_PLAN and _split_plan_pays(V, n_rows) and row_idx.is_contiguous():
        nbytes = int(lib.dva_plan_split_table_bytes(V, n_rows))
        if nbytes > 0:
            row_ptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
            counts = torch.empty(n_rows, dtype=torch.int32, device=dev) if with_counts else None
            tables = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            lows = torch.empty(V, dtype=torch.int16, device=dev)
            with _timed("row_plan", V * 10):      # keys read twice, 2-byte digits written + read
                check(lib.dva_plan_split_build(ptr(row_idx), V, n_rows, ptr(row_ptr), ptr(counts), ptr(tables), nbytes,
                                               ptr(lows), V * 2, stream_of(row_idx)), "dva_plan_split_build")
            return SplitPlan(row_idx, n_rows, row_ptr, tables), counts
    return _legacy_row_plan(row_idx, n_rows, with_counts)


def rows_grad_rec16(gout, plan, rec, R, C, G, out_dtype, stream):
    """Rows gradient from the 16-byte view records of ``dva_chain_attn_bwd`` (``rec`` int32 [V, 4], view order; consumed):
    over the permutation plan, or -- ``SplitPlan`` -- after the records themselves went through the plan's two passes."""
    lib = _lib.load()
    V = rec.shape[0]
    if isinstance(plan, SplitPlan):
        if SPLIT_FUSED and out_dtype == gout.dtype:
            fused = plan.rows_grad_fused(gout, rec, C, G, stream)
            if fused is not None:
                return fused
        rec = plan.sort_records(rec, keyed=True)
        perm, row_ptr = None, plan.row_ptr
    else:
        perm, row_ptr = plan
    g = torch.empty((R, C), dtype=out_dtype, device=gout.device)
    with _timed("view_gather_rows_grad", V * ((4 if perm is not None else 0) + 16 + C * 2) + R * (C * 2 + 4)):
        check(lib.dva_view_gather_rows_grad_rec16_to(ptr(gout), ptr(perm), ptr(row_ptr), ptr(rec), ptr(g), dtype_code(g),
                                                     R, V, C, G, dtype_code(gout), stream),
              "dva_view_gather_rows_grad_rec16_to")
    return g


def csr_expand(csr_idx, n_views):
    """int32 [V]: the point (segment) of every view -- the dense form of the CSR pointers."""
    lib = _lib.load()
    require_device(csr_idx)
    vp = torch.empty(n_views, dtype=torch.int32, device=csr_idx.device)
    check(lib.dva_csr_expand(ptr(csr_idx), csr_idx.shape[0] - 1, ptr(vp), stream_of(csr_idx)),
          "dva_csr_expand")
    return vp


def gather_row_index(packed_idx, B, H, W, row_offset=0, with_counts=True, with_plan=False, split=True):
    """Flat row index of every atom into the [B*H*W, C] view of a channels-last map, and the number
    of atoms per row (int32 [B*H*W]) if ``with_counts``.  ``with_plan``: also return the row plan
    (``row_plan``); the counts then come from the plan instead of a histogram with atomics."""
    lib = _lib.load()
    require_device(packed_idx)
    P = packed_idx.shape[0]
    row_idx = torch.empty(P, dtype=torch.int32, device=packed_idx.device)
    hist = with_counts and not with_plan
    counts = torch.zeros(B * H * W, dtype=torch.int32, device=packed_idx.device) if hist else None
    with _timed("gather_row_index", P * 12):
        check(lib.dva_gather_row_index(ptr(packed_idx), P, B, H, W, int(row_offset), ptr(row_idx),
                                       ptr(counts), stream_of(packed_idx)), "dva_gather_row_index")
    if with_plan:
        assert row_offset == 0, "a plan is built over the rows of one map"
        plan, counts = row_plan(row_idx, B * H * W, with_counts, split)
        return row_idx, counts, plan
    return row_idx, counts


def _mapping_row_index_split(images, pixels, ratio, B, H, W, with_counts):
    """Row index and split plan of an exact mapping from one call (``dva_mapping_row_index_split``: the keys and the
    plan's first histogram in one kernel), or None where the split plan does not apply."""
    lib = _lib.load()
    V, R, dev = images.shape[0], B * H * W, pixels.device
    es = pixels.element_size()
    if not (SPLIT_PLAN and _split_plan_pays(V, R)) or pixels.shape[0] != V or pixels.data_ptr() % (2 * es):
        return None
    nbytes = int(lib.dva_plan_split_table_bytes(V, R))
    if nbytes <= 0:
        return None
    row_idx = torch.empty(V, dtype=torch.int32, device=dev)
    row_ptr = torch.empty(R + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(R, dtype=torch.int32, device=dev) if with_counts else None
    tables = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lows = torch.empty(V, dtype=torch.int16, device=dev)
    # image id + pixel pair read, key written, read once more (scatter<LOWS>), 2-byte digits written + read
    with _timed("mapping_row_plan", V * (8 + 2 * es + 4 + 4 + 4)):
        check(lib.dva_mapping_row_index_split(ptr(images), ptr(pixels), es, float(ratio), V, B, H, W, ptr(row_idx),
                                              ptr(row_ptr), ptr(counts), ptr(tables), nbytes, ptr(lows), V * 2,
                                              stream_of(pixels)), "dva_mapping_row_index_split")
    return row_idx, counts, SplitPlan(row_idx, R, row_ptr, tables)


def mapping_row_index(images, atom_ptr, pixels, ratio, B, H, W, with_counts=True, with_plan=True, split=True, exact=False):
    """``gather_row_index(pack_gather_index(images, atom_ptr, pixels, ratio), B, H, W)`` in one pass (no packed index):
    (row_idx, counts, plan) with the counts taken from the row plan.  ``exact``: the caller knows that every view owns
    exactly one atom (``atom_ptr`` = 0 .. V); where the plan is a split plan, the index and the plan then come from one
    call that does not read ``atom_ptr``."""
    lib = _lib.load()
    require_device(images, atom_ptr, pixels)
    images = images.contiguous()
    atom_ptr = _check_ptr(atom_ptr)
    pixels = pixels.contiguous()
    if pixels.dtype not in (torch.int16, torch.int32, torch.int64):
        raise TypeError(f"pixels must be int16/int32/int64, got {pixels.dtype}")
    if exact and split and with_plan:
        fused = _mapping_row_index_split(images, pixels, ratio, B, H, W, with_counts)
        if fused is not None:
            return fused
    V, P = images.shape[0], pixels.shape[0]
    row_idx = torch.empty(P, dtype=torch.int32, device=pixels.device)
    with _timed("gather_row_index", V * 28 + P * 8):
        check(lib.dva_mapping_row_index(ptr(images), ptr(atom_ptr), ptr(pixels), pixels.element_size(), float(ratio),
                                        V, P, B, H, W, ptr(row_idx), stream_of(pixels)), "dva_mapping_row_index")
    if not with_plan:
        return row_idx, None, None
    plan, counts = row_plan(row_idx, B * H * W, with_counts, split)
    return row_idx, counts, plan


class GatheredFeatures:
    """Result of a NEAREST view gather that has not been materialised: ``x_mod[p] = rows[row_idx[p]]``.

    ``rows`` is the [R, C] row view of the channels-last feature map(s) (a differentiable function of
    the 2D encoder output), ``row_idx`` int32 [P], ``counts`` int32 [R] = atoms per row.  Row-wise
    modules (Linear / BatchNorm / activation) commute with the gather, so consumers that understand
    this type apply them to ``rows`` (R << P) and hand ``row_idx`` to the fused gather-attention
    kernel; everything else calls ``materialize()`` and gets the reference's [P, C] tensor.
    ``exact`` tells that every view owns exactly one atom (P == V): the atomic pool is the identity.
    """

    def __init__(self, rows, row_idx, counts, exact, plan=None):
        self.rows, self.row_idx, self.counts, self.exact = rows, row_idx, counts, exact
        self.plan = plan    # (perm, row_ptr) of row_idx, or None: built on demand in backward

    def with_rows(self, rows):
        """Same gather applied to another [R, C'] row tensor (e.g. E_mod(rows))."""
        assert rows.shape[0] == self.rows.shape[0]
        plan = self.plan
        if isinstance(plan, SplitPlan) and not split_plan_serves(rows.dtype, rows.shape[1]):
            plan = None      # the consumer of these rows wants a permutation: built in its backward
        return GatheredFeatures(rows, self.row_idx, self.counts, self.exact, plan)

    @property
    def shape(self):
        return torch.Size((self.row_idx.shape[0], self.rows.shape[1]))

    @property
    def device(self):
        return self.rows.device

    @property
    def dtype(self):
        return self.rows.dtype

    def dim(self):
        return 2

    def materialize(self):
        return gather_rows(self.rows, self.row_idx)

    @staticmethod
    def cat(items, order=None):
        """Concatenate lazily gathered features of several settings (rows are stacked, indices
        offset) and optionally permute the atoms (UnimodalBranch view_cat_sorting)."""
        offs, rows, idx, cnt = 0, [], [], []
        for it in items:
            rows.append(it.rows)
            idx.append(it.row_idx + offs)
            cnt.append(it.counts)
            offs += it.rows.shape[0]
        if len(items) == 1 and order is None:
            return items[0]
        row_idx = torch.cat(idx)
        if order is not None:
            row_idx = row_idx[order]
        return GatheredFeatures(torch.cat(rows, dim=0), row_idx.contiguous(), torch.cat(cnt),
                                all(it.exact for it in items))


def lazy_gather_nearest(x, packed_idx, exact):
    """Lazy counterpart of ``gather_nearest``: no [P, C] tensor is produced."""
    assert x.dim() == 4
    B, C, H, W = x.shape
    rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C)   # view when x is channels_last
    # the split plan serves the 16-byte-record rows gradient: bf16 maps, one atom per view
    row_idx, counts, plan = gather_row_index(packed_idx, B, H, W, with_plan=True,
                                             split=bool(exact) and split_plan_serves(x.dtype, C))
    return GatheredFeatures(rows, row_idx, counts, exact, plan)


def lazy_gather_nearest_mapping(x, images, atom_ptr, pixels, ratio, exact):
    """``lazy_gather_nearest(x, pack_gather_index(images, atom_ptr, pixels, ratio), exact)`` without the packed index."""
    assert x.dim() == 4
    B, C, H, W = x.shape
    rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C)   # view when x is channels_last
    row_idx, counts, plan = mapping_row_index(images, atom_ptr, pixels, ratio, B, H, W,
                                              split=bool(exact) and split_plan_serves(x.dtype, C), exact=bool(exact))
    return GatheredFeatures(rows, row_idx, counts, exact, plan)


def _atoms_per_view_ok(atom_ptr):
    """True when no view owns more than 65534 atoms (the uint16 arg offsets of the fused max pool).  One device
    synchronisation per mapping tensor; the verdict is remembered ON the tensor object together with its version
    counter (not under its address: the caching allocator hands the same address to the next mapping), so a
    new or modified pointer tensor is always measured again."""
    memo = getattr(atom_ptr, "_dva_atoms_ok", None)
    if memo is not None and memo[0] == atom_ptr._version:
        return memo[1]
    n = atom_ptr.shape[0] - 1
    ok = n == 0 or int((atom_ptr[1:] - atom_ptr[:-1]).max()) <= 0xfffe
    try:
        atom_ptr._dva_atoms_ok = (atom_ptr._version, ok)
    except AttributeError:       # a tensor subclass without a __dict__: measure every time
        pass
    return ok


def _identity_gather(xv):
    """Pooled [V, C] rows as ``GatheredFeatures`` under the identity gather (one view per row, exact, with the identity
    row plan): what an atomic pool hands to the view pooling, so that it keeps its fused path (E_mod on the [V, C] rows --
    it does not commute with the pool --, then the recompute chain)."""
    V = xv.shape[0]
    ident = torch.arange(V + 1, dtype=torch.int32, device=xv.device)
    return GatheredFeatures(xv, ident[:V], torch.ones(V, dtype=torch.int32, device=xv.device), True, (ident[:V], ident))


class _GatherSegmentReduce(torch.autograd.Function):
    """``segment_csr(rows[row_idx], csr_idx, reduce)`` for max / mean / sum / min without the [P, C] tensor, forward and backward
    (csrc/gather_reduce.hip).  ``plan`` = the row plan of the items (a split plan hands out its permutation on first
    use and keeps it), or None: built in backward."""

    @staticmethod
    def forward(ctx, rows, row_idx, csr_idx, plan, reduce):
        lib = _lib.load()
        require_device(rows, row_idx, csr_idx)
        rows = rows.contiguous()
        (R, C), S, P = rows.shape, csr_idx.shape[0] - 1, row_idx.shape[0]
        code = _lib.REDUCE_CODE[reduce]
        out = torch.empty((S, C), dtype=rows.dtype, device=rows.device)
        arg = torch.empty((S, C), dtype=torch.int16, device=rows.device) if code in (_lib.DVA_MAX, _lib.DVA_MIN) else None
        es = rows.element_size()
        with _timed("gather_segment_reduce_fwd", P * (4 + C * es) + S * (8 + C * es) + (S * C * 2 if arg is not None else 0)):
            check(lib.dva_gather_segment_reduce_fwd(ptr(rows), ptr(row_idx), ptr(csr_idx), ptr(out), ptr(arg), S, P, R, C,
                                                    dtype_code(rows), code, stream_of(rows)),
                  "dva_gather_segment_reduce_fwd")
        ctx.save_for_backward(row_idx, csr_idx, arg if arg is not None else csr_idx)
        ctx.meta = (R, C, rows.dtype, code, arg is not None)
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        row_idx, csr_idx, arg = ctx.saved_tensors
        R, C, dt, code, has_arg = ctx.meta
        S, P = csr_idx.shape[0] - 1, row_idx.shape[0]
        if P == 0 or R == 0 or C == 0:
            return torch.zeros((R, C), dtype=dt, device=gout.device), None, None, None, None
        gout = gout.contiguous().to(dt)
        perm, row_ptr = _plan_or_build(ctx.plan, row_idx, R, False)      # a split plan builds its permutation once
        soi = csr_expand(csr_idx, P)
        grows = torch.empty((R, C), dtype=dt, device=gout.device)
        es = gout.element_size()
        per_item = 8 + C * es + (0 if code == _lib.DVA_SUM else 8) + (2 * C if has_arg else 0)
        with _timed("gather_segment_reduce_bwd", P * per_item + R * (4 + C * es)):
            check(lib.dva_gather_segment_reduce_bwd(ptr(gout), ptr(arg) if has_arg else None, ptr(csr_idx), ptr(perm),
                                                    ptr(row_ptr), ptr(soi), ptr(grows), S, P, R, C, dtype_code(gout), code,
                                                    stream_of(gout)), "dva_gather_segment_reduce_bwd")
        return grows, None, None, None, None


# A/B and tests: False sends the pools of nearest-gathered features down the materialised route
# (``x_mod.materialize()`` + ``segment_csr``): LAZY_NONEXACT the max pool, LAZY_REDUCE the mean / sum / min pools
LAZY_NONEXACT = True
LAZY_REDUCE = True
_LAZY_REDUCES = ("max", "mean", "sum", "min")


def gather_segment_reduce_applicable(x_mod, csr_idx, reduce):
    """Does a module send this pool to ``gather_segment_reduce``?  Nearest-gathered features on the device in fp32 / bf16 /
    fp16 with S, P and R below 2^31; ``max`` and ``min`` keep uint16 arg offsets, so their segments own <= 65534 items.
    Mean / sum / min: any C >= 1 (rows that are not 16-byte aligned or whose C is no multiple of 16 bytes take the kernels'
    element path; non-contiguous rows are copied by the op).  Max: rows of whole 16-byte chunks only, and a contiguous
    slice whose base is not 16-byte aligned takes the materialised route -- the op itself serves those too, the gate is
    the one the max pool was measured with."""
    if not (isinstance(x_mod, GatheredFeatures) and reduce in _LAZY_REDUCES
            and (LAZY_NONEXACT if reduce == "max" else LAZY_REDUCE)):
        return False
    rows = x_mod.rows
    if not (rows.is_cuda and csr_idx.is_cuda and rows.dim() == 2 and rows.shape[1] >= 1
            and rows.dtype in (torch.float32, torch.bfloat16, torch.float16)
            and max(rows.shape[0], x_mod.row_idx.shape[0], csr_idx.shape[0]) < (1 << 31)):
        return False
    if reduce == "max" and not (rows.shape[1] * rows.element_size() % 16 == 0
                                and (not rows.is_contiguous() or rows.data_ptr() % 16 == 0)):
        return False
    return reduce in ("mean", "sum") or _atoms_per_view_ok(csr_idx)


def gather_segment_reduce(x_mod, csr_idx, reduce, level="view"):
    """Max / mean / sum / min pool of lazily gathered features over CSR segments, gather and reduction in one kernel
    (reference: ``BimodalCSRPool(mode)`` on ``x[idx]``, modules/multimodal/pooling.py:14-71).  ``level='view'``: the plain
    [N, C] tensor of a view pooling.  ``level='atom'`` (atomic pool of a non-exact mapping, several pixels per view,
    modules.py:400-407): the pooled [V, C] rows as ``GatheredFeatures`` under the identity gather, so that the view
    pooling behind it keeps its fused path."""
    if reduce not in _LAZY_REDUCES:
        raise ValueError(f"gather_segment_reduce reduces by one of {_LAZY_REDUCES}, got '{reduce}'")
    if level not in ("view", "atom"):
        raise ValueError(f"level must be 'view' or 'atom', got '{level}'")
    csr_idx = _check_ptr(csr_idx)
    xv = _GatherSegmentReduce.apply(x_mod.rows, x_mod.row_idx.contiguous(), csr_idx, x_mod.plan, reduce)
    return xv if level == "view" else _identity_gather(xv)


class InterpolatedFeatures:
    """Result of a BILINEAR view gather (``sparse_interpolation``, reference image.py:105-170) that has not been
    materialised: ``x_mod[p] = sum_k tap_weights[p, k] * rows[tap_rows[p, k]]`` over the 4 corner taps.

    ``rows`` is the [R, C] row view of the channels-last feature maps (a differentiable function of the 2D encoder
    output), ``tap_rows`` int32 [P, 4] / ``tap_weights`` fp32 [P, 4] the taps of ``dva_gather_bilinear_taps`` (border
    replicated: clamped rows).  A consumer that understands this type (GroupBimodalCSRPool through
    ``fused_bilinear``) evaluates E_mod per view inside its kernels -- the first Linear commutes with the
    interpolation and runs on the R map rows; everything else calls ``materialize()`` and gets the reference's
    [P, C] tensor.  ``exact``: every view owns exactly one atom (P == V): the atomic pool is the identity."""

    def __init__(self, x, packed_idx, coords, tap_rows, tap_weights, anchors, exact):
        self.x, self.packed_idx, self.coords, self.exact = x, packed_idx, coords, exact
        self.tap_rows, self.tap_weights, self.anchors = tap_rows, tap_weights, anchors
        B, C, H, W = x.shape
        self.rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C)      # view when x is channels_last
        self.geometry = [(B, H, W)]     # one (B, H, W) per setting: rows / anchors are numbered setting after setting
        self.parts = self.order = None  # cat(): the per-setting gathers and the view order (materialize goes through them)

    @staticmethod
    def cat(items, order=None):
        """The views of several SETTINGS (feature maps of different sizes, ``ImageData`` = list of
        ``SameSettingImageData``) as one lazy gather, optionally permuted into point order (reference
        modules/multimodal/modules.py:514-525 + core/multimodal/image.py:1549-1588 ``view_cat_sorting``: the reference
        concatenates the materialised [V_s, C] tensors and indexes the result).  The map rows of the settings are stacked
        ([sum R_s, C], differentiable), tap rows and anchors offset into the stacked numbering, so a consumer of taps
        (fused_bilinear) sees one gather; ``materialize()`` still evaluates setting by setting."""
        if len(items) == 1 and order is None:
            return items[0]
        assert all(isinstance(it, InterpolatedFeatures) and it.parts is None for it in items)
        out = InterpolatedFeatures.__new__(InterpolatedFeatures)
        out.x = out.packed_idx = out.coords = None
        out.parts, out.order = list(items), order
        out.exact = all(it.exact for it in items)
        out.geometry = [g for it in items for g in it.geometry]
        out.rows = torch.cat([it.rows for it in items], dim=0)
        # one pass (dva_bilinear_taps_cat): concatenate, offset rows / anchors into the stacked numbering, permute
        import ctypes
        lib = _lib.load()
        S = len(items)
        dev = items[0].tap_rows.device
        V = sum(it.tap_rows.shape[0] for it in items)
        if order is not None:
            order = order.to(torch.int64).contiguous()
            assert order.shape[0] == V
        keep = [(it.tap_rows.contiguous(), it.tap_weights.contiguous(), it.anchors.contiguous()) for it in items]
        arr = lambda k: (ctypes.c_void_p * S)(*[t[k].data_ptr() for t in keep])
        i64 = lambda vals: (ctypes.c_int64 * S)(*vals)
        rows4 = torch.empty((V, 4), dtype=torch.int32, device=dev)
        w4 = torch.empty((V, 4), dtype=torch.float32, device=dev)
        anchors = torch.empty(V, dtype=torch.int32, device=dev)
        with _timed("bilinear_taps_cat", V * (8 + 2 * 36)):
            check(lib.dva_bilinear_taps_cat(S, arr(0), arr(1), arr(2), i64([t[0].shape[0] for t in keep]),
                                            i64([it.rows.shape[0] for it in items]),
                                            i64([n_anchors(it.geometry) for it in items]), ptr(order), V, ptr(rows4),
                                            ptr(w4), ptr(anchors), stream_of(rows4)), "dva_bilinear_taps_cat")
        out.tap_rows, out.tap_weights, out.anchors = rows4, w4, anchors
        return out

    @property
    def shape(self):
        return torch.Size((self.tap_rows.shape[0], self.rows.shape[1]))

    @property
    def device(self):
        return self.rows.device

    @property
    def dtype(self):
        return self.rows.dtype

    def dim(self):
        return 2

    def materialize(self, rows=None):
        """The reference's [P, C] tensor; ``rows`` [R, C']: the same interpolation of another per-row tensor (a linear
        function of the map rows, e.g. the hoisted first Linear of E_mod)."""
        if self.parts is not None:      # several settings: setting by setting, then the view order of cat()
            splits = [None] * len(self.parts) if rows is None else torch.split(rows, [p.rows.shape[0] for p in self.parts])
            out = torch.cat([p.materialize(rows=r) for p, r in zip(self.parts, splits)], dim=0)
            return out if self.order is None else out[self.order]
        if rows is None:
            return gather_bilinear(self.x, self.packed_idx, self.coords)
        B, _, H, W = self.x.shape
        return gather_bilinear(rows.view(B, H, W, rows.shape[1]).permute(0, 3, 1, 2), self.packed_idx, self.coords)


def lazy_gather_bilinear(x, packed_idx, coords, exact):
    """Lazy counterpart of ``gather_bilinear``: the taps are computed, no [P, C] tensor is produced."""
    assert x.dim() == 4 and coords.dim() == 2 and coords.shape[1] == 2
    lib = _lib.load()
    require_device(x, packed_idx, coords)
    B, C, H, W = x.shape
    coords = coords.float().contiguous()
    P = packed_idx.shape[0]
    rows4 = torch.empty((P, 4), dtype=torch.int32, device=x.device)
    w4 = torch.empty((P, 4), dtype=torch.float32, device=x.device)
    anchors = torch.empty(P, dtype=torch.int32, device=x.device)
    with _timed("bilinear_taps", P * (16 + 36)):
        check(lib.dva_gather_bilinear_taps_anchor(ptr(packed_idx), ptr(coords), P, B, H, W, ptr(rows4), ptr(w4),
                                                  ptr(anchors), stream_of(x)), "dva_gather_bilinear_taps_anchor")
    return InterpolatedFeatures(x, packed_idx, coords, rows4, w4, anchors, exact)


class _InterpSegmentReduce(torch.autograd.Function):
    """``segment_csr(x_mod.materialize(), csr_idx, reduce)`` of a bilinear lazy gather for max / mean / sum / min without
    the [P, C] tensor, forward and backward (csrc/interp_reduce.hip).  The gradient goes to the stacked map rows; the plan
    (over the P anchors where ``_anchor_ok`` serves the shape and ``anchors`` / ``geometry`` are given, over the 4 P taps
    elsewhere) and the segment of every item are built in backward and not kept."""

    @staticmethod
    def forward(ctx, rows, tap_rows, tap_weights, csr_idx, reduce, anchors=None, geometry=None):
        lib = _lib.load()
        require_device(rows, tap_rows, tap_weights, csr_idx)
        rows = rows.contiguous()
        (R, C), S, P = rows.shape, csr_idx.shape[0] - 1, tap_rows.shape[0]
        code = _lib.REDUCE_CODE[reduce]
        has_arg = code in (_lib.DVA_MAX, _lib.DVA_MIN)
        out = torch.empty((S, C), dtype=rows.dtype, device=rows.device)
        arg = torch.empty((S, C), dtype=torch.int16, device=rows.device) if has_arg else None
        es = rows.element_size()
        with _timed("interp_segment_reduce_fwd", P * (32 + 4 * C * es) + S * (8 + C * es) + (S * C * 2 if has_arg else 0)):
            check(lib.dva_interp_segment_reduce_fwd(ptr(rows), ptr(tap_rows), ptr(tap_weights), ptr(csr_idx), ptr(out),
                                                    ptr(arg), S, P, R, C, dtype_code(rows), code, stream_of(rows)),
                  "dva_interp_segment_reduce_fwd")
        ctx.save_for_backward(tap_rows, tap_weights, csr_idx, arg if has_arg else csr_idx,
                              anchors if anchors is not None else csr_idx)
        ctx.meta = (R, C, rows.dtype, code, has_arg, geometry if anchors is not None else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        tap_rows, tap_weights, csr_idx, arg, anchors = ctx.saved_tensors
        R, C, dt, code, has_arg, geometry = ctx.meta
        S, P = csr_idx.shape[0] - 1, tap_rows.shape[0]
        none = (None,) * 6
        if P == 0 or R == 0 or C == 0:
            return (torch.zeros((R, C), dtype=dt, device=gout.device),) + none
        gout = gout.contiguous().to(dt)
        soi = csr_expand(csr_idx, P)
        if INTERP_REDUCE_ANCHOR and geometry is not None and _anchor_ok(C, dt):
            return (_interp_anchor_backward(gout, arg if has_arg else None, csr_idx, tap_rows, tap_weights, anchors, soi,
                                            geometry, R, C, code).to(dt),) + none
        perm, row_ptr = row_plan(tap_rows.view(-1), R, with_counts=False, split=False)[0]
        grows = torch.empty((R, C), dtype=dt, device=gout.device)
        es = gout.element_size()
        per_tap = 12 + C * es + (0 if code == _lib.DVA_SUM else 8) + (2 * C if has_arg else 0)
        with _timed("interp_segment_reduce_bwd", 4 * P * per_tap + R * (4 + C * es)):
            check(lib.dva_interp_segment_reduce_bwd(ptr(gout), ptr(arg) if has_arg else None, ptr(csr_idx), ptr(perm),
                                                    ptr(row_ptr), ptr(tap_weights), ptr(soi), ptr(grows), S, P, R, C,
                                                    dtype_code(gout), code, stream_of(gout)),
                  "dva_interp_segment_reduce_bwd")
        return (grows,) + none


def _interp_anchor_backward(gout, arg, csr_idx, tap_rows, tap_weights, anchors, soi, geometry, R, C, code):
    """fp32 [R, C] gradient of ``_InterpSegmentReduce`` over the ANCHOR plan of the items, as ``bilinear_scatter`` forms it
    for a materialised gradient, the [P, C] gradient being evaluated on the fly from ``gout`` [S, C]: per-anchor sums
    (``dva_interp_anchor_rows_sum``, images in chunks within the workspace budget), the 2 x 2 stencil
    (``dva_anchor_combine``), then the items of the dummy anchor tap by tap (``dva_interp_anchor_fixup``)."""
    lib = _lib.load()
    P, dev, st, es = tap_rows.shape[0], gout.device, stream_of(gout), gout.element_size()
    dummy = n_anchors(geometry)
    perm, row_ptr = anchor_plan(anchors, geometry)
    out = torch.empty((R, C), dtype=torch.float32, device=dev)
    chunks = [_anchor_chunk_images(b, (h + 1) * (w + 1) * 4 * C * 4, dev) for b, h, w in geometry]
    S = torch.empty((max(min(i, b) * (h + 1) * (w + 1) for i, (b, h, w) in zip(chunks, geometry)) + 1, 4, C),
                    dtype=torch.float32, device=dev)
    per_item = 24 + C * es + (0 if code == _lib.DVA_SUM else 16) + (2 * C if arg is not None else 0)
    a_off = r_off = 0
    for imgs, (Bs, Hs, Ws) in zip(chunks, geometry):
        per_image = (Hs + 1) * (Ws + 1)
        for b0 in range(0, Bs, imgs):
            nb = min(imgs, Bs - b0)
            a0, na = a_off + b0 * per_image, nb * per_image
            with _timed("interp_anchor_sum", P * per_item * na // max(dummy, 1) + na * 4 * C * 4):
                check(lib.dva_interp_anchor_rows_sum(ptr(gout), ptr(arg), ptr(csr_idx), ptr(perm),
                                                     ptr(row_ptr[a0:a0 + na + 1]), ptr(tap_weights), ptr(soi), ptr(S), na,
                                                     P, C, dtype_code(gout), code, st), "dva_interp_anchor_rows_sum")
            with _timed("bilinear_anchor_combine", na * 4 * C * 4 + nb * Hs * Ws * C * 4):
                check(lib.dva_anchor_combine(ptr(S), ptr(out[r_off + b0 * Hs * Ws:]), nb, Hs, Ws, C, st),
                      "dva_anchor_combine")
        a_off += Bs * per_image
        r_off += Bs * Hs * Ws
    check(lib.dva_interp_anchor_fixup(ptr(gout), ptr(arg), ptr(csr_idx), ptr(perm), ptr(row_ptr), ptr(tap_rows),
                                      ptr(tap_weights), ptr(soi), ptr(out), dummy, P, C, dtype_code(gout), code, st),
          "dva_interp_anchor_fixup")
    return out


# A/B and tests: False sends max / mean / sum / min pools of a bilinear lazy gather down the materialised route
# (``x_mod.materialize()`` + ``segment_csr``)
LAZY_INTERP_REDUCE = True
# A/B and tests: False keeps the backward of ``interp_segment_reduce`` on the plan over the 4 P taps where the anchor plan
# (P keys, ``_anchor_ok`` shapes) would serve it
INTERP_REDUCE_ANCHOR = True
_INTERP_REDUCES = ("max", "mean", "sum", "min")


def interp_segment_reduce_applicable(x_mod, csr_idx, reduce):
    """Does ``interp_segment_reduce`` serve this pool?  A bilinear lazy gather (one setting or a ``cat`` of several) on the
    device with fp32 / bf16 / fp16 map rows, any C >= 1; 4 P taps, R map rows and S segments below 2^31 (int32 tap plan);
    ``max`` and ``min`` keep uint16 arg offsets, so their segments own <= 65534 items.  Not gated on C: on shapes whose
    backward runs over the tap plan (``_anchor_ok`` false) the route measured 0.74 to 1.07 x the materialised one at C = 13
    (profiles/view_pool_bilinear_bench.json) and is kept there for its 1.75 to 2.1 x lower peak memory."""
    if not (LAZY_INTERP_REDUCE and isinstance(x_mod, InterpolatedFeatures) and reduce in _INTERP_REDUCES):
        return False
    rows, taps = x_mod.rows, x_mod.tap_rows
    if not (rows.is_cuda and csr_idx.is_cuda and taps.is_cuda and rows.dim() == 2 and rows.shape[1] >= 1
            and rows.dtype in (torch.float32, torch.bfloat16, torch.float16)
            and max(rows.shape[0], 4 * taps.shape[0], csr_idx.shape[0]) < (1 << 31)):
        return False
    return reduce in ("mean", "sum") or _atoms_per_view_ok(csr_idx)


def _taps16(t):
    """The [P, 4] tap tensor as the kernels read it: contiguous 16-byte records."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def interp_segment_reduce(x_mod, csr_idx, reduce, level="view"):
    """Max / mean / sum / min pool of bilinearly gathered features over CSR segments, interpolation and reduction in one
    kernel (reference: ``BimodalCSRPool(mode)`` on ``sparse_interpolation(x, coords, batch)``, modules/multimodal/
    pooling.py:14-71 on core/multimodal/image.py:105-170).  ``level='view'``: the plain [S, C] tensor.  ``level='atom'``
    (atomic pool of a non-exact mapping, modules.py:400-407): the pooled [V, C] rows as ``GatheredFeatures`` under the
    identity gather, as ``gather_segment_reduce`` returns them."""
    if reduce not in _INTERP_REDUCES:
        raise ValueError(f"interp_segment_reduce reduces by one of {_INTERP_REDUCES}, got '{reduce}'")
    if level not in ("view", "atom"):
        raise ValueError(f"level must be 'view' or 'atom', got '{level}'")
    if not isinstance(x_mod, InterpolatedFeatures):
        raise TypeError(f"interp_segment_reduce pools InterpolatedFeatures, got {type(x_mod).__name__}")
    csr_idx = _check_ptr(csr_idx)
    anchors = getattr(x_mod, "anchors", None)
    xv = _InterpSegmentReduce.apply(x_mod.rows, _taps16(x_mod.tap_rows), _taps16(x_mod.tap_weights), csr_idx, reduce,
                                    anchors.contiguous() if anchors is not None else None, _geometry(x_mod.geometry))
    return xv if level == "view" else _identity_gather(xv)


LAZY_TYPES = (GatheredFeatures, InterpolatedFeatures)     # what .materialize() turns into the reference's [P, C] tensor


def lazy_pool_applicable(x_mod, csr_idx, reduce, atomic):
    """Does ``lazy_pool`` serve ``BimodalCSRPool(reduce)`` on the lazy gather ``x_mod``?  ``atomic``: the pool of the atoms
    of every view (``x_map is None``), else the pool of the views of every point.  A nearest gather at the atomic level is
    pooled only where that shrinks it (S < P)."""
    if isinstance(x_mod, GatheredFeatures):
        return ((not atomic or csr_idx.shape[0] - 1 < x_mod.shape[0])
                and gather_segment_reduce_applicable(x_mod, csr_idx, reduce))
    return interp_segment_reduce_applicable(x_mod, csr_idx, reduce)


def lazy_pool(x_mod, csr_idx, reduce, atomic):
    """``segment_csr(x_mod.materialize(), csr_idx, reduce)`` in one kernel, forward and backward without a [P, C] tensor.
    Nearest gather: a plain [N, C] tensor at the view level; at the atomic level the pooled [V, C] rows stay lazy under the
    identity gather, so that the view pooling keeps its fused path.  Bilinear gather: the plain pooled tensor at both
    levels -- what the materialised route hands on."""
    if isinstance(x_mod, GatheredFeatures):
        return gather_segment_reduce(x_mod, csr_idx, reduce, level="atom" if atomic else "view")
    return interp_segment_reduce(x_mod, csr_idx, reduce, level="view")


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, row_idx):
        ctx.save_for_backward(row_idx)
        ctx.n_rows = rows.shape[0]
        return rows.index_select(0, row_idx.long())

    @staticmethod
    def backward(ctx, gout):
        (row_idx,) = ctx.saved_tensors
        g = torch.zeros((ctx.n_rows, gout.shape[1]), dtype=torch.float32, device=gout.device)
        g.index_add_(0, row_idx.long(), gout.float())
        return g.to(gout.dtype), None


def gather_rows(rows, row_idx):
    """Materialise ``rows[row_idx]`` (device library op; only used off the fused path)."""
    require_device(rows, row_idx)
    return _GatherRows.apply(rows, row_idx)


def _team_records_ok(C, G, dtype):
    """Mirror of team_geometry() in csrc/attention.hip: the view records are produced by the wavefront-team
    backward kernel only."""
    vec = 4 if dtype == torch.float32 else 8
    if C % vec:
        return False
    lpr = C // vec
    pow2 = lambda x: x > 0 and (x & (x - 1)) == 0
    return pow2(lpr) and lpr <= 64 and pow2(G) and G <= 32 and C % G == 0 and (C // G) % vec == 0


# fp32 rows with four score groups: the lean tile-based attention backward (False: the team kernel; tests A/B)
LEAN_ATTENTION_BWD = True

AttentionBwdRoute = collections.namedtuple("AttentionBwdRoute", "kernel rows_grad records")


def attention_bwd_route(rows_dtype, gout_dtype, out_dtype, C, G, V, R, N, need_rows, aligned16):
    """Which kernels the backward of ``view_gather_attention`` launches, from plain values (no tensor, no device call;
    ``LEAN_ATTENTION_BWD``, ``ATTENTION_ALGO`` and ``ROWS_GRAD_ALGO`` are read when it is called).  ``aligned16``: the value
    rows and ``gout`` both start on 16 bytes.  ``kernel``: "lean_f32" / "lean_16" = the tile kernels of csrc/chain_bwd.hip,
    "team" = csrc/attention.hip; ``rows_grad``: "none", "plan" (segmented reduction over the row plan) or "atomics";
    ``records`` ("team" only): the attention backward writes view records for the rows-gradient pass."""
    use_plan = need_rows and ROWS_GRAD_ALGO == 0
    if (LEAN_ATTENTION_BWD and use_plan and ATTENTION_ALGO != 1 and rows_dtype == torch.float32
            and gout_dtype == torch.float32 and G == 4 and C in (32, 64, 128, 256) and V > 0
            and _lib.fits_buffer(V * 32, max(R, N) * C * 4)):
        return AttentionBwdRoute("lean_f32", "plan", False)
    if (LEAN_ATTENTION_BWD and use_plan and ATTENTION_ALGO != 1 and rows_dtype in (torch.bfloat16, torch.float16)
            and gout_dtype == rows_dtype and out_dtype == rows_dtype and G in (1, 2, 4)
            and C in (32, 64, 128, 256, 512) and V > 0 and _lib.fits_buffer(V * 16, max(R, N) * C * 2)):
        return AttentionBwdRoute("lean_16", "plan", False)
    # (the team kernel takes 16-byte aligned value and gradient rows only: csrc/attention.hip bwd_impl)
    records = bool(use_plan and ATTENTION_ALGO != 1 and _team_records_ok(C, G, rows_dtype) and aligned16)
    return AttentionBwdRoute("team", "plan" if use_plan else "atomics" if need_rows else "none", records)


def _gate_grads(gwb, G, has_gate, w_shape, b_shape):
    """(d gate_w, d gate_b) in the parameters' shapes from the fp32 [2 G] accumulator of an attention backward."""
    g_w = gwb[:G].reshape(w_shape) if (has_gate and w_shape is not None) else None
    g_b = gwb[G:].reshape(b_shape) if (has_gate and b_shape is not None) else None
    return g_w, g_b


def _plan_or_build(plan, row_idx, n_rows, split):
    """The caller's row plan, or one built now; ``split=False`` where the consumer unpacks ``(perm, row_ptr)``."""
    return plan if plan is not None else row_plan(row_idx, n_rows, with_counts=False, split=split)[0]


def _rows_grad_perm(gout, att, gate, vp, perm, row_ptr, rec, rs, R, C, G, rows):
    """fp32 [R, C] rows gradient of ``view_gather_attention``: segmented reduction over the permutation plan, from the
    view records (``rec`` fp32 [V, rs]) or, without them, from ``vp`` (view -> point) + ``att`` + ``gate``."""
    lib = _lib.load()
    V = att.shape[0]
    grows = torch.empty((R, C), dtype=torch.float32, device=rows.device)
    # per view: perm + record (or view_point + scores) + grad_out row; per row: fp32 row written
    per_view = 4 + (rs * 4 if rec is not None else 4 + 2 * G * 4) + C * rows.element_size()
    with _timed("view_gather_rows_grad", V * per_view + R * (C * 4 + 4)):
        check(lib.dva_view_gather_rows_grad(
            ptr(gout), ptr(att), ptr(gate), ptr(vp), ptr(perm), ptr(row_ptr), ptr(rec), rs, ptr(grows), R, V, C, G,
            dtype_code(rows), stream_of(rows)), "dva_view_gather_rows_grad")
    return grows


# The three attention backwards (attention_bwd_route picks one).  Arguments: the route, the caller's row plan or None, the
# forward's saved tensors (gw / gb None without gating), grad_out, the score gradients to fill, the gate accumulator or None,
# scaling, eps.  Each returns (grows, gcompat).

def _attn_bwd_lean_f32(route, plan, rows, row_idx, compat, csr_idx, att, gate, amax, gw, gb, out, gout, gcompat, gwb,
                       scaling, eps):
    # fp32 rows, four score groups (the no-autocast headline shape): the tile-based attention backward of the
    # chain path (csrc/chain_bwd.hip attn_bwd_kernel<float, ...>: scores in, score gradients + 32-byte view
    # records out) instead of the team kernel: 2.8 -> 2.0 ms at V = 33.5 M
    from .fused_chain import build_tiles
    lib = _lib.load()
    N, V, (R, C), G = csr_idx.shape[0] - 1, row_idx.shape[0], rows.shape, compat.shape[1]
    tiles, n_tiles = build_tiles(csr_idx, V)
    vp = csr_expand(csr_idx, V)
    rec = torch.empty((V, 8), dtype=torch.float32, device=rows.device)
    with _timed("view_gather_attention_bwd", V * (C * 4 + 16 + 8 + 16 + 32) + N * (C * 4 + 8)):
        check(lib.dva_chain_attn_bwd_f32(
            ptr(compat), ptr(vp), ptr(tiles), ptr(n_tiles), ptr(rows), ptr(row_idx), ptr(csr_idx), ptr(gw), ptr(gb),
            ptr(gout), ptr(out), ptr(gcompat), ptr(rec), ptr(gwb), N, V, R, C, G, scaling, eps, stream_of(rows)),
            "dva_chain_attn_bwd_f32")
    plan = _plan_or_build(plan, row_idx, R, split_plan_serves(rows.dtype, C))
    grows = None
    if isinstance(plan, SplitPlan) and SPLIT_FUSED:
        # round 6: the 32-byte records through pass A of the split plan + the fp32 bucket kernel
        grows = plan.rows_grad_f32(gout, rec, C, G, stream_of(rows))
    if grows is None:
        perm, row_ptr = plan
        grows = _rows_grad_perm(gout, att, gate if gw is not None else None, None, perm, row_ptr, rec, 8, R, C, G, rows)
    return grows, gcompat


def _attn_bwd_lean_16(route, plan, rows, row_idx, compat, csr_idx, att, gate, amax, gw, gb, out, gout, gcompat, gwb,
                      scaling, eps):
    # bf16 rows (round 4; QKVBimodalCSRPool on the chain, and every bf16 caller with <= 4 score groups): the
    # chain path's attention backward (scores [V, 4] in, score gradients + 16-byte view records out) and its
    # 16-byte-record rows gradient instead of the team kernels: 1.6 + 1.3 -> 0.9 + 1.3 ms at V = 33.5 M
    from .fused_chain import build_tiles
    lib = _lib.load()
    N, V, (R, C), G = csr_idx.shape[0] - 1, row_idx.shape[0], rows.shape, compat.shape[1]
    tiles, n_tiles = build_tiles(csr_idx, V)
    vp = csr_expand(csr_idx, V)
    if G == 4:
        sc4 = compat
    else:
        sc4 = torch.zeros((V, 4), dtype=torch.float32, device=rows.device)
        sc4[:, :G] = compat
    dc = torch.empty((V, 4), dtype=torch.float32, device=rows.device)
    rec = torch.empty((V, 4), dtype=torch.int32, device=rows.device)
    with _timed("view_gather_attention_bwd", V * (C * 2 + 16 + 8 + 16 + 16) + N * (C * 2 + 8)):
        check(lib.dva_chain_attn_bwd_dt(
            ptr(sc4), ptr(vp), ptr(tiles), ptr(n_tiles), ptr(rows), ptr(row_idx), ptr(csr_idx), ptr(gw), ptr(gb),
            ptr(gout), ptr(out), ptr(dc), ptr(rec), ptr(gwb), N, V, R, C, G, scaling, eps, dtype_code(rows),
            stream_of(rows)), "dva_chain_attn_bwd_dt")
    plan = _plan_or_build(plan, row_idx, R, True)
    # bf16 / fp16: rounded where it is summed
    grows = rows_grad_rec16(gout, plan, rec, R, C, G, rows.dtype, stream_of(rows))
    return grows, (dc if G == 4 else dc[:, :G].contiguous())


def _attn_bwd_team(route, plan, rows, row_idx, compat, csr_idx, att, gate, amax, gw, gb, out, gout, gcompat, gwb,
                   scaling, eps):
    lib = _lib.load()
    N, V, (R, C), G = csr_idx.shape[0] - 1, row_idx.shape[0], rows.shape, compat.shape[1]
    es = rows.element_size()
    grows = torch.zeros((R, C), dtype=torch.float32, device=rows.device) if route.rows_grad == "atomics" else None
    # per-view records (point id | gate * attention per group) for the rows-gradient pass: one 32-byte
    # sector per view instead of scattered reads of view_point, att and gate
    rs = ((G + 1 + 7) // 8) * 8
    rec = torch.empty((V, rs), dtype=torch.float32, device=rows.device) if route.records else None
    per_view = C * es + 4 + 2 * G * 4 + (C * 4 * 2 if grows is not None else 0) + (rs * 4 if rec is not None else 0)
    with _timed("view_gather_attention_bwd", V * per_view + N * (C * es + 8 + 3 * G * 4)):
        check(lib.dva_view_gather_attention_bwd(
            ptr(gout), ptr(rows), ptr(row_idx), ptr(compat), ptr(att), ptr(gate), ptr(amax), ptr(csr_idx), ptr(gw), ptr(gb),
            ptr(grows), ptr(gcompat), ptr(gwb), ptr(rec), rs, N, V, C, G, scaling, dtype_code(rows), ATTENTION_ALGO,
            stream_of(rows)), "dva_view_gather_attention_bwd")
    if route.rows_grad == "plan":
        perm, row_ptr = _plan_or_build(plan, row_idx, R, False)
        vp = csr_expand(csr_idx, V) if rec is None else None
        grows = _rows_grad_perm(gout, att, gate if gw is not None else None, vp, perm, row_ptr, rec, rs, R, C, G, rows)
    return (grows.to(rows.dtype) if grows is not None else None), gcompat


class _ViewGatherAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, row_idx, compat, csr_idx, gate_w, gate_b, scaling, eps, plan):
        lib = _lib.load()
        require_device(rows, row_idx, compat, csr_idx, gate_w, gate_b)
        ctx.plan = plan
        rows = rows.contiguous()
        compat = compat.contiguous()
        N, V, (R, C), G = csr_idx.shape[0] - 1, row_idx.shape[0], rows.shape, compat.shape[1]
        gw = gate_w.detach().reshape(-1).float().contiguous() if gate_w is not None else None
        gb = gate_b.detach().reshape(-1).float().contiguous() if gate_b is not None else None
        if (gw is None) != (gb is None):
            gw = gw if gw is not None else torch.ones(G, device=rows.device)
            gb = gb if gb is not None else torch.zeros(G, device=rows.device)
        out = torch.empty((N, C), dtype=rows.dtype, device=rows.device)
        att = torch.empty((V, G), dtype=torch.float32, device=rows.device)   # every view belongs to a point
        gate = torch.empty((N, G), dtype=torch.float32, device=rows.device)
        amax = torch.empty((N, G), dtype=torch.int32, device=rows.device)
        es = rows.element_size()
        # SURVEY.md 8(d) "fused view-gather+attention": V*(g*C*s + idx) + scores + N*(C*s + ptr)
        with _timed("view_gather_attention_fwd", V * (C * es + 4 + 2 * G * 4) + N * (C * es + 8 + 2 * G * 4)):
            check(lib.dva_view_gather_attention_fwd(
                ptr(rows), ptr(row_idx), ptr(compat), ptr(csr_idx), ptr(gw), ptr(gb), ptr(out), ptr(att),
                ptr(gate), ptr(amax), N, V, C, G, int(scaling), float(eps), dtype_code(rows),
                ATTENTION_ALGO, stream_of(rows)), "dva_view_gather_attention_fwd")
        ctx.save_for_backward(rows, row_idx, compat, csr_idx, att, gate, amax,
                              gw if gw is not None else csr_idx, gb if gb is not None else csr_idx, out)
        ctx.meta = (int(scaling), gw is not None,
                    None if gate_w is None else gate_w.shape, None if gate_b is None else gate_b.shape)
        ctx.eps = float(eps)
        ctx.mark_non_differentiable(att, gate)
        return out, att, gate

    @staticmethod
    def backward(ctx, gout, _gatt, _ggate):
        rows, row_idx, compat, csr_idx, att, gate, amax, gw, gb, out = ctx.saved_tensors
        scaling, has_gate, w_shape, b_shape = ctx.meta
        if not has_gate:
            gw = gb = None      # (placeholders in saved_tensors)
        gout = gout.contiguous()
        N, V, (R, C), G = csr_idx.shape[0] - 1, row_idx.shape[0], rows.shape, compat.shape[1]
        gcompat = torch.empty_like(compat)             # every view is written (it belongs to a point)
        gwb = torch.zeros(2 * G, dtype=torch.float32, device=rows.device) if has_gate else None
        route = attention_bwd_route(rows.dtype, gout.dtype, out.dtype, C, G, V, R, N, ctx.needs_input_grad[0],
                                    rows.data_ptr() % 16 == 0 and gout.data_ptr() % 16 == 0)
        helper = {"lean_f32": _attn_bwd_lean_f32, "lean_16": _attn_bwd_lean_16, "team": _attn_bwd_team}[route.kernel]
        grows, gcompat = helper(route, ctx.plan, rows, row_idx, compat, csr_idx, att, gate, amax, gw, gb, out, gout,
                                gcompat, gwb, scaling, ctx.eps)
        g_w, g_b = _gate_grads(gwb, G, has_gate, w_shape, b_shape)
        return grows, None, gcompat, None, g_w, g_b, None, None, None


def view_gather_attention(rows, row_idx, compat, csr_idx, gate_w=None, gate_b=None, scaling=False,
                          eps=1e-12, plan=None):
    """``view_attention`` with the view gather fused in: the value of view v is ``rows[row_idx[v]]``.
    ``plan`` = ``row_plan(row_idx, R)[0]`` if the caller already has it (else built in backward)."""
    csr_idx = _check_ptr(csr_idx)
    if compat.dim() == 1:
        compat = compat.reshape(-1, 1)
    return _ViewGatherAttention.apply(rows, row_idx.contiguous(), compat.float(), csr_idx, gate_w, gate_b,
                                      scaling, eps, plan)


# ---------------------------------------------------------------------------------------------
# E_mod on the feature-map rows: tall-skinny Linear + weighted BatchNorm + LeakyReLU
# ---------------------------------------------------------------------------------------------

def _xty_splitk(a, b, splits=64):
    """``a.T @ b`` for tall operands [R, O], [R, I] -> fp32 [O, I].  A plain GEMM call runs this
    K = R reduction in ONE 64x64 tile (one workgroup, 0.5 ms at R = 262144); ``splits`` batched
    products of R / splits rows fill the device, the partial sums are added in fp32."""
    R = a.shape[0]
    if R < 8192 or R % splits:
        return a.float().t() @ b.float()
    part = torch.bmm(a.view(splits, R // splits, -1).transpose(1, 2), b.view(splits, R // splits, -1))
    return part.sum(0, dtype=torch.float32)        # one reduction kernel (fp32 accumulation), no fp32 copy of `part`


def xty_tall(a, b, splits=64):
    """``_xty_splitk`` for any number of rows: the split-K product over the largest multiple of ``splits`` rows and a
    plain product over the rest (fewer than ``splits`` rows).  [R, O], [R, I] -> fp32 [O, I]."""
    R = a.shape[0]
    main = R - R % splits
    if main < 8192:
        return a.float().t() @ b.float()
    a, b = a.contiguous(), b.contiguous()
    out = _xty_splitk(a[:main], b[:main], splits)
    return out if main == R else out.addmm_(a[main:].float().t(), b[main:].float())


class _TallLinear(torch.autograd.Function):
    """``F.linear`` whose weight gradient is a split-K product (same forward, same autocast rule)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        dt = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled('cuda') else x.dtype
        xc, wc = x.to(dt), weight.to(dt)
        ctx.save_for_backward(xc, wc)
        ctx.meta = (x.dtype, weight.dtype, None if bias is None else bias.dtype)
        return torch.nn.functional.linear(xc, wc, None if bias is None else bias.to(dt))

    @staticmethod
    def backward(ctx, gy):
        xc, wc = ctx.saved_tensors
        x_dt, w_dt, b_dt = ctx.meta
        gy = gy.contiguous()
        gx = (gy @ wc).to(x_dt) if ctx.needs_input_grad[0] else None
        gw = _xty_splitk(gy, xc).to(w_dt) if ctx.needs_input_grad[1] else None
        gb = gy.float().sum(0).to(b_dt) if (b_dt is not None and ctx.needs_input_grad[2]) else None
        return gx, gw, gb


def tall_linear(x, weight, bias=None):
    return _TallLinear.apply(x, weight, bias)


class _RowBNAct(torch.autograd.Function):
    """``leaky(BatchNorm(y))`` on map rows with the statistics weighted by ``counts`` (views per row).
    ``mean`` / ``invstd`` are given (batch statistics from ``rowbn_stats`` or running statistics);
    with ``batch_stats`` the backward includes the statistics terms."""

    @staticmethod
    def forward(ctx, y, counts, gamma, beta, mean, invstd, n, batch_stats, slope, bn_tab=None):
        lib = _lib.load()
        require_device(y)
        y = y.contiguous()
        R, C = y.shape
        if bn_tab is None:
            g = gamma.detach().float() if gamma is not None else torch.ones(C, device=y.device)
            b = beta.detach().float() if beta is not None else torch.zeros(C, device=y.device)
            bn_tab = torch.stack([mean.float(), invstd.float(), g, b]).contiguous()
        bn = bn_tab
        out = torch.empty_like(y)
        with _timed("rowbn_apply", R * C * 2 * y.element_size()):
            check(lib.dva_rowbn_apply(ptr(y), ptr(bn), ptr(out), R, C, float(slope), dtype_code(y),
                                      stream_of(y)), "dva_rowbn_apply")
        ctx.save_for_backward(y, bn, *([counts] if counts is not None else []))
        # the same clamped normaliser as the forward's statistics (bn_table): a sample without views has n = 0
        ctx.meta = (max(float(n), 1.0), bool(batch_stats), float(slope), gamma is not None, beta is not None)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        y, bn = ctx.saved_tensors[:2]
        counts = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        n, batch_stats, slope, has_g, has_b = ctx.meta
        R, C = y.shape
        gout = gout.contiguous().to(y.dtype)
        sums = zeros_small(2 * C, torch.float64, y.device)
        with _timed("rowbn_bwd_stats", R * C * 2 * y.element_size()):
            check(lib.dva_rowbn_bwd_stats(ptr(gout), ptr(y), ptr(bn), ptr(sums), R, C, slope, dtype_code(y),
                                          stream_of(y)), "dva_rowbn_bwd_stats")
        small = torch.empty(4 * C, dtype=torch.float32, device=y.device)    # S/n [2C] | d gamma [C] | d beta [C]
        sm, dg, db = small[:2 * C], small[2 * C:3 * C], small[3 * C:]
        check(lib.dva_bn_bwd_consts(ptr(sums), None, (1.0 / n) if batch_stats else 0.0, 0, ptr(sm), ptr(dg), ptr(db),
                                    C, stream_of(y)), "dva_bn_bwd_consts")
        dy = torch.empty_like(y)
        with _timed("rowbn_bwd_apply", R * C * 3 * y.element_size()):
            check(lib.dva_rowbn_bwd_apply(ptr(gout), ptr(y), ptr(counts), ptr(bn), ptr(sm), ptr(dy), R, C, slope,
                                          dtype_code(y), stream_of(y)), "dva_rowbn_bwd_apply")
        return dy, None, dg if has_g else None, db if has_b else None, None, None, None, None, None, None


def rowbn_sums(y, counts):
    """sum_r counts_r y_r | sum_r counts_r y_r^2 as one float64 [2C] tensor."""
    lib = _lib.load()
    require_device(y)
    y = y.contiguous()
    R, C = y.shape
    sums = zeros_small(2 * C, torch.float64, y.device)
    with _timed("rowbn_stats", R * (C * y.element_size() + 4)):
        check(lib.dva_rowbn_stats(ptr(y), ptr(counts), ptr(sums), R, C, dtype_code(y), stream_of(y)),
              "dva_rowbn_stats")
    return sums


def bn_table(sums, n, bn, batch_stats):
    """fp32 [4, C] = mean | invstd | gamma | beta of an nn.BatchNorm1d from the float64 sums of its input over ``n``
    rows (or from the running statistics), running statistics updated as the module does: one launch."""
    lib = _lib.load()
    C = bn.num_features
    dev = (bn.weight if bn.affine else (sums if sums is not None else bn.running_mean)).device
    out = torch.empty((4, C), dtype=torch.float32, device=dev)
    update = batch_stats and bn.training and bn.track_running_stats
    check(lib.dva_bn_finalize(ptr(sums), float(max(n, 1.0)), ptr(bn.running_mean if (update or not batch_stats) else None),
                              ptr(bn.running_var if (update or not batch_stats) else None),
                              ptr(bn.num_batches_tracked if update else None),
                              ptr(bn.weight.detach()) if bn.affine else None,
                              ptr(bn.bias.detach()) if bn.affine else None,
                              float(bn.momentum), float(bn.eps), 1 if batch_stats else 0, C, ptr(out),
                              stream_of(out)), "dva_bn_finalize")
    return out


def rowbn_stats(y, counts):
    """(sum_r counts_r y_r, sum_r counts_r y_r^2) as float64 [C] each."""
    sums = rowbn_sums(y, counts)
    C = y.shape[1]
    return sums[:C], sums[C:]


def rowbn_act(y, counts, gamma, beta, mean, invstd, n, batch_stats, slope, bn_tab=None):
    return _RowBNAct.apply(y, counts, gamma, beta, mean, invstd, n, batch_stats, slope, bn_tab)


# ---------------------------------------------------------------------------------------------
# E_mod on the map rows, fused: two blocks of Linear + weighted BatchNorm + LeakyReLU in six row passes
# (csrc/emod_rows.hip) instead of library GEMMs, casts and rowbn passes
# ---------------------------------------------------------------------------------------------
EMOD_FUSED = True             # False: pooling.mlp_on_gathered_rows keeps the composition (the A/B partner in tests)
EMOD_ROWS_MAX_BLOCKS = 0      # test hook: cap of the launch grids of the fused row kernels (0: the default grid)
EMOD_ROWS_WIDTHS = (32, 64)
EMOD_ROWS_MAX_BYTES = 0xfffffff0      # (R + 32) * 128 stays below it: 32-bit byte offsets, the rows of a last tile included


def emod_rows_serves(rows, counts, linears, norms):
    """Whether ``emod_rows`` covers this MLP on these rows: two blocks of Linear (no bias, fp32 weight, widths 32 / 64)
    and train-mode BatchNorm1d (fp32 parameters and buffers, a momentum) on contiguous 16-byte-aligned bf16 rows."""
    if len(linears) != 2 or not isinstance(rows, torch.Tensor):
        return False
    if not (rows.is_cuda and rows.dim() == 2 and rows.dtype == torch.bfloat16 and rows.is_contiguous()
            and rows.data_ptr() % 16 == 0 and rows.shape[0] > 0
            and (rows.shape[0] + 32) * 128 <= EMOD_ROWS_MAX_BYTES):
        return False
    if torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') != torch.bfloat16:
        return False
    if counts is not None and not (counts.dtype == torch.int32 and counts.is_cuda and counts.is_contiguous()
                                   and counts.shape == (rows.shape[0],)):
        return False
    c_in = rows.shape[1]
    for lin, bn in zip(linears, norms):
        w = lin.weight
        if not (lin.bias is None and w.dtype == torch.float32 and w.is_cuda and w.is_contiguous()
                and w.data_ptr() % 16 == 0 and w.shape[1] == c_in and c_in in EMOD_ROWS_WIDTHS
                and w.shape[0] in EMOD_ROWS_WIDTHS):
            return False
        if not (isinstance(bn, torch.nn.BatchNorm1d) and bn.training and bn.momentum is not None
                and bn.num_features == w.shape[0]
                and all(t is None or (t.dtype == torch.float32 and t.is_cuda)
                        for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))):
            return False
        c_in = w.shape[0]
    return True


def emod_rows_forward(x, counts, w_a, w_b, bn_a, bn_b, n, slope_a, slope_b, max_blocks=0):
    """The three forward passes; returns ``out`` and what the backward reads: y_a, y_b, the two BatchNorm tables
    (the running statistics of ``bn_a`` / ``bn_b`` are updated as the modules do)."""
    lib = _lib.load()
    require_device(x, counts, w_a, w_b)
    R, c_i = x.shape
    c_m, c_o = w_a.shape[0], w_b.shape[0]
    st, dev, mb = stream_of(x), x.device, int(max_blocks)
    sums_a = zeros_small(2 * c_m, torch.float64, dev)
    y_a = torch.empty((R, c_m), dtype=torch.bfloat16, device=dev)
    with _timed("emod_rows_fwd", R * (c_i + c_m) * 2):
        check(lib.dva_emod_rows_fwd(ptr(x), ptr(w_a), None, ptr(counts), ptr(y_a), ptr(sums_a), R, c_i, c_m, 0.0, mb,
                                    st), "dva_emod_rows_fwd")
    tab_a = bn_table(sums_a, n, bn_a, True)
    sums_b = zeros_small(2 * c_o, torch.float64, dev)
    y_b = torch.empty((R, c_o), dtype=torch.bfloat16, device=dev)
    with _timed("emod_rows_fwd", R * (c_m + c_o) * 2):
        check(lib.dva_emod_rows_fwd(ptr(y_a), ptr(w_b), ptr(tab_a), ptr(counts), ptr(y_b), ptr(sums_b), R, c_m, c_o,
                                    float(slope_a), mb, st), "dva_emod_rows_fwd")
    tab_b = bn_table(sums_b, n, bn_b, True)
    out = torch.empty_like(y_b)
    with _timed("emod_rows_fwd", R * c_o * 4):
        check(lib.dva_rowbn_apply(ptr(y_b), ptr(tab_b), ptr(out), R, c_o, float(slope_b), _lib.DVA_BF16, st),
              "dva_rowbn_apply")
    return dict(out=out, y_a=y_a, y_b=y_b, tab_a=tab_a, tab_b=tab_b, sums_a=sums_a, sums_b=sums_b)


def emod_rows_backward(gout, x, counts, w_a, w_b, fwd, n, slope_a, slope_b, need_gx=True, max_blocks=0):
    """The three backward passes from ``gout`` [R, C_out] bf16 and the forward's tensors; returns g_x (None unless
    ``need_gx``), the six parameter gradients and the stored intermediate g_a."""
    lib = _lib.load()
    R, c_i = x.shape
    c_m, c_o = w_a.shape[0], w_b.shape[0]
    st, dev, mb = stream_of(x), x.device, int(max_blocks)
    inv_n = 1.0 / max(float(n), 1.0)      # the clamped normaliser of bn_table
    y_a, y_b, tab_a, tab_b = fwd["y_a"], fwd["y_b"], fwd["tab_a"], fwd["tab_b"]
    small = torch.empty(4 * (c_o + c_m), dtype=torch.float32, device=dev)    # per layer: S/n [2C] | d gamma | d beta
    sm_b, dg_b, db_b = small[:2 * c_o], small[2 * c_o:3 * c_o], small[3 * c_o:4 * c_o]
    o = 4 * c_o
    sm_a, dg_a, db_a = small[o:o + 2 * c_m], small[o + 2 * c_m:o + 3 * c_m], small[o + 3 * c_m:]
    sums_b = zeros_small(2 * c_o, torch.float64, dev)
    with _timed("emod_rows_bwd", R * c_o * 4):
        check(lib.dva_rowbn_bwd_stats(ptr(gout), ptr(y_b), ptr(tab_b), ptr(sums_b), R, c_o, float(slope_b),
                                      _lib.DVA_BF16, st), "dva_rowbn_bwd_stats")
    check(lib.dva_bn_bwd_consts(ptr(sums_b), None, inv_n, 0, ptr(sm_b), ptr(dg_b), ptr(db_b), c_o, st),
          "dva_bn_bwd_consts")
    parts = int(lib.dva_emod_rows_grid(R, 1, mb))
    n_b, n_a = c_o * c_m, c_m * c_i
    ws = torch.empty(parts * (n_b + n_a), dtype=torch.float32, device=dev)
    ws_b, ws_a = ws[:parts * n_b], ws[parts * n_b:]
    g_a = torch.empty((R, c_m), dtype=torch.bfloat16, device=dev)
    sums_a = zeros_small(2 * c_m, torch.float64, dev)
    with _timed("emod_rows_bwd", R * (2 * c_o + 2 * c_m) * 2 + parts * n_b * 4):
        check(lib.dva_emod_rows_bwd(ptr(gout), ptr(y_b), ptr(tab_b), ptr(sm_b), ptr(counts), ptr(y_a), ptr(tab_a),
                                    ptr(w_b), ptr(g_a), ptr(ws_b), ptr(sums_a), R, c_m, c_o, float(slope_b),
                                    float(slope_a), mb, st), "dva_emod_rows_bwd")
    check(lib.dva_bn_bwd_consts(ptr(sums_a), None, inv_n, 0, ptr(sm_a), ptr(dg_a), ptr(db_a), c_m, st),
          "dva_bn_bwd_consts")
    g_x = torch.empty((R, c_i), dtype=torch.bfloat16, device=dev) if need_gx else None
    with _timed("emod_rows_bwd", R * (2 * c_m + (2 if need_gx else 1) * c_i) * 2 + parts * n_a * 4):
        check(lib.dva_emod_rows_bwd(ptr(g_a), ptr(y_a), ptr(tab_a), ptr(sm_a), ptr(counts), ptr(x), None, ptr(w_a),
                                    ptr(g_x), ptr(ws_a), None, R, c_i, c_m, float(slope_a), 0.0, mb, st),
              "dva_emod_rows_bwd")
    dw = torch.empty(n_b + n_a, dtype=torch.float32, device=dev)
    with _timed("emod_rows_bwd", (parts + 1) * (n_b + n_a) * 4):
        check(lib.dva_emod_rows_dw_reduce(ptr(ws_b), n_b, parts, ptr(dw), ptr(ws_a), n_a, parts, ptr(dw[n_b:]), st),
              "dva_emod_rows_dw_reduce")
    return dict(g_x=g_x, g_a=g_a, dw_a=dw[n_b:].view(c_m, c_i), dw_b=dw[:n_b].view(c_o, c_m), dgamma_a=dg_a,
                dbeta_a=db_a, dgamma_b=dg_b, dbeta_b=db_b, sm_a=sm_a, sm_b=sm_b)


class _EmodRows(torch.autograd.Function):
    """``mlp(rows[row_idx])`` evaluated on the map rows (``pooling.mlp_on_gathered_rows``) for a two-block MLP the
    fused row kernels cover (``emod_rows_serves``)."""

    @staticmethod
    def forward(ctx, x, counts, w_a, gamma_a, beta_a, w_b, gamma_b, beta_b, bn_a, bn_b, n, slope_a, slope_b,
                max_blocks):
        fwd = emod_rows_forward(x, counts, w_a, w_b, bn_a, bn_b, n, slope_a, slope_b, max_blocks)
        ctx.save_for_backward(x, w_a, w_b, fwd["y_a"], fwd["y_b"], fwd["tab_a"], fwd["tab_b"],
                              *([counts] if counts is not None else []))
        ctx.meta = (float(n), float(slope_a), float(slope_b), int(max_blocks))
        return fwd["out"]

    @staticmethod
    def backward(ctx, gout):
        x, w_a, w_b, y_a, y_b, tab_a, tab_b = ctx.saved_tensors[:7]
        counts = ctx.saved_tensors[7] if len(ctx.saved_tensors) > 7 else None
        n, slope_a, slope_b, mb = ctx.meta
        gout = gout.contiguous().to(torch.bfloat16)
        if gout.data_ptr() % 16:
            gout = gout.clone()
        need = ctx.needs_input_grad
        g = emod_rows_backward(gout, x, counts, w_a, w_b, dict(y_a=y_a, y_b=y_b, tab_a=tab_a, tab_b=tab_b), n, slope_a,
                               slope_b, need[0], mb)
        return (g["g_x"], None, g["dw_a"] if need[2] else None, g["dgamma_a"] if need[3] else None,
                g["dbeta_a"] if need[4] else None, g["dw_b"] if need[5] else None,
                g["dgamma_b"] if need[6] else None, g["dbeta_b"] if need[7] else None, None, None, None, None, None,
                None)


def emod_rows(x, counts, linears, norms, slopes, n, max_blocks=None):
    """Two blocks of Linear -> weighted BatchNorm1d -> LeakyReLU on the rows ``x`` [R, C] (bf16), ``counts`` views per
    row (None: one each), ``n`` views in all: six row passes (csrc/emod_rows.hip).  ``emod_rows_serves`` says when."""
    (lin_a, lin_b), (bn_a, bn_b) = linears, norms
    mb = EMOD_ROWS_MAX_BLOCKS if max_blocks is None else max_blocks
    return _EmodRows.apply(x, counts, lin_a.weight, bn_a.weight if bn_a.affine else None,
                           bn_a.bias if bn_a.affine else None, lin_b.weight, bn_b.weight if bn_b.affine else None,
                           bn_b.bias if bn_b.affine else None, bn_a, bn_b, float(n), float(slopes[0]),
                           float(slopes[1]), int(mb))


# ---------------------------------------------------------------------------------------------
# voxel parent index after a strided sparse 3D convolution (modules.py:176-198)
# ---------------------------------------------------------------------------------------------

def voxel_parent_index(in_coords, out_coords, stride_out, batch_col=3):
    """``idx[i] = j`` with ``out_coords[j] == floor_to_stride(in_coords[i])`` (batch column untouched),
    ``-1`` when absent: the torchsparse ``sphashquery(sphash(in), sphash(out))`` of the reference."""
    lib = _lib.load()
    require_device(in_coords, out_coords)
    assert in_coords.dim() == 2 and in_coords.shape[1] == 4 and out_coords.dim() == 2 and out_coords.shape[1] == 4
    ic = in_coords.to(torch.int32).contiguous()
    oc = out_coords.to(torch.int32).contiguous()
    n_in, n_out = ic.shape[0], oc.shape[0]
    idx = torch.empty(n_in, dtype=torch.int64, device=ic.device)
    ws, nbytes = _lib.workspace("dva_voxel_parent_workspace_bytes", ic.device, n_out)
    with _timed("voxel_parent_index", n_in * 24 + n_out * 24):
        check(lib.dva_voxel_parent_index(ptr(ic), n_in, ptr(oc), n_out, int(stride_out), int(batch_col), ptr(idx),
                                         ptr(ws), int(nbytes), stream_of(ic)), "dva_voxel_parent_index")
    return idx


# ---------------------------------------------------------------------------------------------
# mapping merge after a strided 3D convolution (core/multimodal/image.py:2211-2273 + :1728-1795)
# ---------------------------------------------------------------------------------------------
MERGE_TILE_ATOMS = 512      # atoms of a voxel merged in LDS (dva_mapping_merge_tile_atoms); larger voxels sort in the workspace


def _unsupported(op, what):
    """The ``DvaError`` with ``code == DVA_ERR_UNSUPPORTED`` of ``ops.<op>``: the callers take their composition."""
    code = _lib.DVA_ERR_UNSUPPORTED
    return _lib.DvaError(f"ops.{op}: {what}: {_lib._ERRORS[code]}", code=code)


def _mapping_arguments(op, pointers, images, atom_ptr=None, pixels=None, features=None, *, features_dtype=torch.float32,
                       item=None, dev=None, **index_vectors):
    """The argument checks of the ops on the nested mapping CSR ``pointers`` -> ``images`` / ``atom_ptr`` -> ``pixels``
    (+ ``features``): ``(device, points, views, atoms)``, ``points`` / ``atoms`` None without ``pointers`` / ``pixels``.
    One order for every op: shapes (``ValueError``), then what the kernels do not take -- index tensors (the extra
    ``index_vectors`` by name as well) other than int64, pixels other than int16, features other than
    ``features_dtype`` (None: any), 2^31 - 1 or more points, views or atoms -- (``DvaError`` with code -2), then the
    device (``DvaError`` without a code; ``dev``: the device of the items before).  Reads shapes, dtypes and devices
    only; ``op`` and ``item`` go into the messages and nowhere else."""
    of = "" if item is None else f" of item {item}"
    index = dict(pointers=pointers, images=images, atom_ptr=atom_ptr, **index_vectors)
    for name, t in index.items():
        if t is not None and t.dim() != 1:
            raise ValueError(f"ops.{op}: {name}{of} must be 1-D, got {tuple(t.shape)}")
    if pixels is not None and (pixels.dim() != 2 or pixels.shape[1] != 2):
        raise ValueError(f"ops.{op}: pixels{of} must be [P, 2], got {tuple(pixels.shape)}")
    n = None if pointers is None else pointers.shape[0] - 1
    v = images.shape[0]
    p = None if pixels is None else pixels.shape[0]
    if atom_ptr is not None and atom_ptr.shape[0] != v + 1:
        raise ValueError(f"ops.{op}: atom_ptr{of} must have {v + 1} entries for {v} views, got {atom_ptr.shape[0]}")
    if features is not None and (features.dim() < 1 or features.shape[0] != v):
        raise ValueError(f"ops.{op}: features{of} must be [{v}, ...], got {tuple(features.shape)}")
    for name, t in index.items():
        if t is not None and t.dtype != torch.int64:
            raise _unsupported(op, f"{name}{of} is {t.dtype}, not int64")
    if pixels is not None and pixels.dtype != torch.int16:
        raise _unsupported(op, f"pixels{of} are {pixels.dtype}, not int16")
    if features is not None and features_dtype is not None and features.dtype != features_dtype:
        raise _unsupported(op, f"features{of} are {features.dtype}, not {features_dtype}")
    if max(n or 0, v, p or 0) >= 2 ** 31 - 1:
        raise _unsupported(op, f"{n} points, {v} views, {p} atoms{of}")
    device = require_device(*index.values(), pixels, features)
    if dev is not None and device != dev:
        raise _lib.DvaError(f"tensors on different devices: {dev} vs {device}")
    return device, n, v, p


def _mapping_outputs(dev, n, v, p, f):
    """The five tensors of a mapping of ``n`` points, ``v`` views and ``p`` atoms: ``(pointers, images, atom_ptr,
    pixels, features)``, the features fp32 ``[v, f]`` (``f`` may be 0), None for ``f`` None."""
    return (torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(v, dtype=torch.int64, device=dev),
            torch.empty(v + 1, dtype=torch.int64, device=dev), torch.empty((p, 2), dtype=torch.int16, device=dev),
            None if f is None else torch.empty((v, f), dtype=torch.float32, device=dev))


def _mapping_workspace(op, query, dev, what, *args):
    """``_lib.workspace(query, dev, *args)``; sizes the query refuses are what ``ops.<op>`` does not take."""
    ws = _lib.unless_unsupported(_lib.workspace, query, dev, *args)
    if ws is None:
        raise _unsupported(op, what)
    return ws


def merge_mapping(pointers, images, atom_ptr, pixels, features, idx):
    """Mapping of the voxels ``idx[i]`` of the points of a mapping: ``(pointers', images', atom_ptr', pixels',
    features', ok)``.  The views of the points of a voxel are united per image (ascending image id), the pixels of a
    merged view are its distinct (x, y) in ascending order, its features the fp32 mean of the source views in
    ascending point order (``features`` [V, F] or [V] or None).  ``ok`` is False, and the inputs come back, when
    ``idx`` is not one id per point or some id below ``max(idx)`` has no point (the reference returns the mapping
    unchanged then).  One host synchronisation: the readback of the output sizes.  Raises ``DvaError`` with
    ``code == -2`` for what the kernels do not take (pixels other than int16, indices other than int64, 2^31 or more
    views or atoms)."""
    lib = _lib.load()
    dev, n, v, p = _mapping_arguments("merge_mapping", pointers, images, atom_ptr, pixels, features,
                                      features_dtype=None, idx=idx)
    if n < 1:
        raise ValueError(f"ops.merge_mapping: pointers of {n} points")
    if features is not None and features.dim() > 2:
        raise ValueError(f"ops.merge_mapping: features must be [{v}, F] or [{v}], got {tuple(features.shape)}")
    if idx.shape[0] != n:
        return pointers, images, atom_ptr, pixels, features, False
    ws, nbytes = _mapping_workspace("merge_mapping", "dva_mapping_merge_workspace_bytes", dev,
                                    f"{n} points, {v} views, {p} atoms", n, v, p)
    pointers, images, atom_ptr = pointers.contiguous(), images.contiguous(), atom_ptr.contiguous()
    pixels, idx = pixels.contiguous(), idx.contiguous()
    feat = None
    if features is not None:
        feat = features.detach().float().reshape(v, -1).contiguous()
    f = 0 if feat is None else feat.shape[1]
    feat_in = feat if f > 0 else None
    sizes = torch.empty(4, dtype=torch.int64, device=dev)
    s = stream_of(pointers)
    read = n * 8 + v * 16 + p * 4
    with _timed("mapping_merge_count", read + n * 8):
        check(lib.dva_mapping_merge_count(ptr(pointers), ptr(images), ptr(atom_ptr), ptr(pixels), 2, ptr(idx), n, v, p,
                                          ptr(sizes), ptr(ws), int(nbytes), s), "dva_mapping_merge_count")
    m, v_out, p_out, ok = sizes.tolist()                  # host read: the sizes of the outputs
    if not ok:
        return pointers, images, atom_ptr, pixels, features, False
    out_ptr, out_img, out_aptr, out_pix, out_feat = _mapping_outputs(dev, m, v_out, p_out, None if feat is None else f)
    with _timed("mapping_merge_fill", read + v * f * 4 + m * 8 + v_out * 16 + p_out * 4 + v_out * f * 4):
        check(lib.dva_mapping_merge_fill(ptr(pointers), ptr(images), ptr(atom_ptr), ptr(pixels), 2, ptr(feat_in), f,
                                         n, v, p, m, v_out, p_out, ptr(out_ptr), ptr(out_img), ptr(out_aptr),
                                         ptr(out_pix), ptr(out_feat if f > 0 else None), ptr(ws), int(nbytes), s),
              "dva_mapping_merge_fill")
    if out_feat is not None and features.dim() == 1:
        out_feat = out_feat.view(-1)
    return out_ptr, out_img, out_aptr, out_pix, out_feat, True


# ---------------------------------------------------------------------------------------------
# mapping selection: pick, views, images, crop (core/multimodal/image.py:2029-2342, csr.py:235-294)
# ---------------------------------------------------------------------------------------------

def select_mapping(pointers, images, atom_ptr, pixels, features, *, point_idx=None, view_mask=None, image_map=None,
                   compact=False, crop=None, num_images=None, image_keys=None):
    """Filter, compact and renumber a mapping in one device operation: ``(pointers', images', atom_ptr', pixels',
    features', info)``.  Output point ``m`` is source point ``point_idx[m]`` (int64, any order, duplicates allowed;
    all points in order without it).  A source view survives if ``view_mask`` (bool [V]) is set for it and, with
    ``image_map`` (int64 [B]), if ``image_map[image] >= 0``, which is then its new image id; with ``image_keys``
    (int64 [K], ASCENDING) as well, ``image_map`` has one entry per key and a view survives if its image is a key with
    a new id ``>= 0`` -- the form that needs no bound on the image ids.  ``compact`` (exclusive with ``image_map``)
    gives a surviving view the rank of its image among the distinct surviving images, ``info['seen']``; it needs
    ``num_images``, above every image id.  ``crop = (W, H, offsets [B, 2])`` (exclusive with ``image_map`` and
    ``compact``; offsets indexed by image id): atom pixels become ``pixel - offset[image]`` in the pixel dtype, atoms
    outside ``[0, W) x [0, H)`` and views left without atoms are dropped, the surviving views of a point are ordered
    by ascending image id (stably), and the features of a view are the fp32 mean of ``c`` copies of its source
    features, ``c`` its surviving atoms, added one after the other.  Features are copied as bits otherwise.

    ``info``: ``seen`` (int64 device tensor: the distinct surviving images with ``compact``, the distinct images of
    the views that pass the mask with ``crop``, else None), ``seen_host`` (the same as a list), ``num_seen``,
    ``unsupported`` (a crop that leaves two views of one point with the same image, which ``from_dense`` would unite,
    or 2^31 or more views or atoms), ``out_of_range`` (a point index or image id outside its range) and
    ``duplicate_keys``.  With any of the three set the tensors are None.  One host synchronisation: the readback of
    sizes, flags and ``seen`` in one buffer.  Raises ``DvaError`` with ``code == -2`` for what the kernels do not take
    (pixels other than int16, indices other than int64, features other than fp32, 2^31 or more views or atoms)."""
    lib = _lib.load()
    dev, n, v, p = _mapping_arguments("select_mapping", pointers, images, atom_ptr, pixels, features,
                                      point_idx=point_idx, image_map=image_map, image_keys=image_keys)
    require_device(pointers, view_mask)
    if n < 1:
        raise ValueError(f"ops.select_mapping: pointers of {n} points")
    if features is not None and features.dim() > 2:
        raise ValueError(f"ops.select_mapping: features must be [{v}, F] or [{v}], got {tuple(features.shape)}")
    if view_mask is not None and (view_mask.dtype != torch.bool or tuple(view_mask.shape) != (v,)):
        raise ValueError(f"ops.select_mapping: view_mask must be bool [{v}]")
    if image_map is not None and (compact or crop is not None):
        raise ValueError("ops.select_mapping: image_map excludes compact and crop")
    if compact and crop is not None:
        raise ValueError("ops.select_mapping: compact excludes crop")
    if image_keys is not None and (image_map is None or image_map.shape != image_keys.shape):
        raise ValueError("ops.select_mapping: image_keys needs an image_map with one entry per key")
    m = n if point_idx is None else point_idx.shape[0]
    if m < 1:
        raise ValueError("ops.select_mapping: no output point")
    crop_w = crop_h = 0
    offsets = None
    b = 0
    if crop is not None:
        crop_w, crop_h, offsets = int(crop[0]), int(crop[1]), crop[2]
        require_device(pointers, offsets)
        if offsets.dim() != 2 or offsets.shape[1] != 2:
            raise ValueError(f"ops.select_mapping: crop offsets must be [B, 2], got {tuple(offsets.shape)}")
        if offsets.dtype != torch.int64:
            raise _unsupported("select_mapping", f"crop offsets are {offsets.dtype}, not int64")
        if crop_w < 1 or crop_h < 1:
            raise ValueError(f"ops.select_mapping: crop size {(crop_w, crop_h)}")
        offsets = offsets.contiguous()
        b = offsets.shape[0]
        if num_images is not None and int(num_images) != b:
            raise ValueError(f"ops.select_mapping: {b} crop offsets for num_images={num_images}")
    elif compact:
        if num_images is None:
            raise ValueError("ops.select_mapping: compact needs num_images")
        b = int(num_images)
    ws, nbytes = _mapping_workspace("select_mapping", "dva_mapping_select_workspace_bytes", dev,
                                    f"{m} points, {v} views, {b} images", m, v, b, int(crop is not None))
    pointers, images, atom_ptr, pixels = (pointers.contiguous(), images.contiguous(), atom_ptr.contiguous(),
                                          pixels.contiguous())
    point_idx, view_mask, image_map, image_keys = (None if t is None else t.contiguous()
                                                   for t in (point_idx, view_mask, image_map, image_keys))
    f = 0 if features is None else (1 if features.dim() == 1 else features.shape[1])
    feat = None if features is None else features.detach().reshape(v, f).contiguous()
    feat_in = feat if f > 0 else None
    n_map = 0 if image_map is None else image_map.shape[0]
    sizes = torch.empty(4 + b, dtype=torch.int64, device=dev)
    s = stream_of(pointers)
    sel = (ptr(point_idx), m, ptr(view_mask), ptr(image_keys), ptr(image_map), n_map, int(bool(compact)), b, crop_w,
           crop_h, ptr(offsets))
    read = m * 16 + v * (16 + (view_mask is not None)) + (p * 4 if crop is not None else 0)
    with _timed("mapping_select_count", read + m * 8):
        check(lib.dva_mapping_select_count(ptr(pointers), ptr(images), ptr(atom_ptr), ptr(pixels), 2, n, v, p, *sel,
                                           ptr(sizes), ptr(ws), int(nbytes), s), "dva_mapping_select_count")
    host = sizes.tolist()                                 # host read: sizes, flags and the seen images together
    v_out, p_out, n_seen, flags = host[:4]
    tracked = compact or crop is not None
    info = dict(seen=sizes[4:4 + n_seen] if tracked else None, seen_host=host[4:4 + n_seen] if tracked else None,
                num_seen=n_seen, unsupported=bool(flags & 1), out_of_range=bool(flags & 2),
                duplicate_keys=bool(flags & 4), num_views=v_out, num_atoms=p_out)
    if flags:
        return None, None, None, None, None, info
    out_ptr, out_img, out_aptr, out_pix, out_feat = _mapping_outputs(dev, m, v_out, p_out, None if feat is None else f)
    with _timed("mapping_select_fill", read + p * 4 + m * 8 + v_out * (16 + 8 * f) + p_out * 8):
        check(lib.dva_mapping_select_fill(ptr(pointers), ptr(images), ptr(atom_ptr), ptr(pixels), 2, ptr(feat_in), f,
                                          n, v, p, *sel, v_out, p_out, ptr(out_ptr), ptr(out_img), ptr(out_aptr),
                                          ptr(out_pix), ptr(out_feat if f > 0 else None), ptr(ws), int(nbytes), s),
              "dva_mapping_select_fill")
    if out_feat is not None:
        out_feat = out_feat.view((v_out,) + tuple(features.shape[1:]))
    return out_ptr, out_img, out_aptr, out_pix, out_feat, info


def mapping_image_stats(images, atom_ptr, pixels, num_images):
    """Per image id ``< num_images`` of a mapping: ``(count, x_min, x_max, y_min, y_max)``, int64 [num_images] each --
    its number of atoms and the bounding box of its pixels, by integer atomics (order-free).  An image without atoms
    has ``iinfo(int64).max`` / ``.min`` as minima / maxima, the sentinels of ``ImageMapping.bounding_boxes``.  No
    host synchronisation.  ``DvaError`` with ``code == -2`` for pixels other than int16 or indices other than int64."""
    lib = _lib.load()
    dev, _, v, p = _mapping_arguments("mapping_image_stats", None, images, atom_ptr, pixels)
    b = int(num_images)
    if b < 0:
        raise ValueError(f"ops.mapping_image_stats: {b} images")
    images, atom_ptr, pixels = images.contiguous(), atom_ptr.contiguous(), pixels.contiguous()
    stats = torch.empty((5, b), dtype=torch.int64, device=dev)
    with _timed("mapping_image_stats", v * 16 + p * 4 + b * 40):
        check(lib.dva_mapping_image_stats(ptr(images), ptr(atom_ptr), ptr(pixels), 2, v, p, b, ptr(stats),
                                          stream_of(images)), "dva_mapping_image_stats")
    return stats[0], stats[1], stats[2], stats[3], stats[4]


# ---------------------------------------------------------------------------------------------
# the image picks: CenterRoll and the coverage counts of PickImagesFromMemoryCredit
# (core/data_transform/multimodal/image.py:962-1037, :765-874)
# ---------------------------------------------------------------------------------------------

def mapping_center_rollings(images, atom_ptr, pixels, num_images, width, angular_res=16):
    """CenterRoll's offsets (reference :999-1029) in one device operation: ``(rollings, info)``.  ``rollings`` int64
    ``[num_images]``: per image the roll ``long(float(r) / 256 * width)`` of the first candidate ``r`` in
    ``arange(0, 256, int(256 / angular_res))`` that minimises span + centring distance of the image's atom columns in
    8-bit angular coordinates; 0 for an image without atoms.  ``info`` int32 ``[2]`` on the device: the number of images
    without atoms, and flags -- bit 0 a view whose image is outside ``[0, num_images)``, bit 1 an atom column outside
    ``[0, width)``; with a flag set the offsets leave those views / atoms out and the caller takes the composition.
    Integer arithmetic, exactly the reference's float expressions for ``width <= 32767``; integer OR atomics only, so
    two runs give the same bits.  No host synchronisation.  ``angular_res`` is an int in 1..256 (``ValueError``);
    ``DvaError`` with ``code == -2`` for pixels other than int16, indices other than int64 or ``width > 32767``."""
    lib = _lib.load()
    if not isinstance(angular_res, int) or isinstance(angular_res, bool) or not 1 <= angular_res <= 256:
        raise ValueError(f"ops.mapping_center_rollings: angular_res must be an int in 1..256, got {angular_res!r}")
    dev, _, v, p = _mapping_arguments("mapping_center_rollings", None, images, atom_ptr, pixels)
    b, w = int(num_images), int(width)
    if b < 0 or w < 1:
        raise ValueError(f"ops.mapping_center_rollings: {b} images of width {w}")
    if w > 32767:
        raise _unsupported("mapping_center_rollings", f"width {w} above 32767")
    images, atom_ptr, pixels = images.contiguous(), atom_ptr.contiguous(), pixels.contiguous()
    ws, nbytes = _lib.workspace("dva_mapping_center_workspace_bytes", dev, b)
    rollings = torch.empty(b, dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    with _timed("mapping_center_rollings", v * 16 + p * 4 + b * 72):
        check(lib.dva_mapping_center_rollings(ptr(images), ptr(atom_ptr), ptr(pixels), 2, v, p, b, w, angular_res,
                                              ptr(rollings), ptr(info), ptr(ws), int(nbytes), stream_of(images)),
              "dva_mapping_center_rollings")
    return rollings, info


def roll_mapping_pixels(images, atom_ptr, pixels, rollings, width):
    """The mapping half of ``update_rollings`` (reference :610-621) in one device operation, IN PLACE:
    ``pixels[a, 0] = (pixels[a, 0] + rollings[image of a]) % width`` for every atom ``a``.  ``pixels`` is int16
    ``[P, 2]`` and contiguous (it is written where it is, so a copy would be wrong: ``ValueError``), ``rollings`` int64
    ``[B]``.  Returns ``pixels``.  No host synchronisation.  ``DvaError`` with ``code == -2`` for pixels other than
    int16, indices other than int64 or ``width > 32767``."""
    lib = _lib.load()
    _, _, v, p = _mapping_arguments("roll_mapping_pixels", None, images, atom_ptr, pixels, rollings=rollings)
    w = int(width)
    if w < 1:
        raise ValueError(f"ops.roll_mapping_pixels: width {w}")
    if w > 32767:
        raise _unsupported("roll_mapping_pixels", f"width {w} above 32767")
    if not pixels.is_contiguous() or pixels.data_ptr() % 4:
        raise ValueError("ops.roll_mapping_pixels: pixels must be contiguous and 4-byte aligned to be rolled in place")
    images, atom_ptr, rollings = images.contiguous(), atom_ptr.contiguous(), rollings.contiguous()
    with _timed("roll_mapping_pixels", v * 16 + p * 8):
        check(lib.dva_mapping_roll_pixels(ptr(images), ptr(atom_ptr), ptr(pixels), 2, v, p, ptr(rollings),
                                          rollings.shape[0], w, stream_of(images)), "dva_mapping_roll_pixels")
    return pixels


class MappingCoverage:
    """The coverage counts of ``PickImagesFromMemoryCredit`` (reference :803-868) without its dense ``[B, N]``
    matrix.  ``items`` is a list of ``(pointers, images, num_images)``, one per setting: int64 device tensors of
    mappings over the SAME ``num_points`` points (a mapping may cover fewer).  Image ``j`` of item ``b`` has the global
    id ``bases[b] + j``, ``bases`` the running sum of ``num_images``.

    ``step(pick)`` marks the points that global image ``pick`` sees as covered (``pick = -1``: none) and returns
    ``counts`` int64 ``[total images]`` on the device, ``counts[i] = |{p : image i sees p, no picked image sees p}|``:
    the row sums of the reference's ``unseen`` after ``unseen &= ~unseen[pick]`` for every pick so far.  One launch per
    32 items, which also clears the row of the next step; integer atomics only (an LDS histogram per workgroup up to
    ``hist_images()`` images in all, global atomics above), so the counts are exact and order-free.  No host
    synchronisation; the tensor a step returns is valid until the step after the next.

    PRECONDITION: a view is a distinct (point, image) pair, as in every ``ImageMapping`` the library builds
    (``from_dense`` unites repeated pairs); a repeated pair would count twice.

    State: ``covered`` uint8 ``[num_points]`` and two count rows -- ``num_points + 16 * total`` bytes."""

    @staticmethod
    def hist_images():
        return int(_lib.load().dva_mapping_coverage_hist_images())

    def __init__(self, items, num_points):
        lib = _lib.load()
        if not isinstance(items, (list, tuple)) or len(items) == 0:
            raise ValueError("ops.MappingCoverage: a non-empty list of items")
        self.num_points = int(num_points)
        if self.num_points < 1:
            raise ValueError(f"ops.MappingCoverage: {self.num_points} points")
        self._keep = []
        self._descriptors = (_lib.DvaCoverageItem * len(items))()
        base, self.device = 0, None
        for b, (pointers, images, num_images) in enumerate(items):
            self.device, n, v, _ = _mapping_arguments("MappingCoverage", pointers, images, item=b, dev=self.device)
            k = int(num_images)
            if n < 0 or n > self.num_points or k < 0:
                raise ValueError(f"ops.MappingCoverage: item {b} has {n} points of {self.num_points} and {k} images")
            pointers, images = pointers.contiguous(), images.contiguous()
            self._keep.append((pointers, images))
            d = self._descriptors[b]
            d.pointers = pointers.data_ptr() if n > 0 else None
            d.images = images.data_ptr() if v > 0 else None
            d.n_points, d.n_views, d.n_images, d.image_base = n, v, k, base
            base += k
        self.num_images = base
        if self.num_images < 1:
            raise ValueError("ops.MappingCoverage: no image")
        if max(self.num_points, self.num_images) >= 2 ** 31 - 1:
            raise _unsupported("MappingCoverage", f"{self.num_points} points, {self.num_images} images")
        self._lib = lib
        self.covered = torch.zeros(self.num_points, dtype=torch.uint8, device=self.device)
        self._counts = torch.zeros((2, self.num_images), dtype=torch.int64, device=self.device)
        self._row = 0

    def step(self, pick=-1):
        pick = int(pick)
        if not -1 <= pick < self.num_images:
            raise ValueError(f"ops.MappingCoverage.step: pick {pick} outside [-1, {self.num_images})")
        counts, clear = self._counts[self._row], self._counts[1 - self._row]
        views = sum(d.n_views for d in self._descriptors)
        with _timed("mapping_coverage_step", self.num_points * 18 + views * 8 + self.num_images * 16):
            check(self._lib.dva_mapping_coverage_step(self._descriptors, len(self._descriptors), self.num_points,
                                                      self.num_images, pick, ptr(self.covered), ptr(counts), ptr(clear),
                                                      stream_of(self.covered)), "dva_mapping_coverage_step")
        self._row = 1 - self._row
        return counts


# ---------------------------------------------------------------------------------------------
# mapping collation: CSRBatch.from_csr_list on ImageMappings + insert_empty_groups (core/multimodal/csr.py:352-420)
# ---------------------------------------------------------------------------------------------

def collate_mapping(items, point_bases=None, num_points=None):
    """Stack mappings into one batch mapping in one device operation: ``(pointers, images, atom_ptr, pixels, features,
    image_offsets)``.  ``items`` is a list of ``(pointers, images, atom_ptr, pixels, features_or_None)`` device tensors
    (int64, int64, int64, int16 ``[P, 2]``, fp32 ``[V]`` or ``[V, ...]``; made contiguous where they are not).  Item
    ``b`` lands at the points ``point_bases[b] ...`` of the result (ascending, no overlap; back to back without
    ``point_bases``), which has ``num_points`` points (at least the end of the last item); the points no item covers
    are empty groups, as ``insert_empty_groups`` makes them.  Views, atom pointers and pixels follow in item order;
    the image ids of item ``b`` are raised by ``image_offsets[b]``, the sum over the items before it of
    ``max(images) + 1`` (0 for an item without views), int64 on the device.  Pixels and features are copied as bits;
    the features take the items' trailing shape back.  Items without points (``pointers == [0]``) or views are
    legal.  No host synchronisation: every size comes from a tensor shape.  Raises ``DvaError`` with ``code == -2``
    for what the kernel does not take: dtypes other than int64 / int16 / fp32, features on some items only, items
    whose features differ in their trailing shape, 2^31 - 1 or more points, views or atoms."""
    lib = _lib.load()
    if not isinstance(items, (list, tuple)) or len(items) == 0:
        raise ValueError("ops.collate_mapping: a non-empty list of items")
    with_features = [item[4] is not None for item in items]
    if any(with_features) and not all(with_features):
        raise _unsupported("collate_mapping", "features on some items only")
    trailing = dev = None
    rows, keep = [], []
    for b, item in enumerate(items):
        dev, n, v, p = _mapping_arguments("collate_mapping", *item, item=b, dev=dev)
        if n < 0:
            raise ValueError(f"ops.collate_mapping: pointers of item {b} are empty")
        features = item[4]
        if features is not None:
            if trailing is None:
                trailing = tuple(features.shape[1:])
            elif tuple(features.shape[1:]) != trailing:
                raise _unsupported("collate_mapping", f"features of item {b} are [V, {tuple(features.shape[1:])}], "
                                                      f"those of item 0 [V, {trailing}]")
        rows.append((n, v, p))
    f = 0 if trailing is None else int(np.prod(trailing, dtype=np.int64))
    if point_bases is None:
        bases = [0] * len(rows)
        for b in range(1, len(rows)):
            bases[b] = bases[b - 1] + rows[b - 1][0]
    else:
        bases = [int(x) for x in point_bases]
        if len(bases) != len(rows):
            raise ValueError(f"ops.collate_mapping: {len(bases)} point bases for {len(rows)} items")
    end = bases[-1] + rows[-1][0]
    n_out = end if num_points is None else int(num_points)
    v_out, p_out = sum(r[1] for r in rows), sum(r[2] for r in rows)
    if max(n_out, v_out, p_out) >= 2 ** 31 - 1:
        raise _unsupported("collate_mapping", f"{n_out} points, {v_out} views, {p_out} atoms")
    descriptors = (_lib.DvaCollateItem * len(rows))()
    for b, ((pointers, images, atom_ptr, pixels, features), (n, v, p)) in enumerate(zip(items, rows)):
        # (no aten call for what is contiguous already: a batch is launch-bound, and so is the host in front of it)
        pointers, images, atom_ptr, pixels = (t if t.is_contiguous() else t.contiguous()
                                              for t in (pointers, images, atom_ptr, pixels))
        if pixels.data_ptr() % 4:
            pixels = pixels.clone()                       # an int16 view that starts on an odd element
        feat = None
        if f > 0 and features is not None:
            feat = features if features.dim() == 2 else features.reshape(v, f)
            feat = feat if feat.is_contiguous() else feat.contiguous()
        held = (pointers, images, atom_ptr, pixels, feat)
        keep.append(held)
        d = descriptors[b]
        d.pointers, d.images, d.atom_ptr, d.pixels = (h.data_ptr() if h.numel() else None for h in held[:4])
        d.features = feat.data_ptr() if feat is not None and feat.numel() else None
        d.n_points, d.n_views, d.n_atoms, d.point_base = n, v, p, bases[b]
    ws, nbytes = _lib.workspace("dva_mapping_collate_workspace_bytes", dev, len(rows))
    out_ptr, out_img, out_aptr, out_pix, out_feat = _mapping_outputs(dev, n_out, v_out, p_out,
                                                                     None if trailing is None else f)
    offsets = torch.empty(len(rows), dtype=torch.int64, device=dev)
    moved = (n_out + 1) * 8 + sum(r[0] for r in rows) * 8 + v_out * (40 + 8 * f) + p_out * 8
    with _timed("mapping_collate", moved):
        check(lib.dva_mapping_collate(descriptors, len(rows), 2, f, n_out, v_out, p_out, ptr(out_ptr), ptr(out_img),
                                      ptr(out_aptr), ptr(out_pix), ptr(out_feat if f > 0 else None), ptr(offsets),
                                      ptr(ws), int(nbytes), stream_of(out_ptr)), "dva_mapping_collate")
    del keep                                              # the launches are queued: the stream orders the frees
    if out_feat is not None:
        out_feat = out_feat.view((v_out,) + trailing)
    return out_ptr, out_img, out_aptr, out_pix, out_feat, offsets


# ---------------------------------------------------------------------------------------------
# sparse 3D convolution on voxel tensors (modules/SparseConv3d over torchsparse 1.1.0 Conv3d)
# ---------------------------------------------------------------------------------------------

def voxel_kernel_map(src_coords, dst_coords, offsets):
    """``nbr[k, j] = i`` with ``src_coords[i] == dst_coords[j] + offsets[k]`` (spatial columns; equal batch
    column), ``-1`` when absent.  int32 [K, n_dst]."""
    lib = _lib.load()
    require_device(src_coords, dst_coords)
    assert src_coords.dim() == 2 and src_coords.shape[1] == 4 and dst_coords.dim() == 2 and dst_coords.shape[1] == 4
    sc = src_coords.to(torch.int32).contiguous()
    dc = dst_coords.to(torch.int32).contiguous()
    off = torch.as_tensor(offsets, dtype=torch.int32).reshape(-1, 3).to(sc.device).contiguous()
    K, n_src, n_dst = off.shape[0], sc.shape[0], dc.shape[0]
    nbr = torch.empty((K, n_dst), dtype=torch.int32, device=sc.device)
    ws, nbytes = _lib.workspace("dva_voxel_parent_workspace_bytes", sc.device, n_src)
    with _timed("voxel_kernel_map", n_src * 24 + K * n_dst * 24):
        check(lib.dva_voxel_kernel_map(ptr(sc), n_src, ptr(dc), n_dst, ptr(off), K, ptr(nbr), ptr(ws), int(nbytes),
                                       stream_of(sc)), "dva_voxel_kernel_map")
    return nbr


# flags of dva_voxel_level's record (include/dva.h)
VOXEL_LEVEL_FLAG_STRIDE, VOXEL_LEVEL_FLAG_KEY, VOXEL_LEVEL_FLAG_BOUNDS = 1, 2, 4

VoxelLevel = collections.namedtuple("VoxelLevel", "out_coords parent nbr nbr_t direct")


def voxel_bounds(coords):
    """``((min x, y, z, batch), (max x, y, z, batch))`` of int32 [n, 4] coordinates as Python ints, None for n = 0:
    one launch pair and one host read.  Floored to a coarser stride on the host, these are the exact bounds of every
    coarser level of the same pyramid (floor is monotone), which is how ``voxel_level`` takes them."""
    lib = _lib.load()
    require_device(coords)
    assert coords.dim() == 2 and coords.shape[1] == 4
    c = coords.to(torch.int32).contiguous()
    n = c.shape[0]
    if n == 0:
        return None
    out = torch.empty(8, dtype=torch.int64, device=c.device)
    ws, nbytes = _lib.workspace("dva_voxel_level_workspace_bytes", c.device, n)
    with _timed("voxel_bounds", n * 16):
        check(lib.dva_voxel_bounds(ptr(c), n, ptr(out), ptr(ws), int(nbytes), stream_of(c)), "dva_voxel_bounds")
    b = out.tolist()                                      # host read: the sort's bit count
    return tuple(b[:4]), tuple(b[4:])


def voxel_level(coords, ratio, in_stride, maps=True, bounds=None):
    """One strided level of a voxel pyramid from one sort: ``VoxelLevel(out_coords, parent, nbr, nbr_t, direct)``.

    ``coords`` int32 [n, 4] = (x, y, z, batch) at tensor stride ``in_stride``; ``ratio`` the output tensor stride.
    ``out_coords`` int32 [n_out, 4]: the unique rows of ``(floor(xyz / ratio) * ratio, batch)``, ascending (batch, z,
    y, x) -- ``snn.downsample_coords``; ``parent`` int64 [n]: ``voxel_parent_index(coords, out_coords, ratio)``.
    With ``maps`` and ``ratio == 2 * in_stride`` on coordinates that are multiples of ``in_stride``, ``direct`` is True
    and ``nbr`` int32 [8, n_out], ``nbr_t`` int32 [8, n] are the kernel map pair of a kernel_size 2 / stride 2 /
    dilation 1 convolution (``voxel_kernel_map(coords, out_coords, offs)`` and ``(out_coords, coords, -offs)``);
    otherwise both are None and the caller builds them with ``voxel_kernel_map``.

    ``bounds``: ``voxel_bounds`` of ``coords`` or of any finer tensor of the same pyramid (None: computed here, one more
    host read).  One host read of its own: ``n_out`` and the flags together.  Where the key (batch, z, y, x) does not fit
    ``downsample_coords``' 62 bits, or a row lies outside ``bounds``, every field is None (``direct`` False): the caller
    takes the composition."""
    lib = _lib.load()
    require_device(coords)
    assert coords.dim() == 2 and coords.shape[1] == 4
    ratio, in_stride = int(ratio), int(in_stride)
    if ratio <= 0 or in_stride <= 0:
        raise ValueError(f"ops.voxel_level: ratio and in_stride must be positive, got {ratio} and {in_stride}")
    c = coords.to(torch.int32).contiguous()
    n, dev = c.shape[0], c.device
    want_maps = bool(maps) and ratio == 2 * in_stride
    if n == 0:
        empty = (lambda: torch.empty((8, 0), dtype=torch.int32, device=dev)) if want_maps else (lambda: None)
        return VoxelLevel(torch.empty((0, 4), dtype=torch.int32, device=dev),
                          torch.empty(0, dtype=torch.int64, device=dev), empty(), empty(), want_maps)
    lo, hi = bounds if bounds is not None else voxel_bounds(c)
    floored = [v // ratio * ratio for v in lo[:3]] + [lo[3]] + [v // ratio * ratio for v in hi[:3]] + [hi[3]]
    out_coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
    parent = torch.empty(n, dtype=torch.int64, device=dev)
    record = torch.empty(2, dtype=torch.int64, device=dev)
    ws, nbytes = _lib.workspace("dva_voxel_level_workspace_bytes", dev, n)
    with _timed("voxel_level", n * 24):                   # compulsory: rows in, parents out (+ 16 n_out, not known yet)
        check(lib.dva_voxel_level(ptr(c), n, ratio, in_stride, (ctypes.c_int64 * 8)(*floored), ptr(out_coords),
                                  ptr(parent), ptr(record), ptr(ws), int(nbytes), stream_of(c)), "dva_voxel_level")
    n_out, flags = record.tolist()                        # host read: the output shapes and the flags, together
    if flags & (VOXEL_LEVEL_FLAG_KEY | VOXEL_LEVEL_FLAG_BOUNDS):
        return VoxelLevel(None, None, None, None, False)
    out_coords = out_coords[:n_out].clone()               # release the capacity
    if not want_maps or flags & VOXEL_LEVEL_FLAG_STRIDE:
        return VoxelLevel(out_coords, parent, None, None, False)
    nbr = torch.empty((8, n_out), dtype=torch.int32, device=dev)
    nbr_t = torch.empty((8, n), dtype=torch.int32, device=dev)
    with _timed("voxel_level_maps", n * 56 + n_out * 32):  # rows and parents in, both maps out
        check(lib.dva_voxel_level_maps(ptr(c), ptr(parent), n, n_out, ratio, in_stride, ptr(nbr), ptr(nbr_t),
                                       stream_of(c)), "dva_voxel_level_maps")
    return VoxelLevel(out_coords, parent, nbr, nbr_t, True)


SPARSE_CONV_TIMER_SHAPES = False  # bench tools: label the KernelTimer entries with the layer shape


def _pad16(c):
    return (c + 15) // 16 * 16


def _sparse_conv_apply(x, nbr, W, bias, n_dst, mode):
    """out[j] = bias + sum_k x[nbr[k, j]] @ (W[k] if mode == 0 else W[k].T); channel counts padded to 16."""
    lib = _lib.load()
    K = nbr.shape[0]
    cin, cout = (W.shape[1], W.shape[2]) if mode == 0 else (W.shape[2], W.shape[1])
    assert x.shape[1] == cin, f"features have {x.shape[1]} channels, the kernel expects {cin}"
    if x.shape[0] == 0 or n_dst == 0:
        out = torch.zeros((n_dst, cout), dtype=x.dtype, device=x.device)
        return out if bias is None else out + bias.to(x.dtype)
    cin_p, cout_p = _pad16(cin), _pad16(cout)
    Wf = W.detach().float()
    if cin_p != cin or cout_p != cout:
        pa, pb = (cin_p - cin, cout_p - cout) if mode == 0 else (cout_p - cout, cin_p - cin)
        Wf = torch.nn.functional.pad(Wf, (0, pb, 0, pa))
        x = torch.nn.functional.pad(x, (0, cin_p - cin))
        if bias is not None:
            bias = torch.nn.functional.pad(bias.detach().float(), (0, cout_p - cout))
    x, Wf = x.contiguous(), Wf.contiguous()
    bias = None if bias is None else bias.detach().float().contiguous()
    out = torch.empty((n_dst, cout_p), dtype=x.dtype, device=x.device)
    code = dtype_code(x)
    ws, nbytes = _lib.workspace("dva_sparse_conv_workspace_bytes", x.device, K, cin_p, cout_p, code)
    s = x.element_size()
    with _timed(f"sparse_conv_apply{SPARSE_CONV_TIMER_SHAPES and f'[{K}x{cin_p}->{cout_p}@{n_dst}]' or ''}",
                n_dst * (K * 4 + cout_p * s) + x.shape[0] * cin_p * s):
        check(lib.dva_sparse_conv_apply(ptr(x), ptr(nbr), ptr(Wf), ptr(bias), ptr(out), x.shape[0], n_dst, K, cin_p,
                                        cout_p, mode, code, ptr(ws), nbytes, stream_of(x)), "dva_sparse_conv_apply")
    return out if cout_p == cout else out[:, :cout].contiguous()


def _sparse_conv_wgrad(x, nbr, gout, cin, cout):
    lib = _lib.load()
    K, n_dst = nbr.shape
    cin_p, cout_p = _pad16(cin), _pad16(cout)
    if cin_p != cin:
        x = torch.nn.functional.pad(x, (0, cin_p - cin))
    if cout_p != cout:
        gout = torch.nn.functional.pad(gout, (0, cout_p - cout))
    x, gout = x.contiguous(), gout.contiguous()
    gW = torch.empty((K, cin_p, cout_p), dtype=torch.float32, device=x.device)
    s = x.element_size()
    with _timed(f"sparse_conv_wgrad{SPARSE_CONV_TIMER_SHAPES and f'[{K}x{cin_p}->{cout_p}@{n_dst}]' or ''}",
                n_dst * (K * 4 + cout_p * s) + x.shape[0] * cin_p * s):
        check(lib.dva_sparse_conv_wgrad(ptr(x), ptr(nbr), ptr(gout), ptr(gW), x.shape[0], n_dst, K, cin_p, cout_p,
                                        dtype_code(x), stream_of(x)), "dva_sparse_conv_wgrad")
    return gW if (cin_p == cin and cout_p == cout) else gW[:, :cin, :cout].contiguous()


class _SparseConv(torch.autograd.Function):
    """out = bias + sum_k x[nbr[k]] @ W[k].  ``nbr`` [K, n_dst] maps destination voxels to source rows, ``nbr_t``
    [K, n_src] is the transposed map (source voxel -> destination row under the same offset)."""

    @staticmethod
    def forward(ctx, x, W, bias, nbr, nbr_t):
        require_device(x, W, nbr, nbr_t)
        ctx.save_for_backward(x, W, nbr, nbr_t)
        ctx.has_bias = bias is not None
        return _sparse_conv_apply(x, nbr, W, bias, nbr.shape[1], 0)

    @staticmethod
    def backward(ctx, gout):
        x, W, nbr, nbr_t = ctx.saved_tensors
        gout = gout.contiguous().to(x.dtype)
        gx = gW = gb = None
        if ctx.needs_input_grad[0]:
            gx = _sparse_conv_apply(gout, nbr_t, W, None, x.shape[0], 1)
        if ctx.needs_input_grad[1]:
            gW = _sparse_conv_wgrad(x, nbr, gout, W.shape[1], W.shape[2]).to(W.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gout.float().sum(0)
        return gx, gW, gb, None, None


SPARSE_CONV_MAX_PARTS = 4          # SC_MAX_PARTS of csrc/sparseconv.hip


def _parts_widths(parts):
    return tuple(int(p.shape[1]) for p in parts)


def _parts_common(parts, what):
    """The parts of a features list, each brought on its own to the dtype the call on ``torch.cat(parts, 1)`` would
    run in: the autocast rule of ``sparse_conv``, else torch's promotion over the parts."""
    parts = list(parts)
    if not parts or not all(torch.is_tensor(p) and p.dim() == 2 for p in parts):
        raise ValueError(f"{what}: the features are a tensor [n, C] or a non-empty list of such tensors")
    if len(parts) > SPARSE_CONV_MAX_PARTS:
        raise ValueError(f"{what}: at most {SPARSE_CONV_MAX_PARTS} parts, got {len(parts)} (concatenate some of them)")
    n = parts[0].shape[0]
    if any(p.shape[0] != n for p in parts):
        raise ValueError(f"{what}: the parts have {[p.shape[0] for p in parts]} rows; they must sit on the same voxels")
    if any(p.shape[1] == 0 for p in parts):
        raise ValueError(f"{what}: a part without channels")
    require_device(*parts)
    dtype = sparse_conv_parts_dtype(parts)
    return [p.to(dtype) for p in parts]


def _parts_padded(parts):
    """Every part contiguous and at a multiple of 16 channels: a narrow part is padded alone, the others are not copied."""
    return [(p if p.shape[1] % 16 == 0 else torch.nn.functional.pad(p, (0, _pad16(p.shape[1]) - p.shape[1]))).contiguous()
            for p in parts]


def _parts_table(parts):
    """The host arrays of the ``*_parts`` entries: device pointers and widths."""
    P = len(parts)
    return ((ctypes.c_void_p * P)(*[p.data_ptr() for p in parts]),
            (ctypes.c_int32 * P)(*[p.shape[1] for p in parts]), P)


def _parts_weights(W, widths, cout_p):
    """W fp32 [K, sum widths, Cout] -> [K, sum pad16(widths), cout_p]: every part's zero rows in place."""
    Wf = W.detach().float()
    cout = Wf.shape[2]
    if cout_p == cout and all(w % 16 == 0 for w in widths):
        return Wf.contiguous()
    pieces, a = [], 0
    for w in widths:
        pieces.append(torch.nn.functional.pad(Wf[:, a:a + w], (0, cout_p - cout, 0, _pad16(w) - w)))
        a += w
    return torch.cat(pieces, 1).contiguous()


def _sparse_conv_apply_parts(parts, nbr, W, bias, n_dst):
    """``_sparse_conv_apply`` in mode 0 on the channel concatenation of ``parts`` (one dtype), which is not written."""
    lib = _lib.load()
    K, cout = nbr.shape[0], W.shape[2]
    widths = _parts_widths(parts)
    assert sum(widths) == W.shape[1], f"the parts have {sum(widths)} channels, the kernel expects {W.shape[1]}"
    x0 = parts[0]
    if x0.shape[0] == 0 or n_dst == 0:
        out = torch.zeros((n_dst, cout), dtype=x0.dtype, device=x0.device)
        return out if bias is None else out + bias.to(x0.dtype)
    cout_p = _pad16(cout)
    Wf = _parts_weights(W, widths, cout_p)
    cin_p = Wf.shape[1]
    bias = None if bias is None else bias.detach().float()
    if bias is not None and cout_p != cout:
        bias = torch.nn.functional.pad(bias, (0, cout_p - cout))
    bias = None if bias is None else bias.contiguous()
    parts = _parts_padded(parts)
    out = torch.empty((n_dst, cout_p), dtype=x0.dtype, device=x0.device)
    code = dtype_code(x0)
    ws, nbytes = _lib.workspace("dva_sparse_conv_workspace_bytes", x0.device, K, cin_p, cout_p, code)
    s = x0.element_size()
    ptrs, wid, P = _parts_table(parts)
    with _timed(f"sparse_conv_apply_parts{SPARSE_CONV_TIMER_SHAPES and f'[{K}x{cin_p}->{cout_p}@{n_dst}]' or ''}",
                n_dst * (K * 4 + cout_p * s) + x0.shape[0] * cin_p * s):
        check(lib.dva_sparse_conv_apply_parts(ptrs, wid, P, ptr(nbr), ptr(Wf), ptr(bias), ptr(out), x0.shape[0], n_dst,
                                              K, cout_p, code, ptr(ws), nbytes, stream_of(x0)),
              "dva_sparse_conv_apply_parts")
    return out if cout_p == cout else out[:, :cout].contiguous()


def _sparse_conv_wgrad_parts(parts, nbr, gout, cout):
    """``_sparse_conv_wgrad`` on the parts: fp32 [K, sum widths, Cout], the padding rows of a narrow part cut."""
    lib = _lib.load()
    K, n_dst = nbr.shape
    widths = _parts_widths(parts)
    cout_p = _pad16(cout)
    if cout_p != cout:
        gout = torch.nn.functional.pad(gout, (0, cout_p - cout))
    gout = gout.contiguous()
    parts = _parts_padded(parts)
    cin_p = sum(p.shape[1] for p in parts)
    x0 = parts[0]
    gW = torch.empty((K, cin_p, cout_p), dtype=torch.float32, device=x0.device)
    s = x0.element_size()
    ptrs, wid, P = _parts_table(parts)
    with _timed(f"sparse_conv_wgrad_parts{SPARSE_CONV_TIMER_SHAPES and f'[{K}x{cin_p}->{cout_p}@{n_dst}]' or ''}",
                n_dst * (K * 4 + cout_p * s) + x0.shape[0] * cin_p * s):
        check(lib.dva_sparse_conv_wgrad_parts(ptrs, wid, P, ptr(nbr), ptr(gout), ptr(gW), x0.shape[0], n_dst, K, cout_p,
                                              dtype_code(x0), stream_of(x0)), "dva_sparse_conv_wgrad_parts")
    if cin_p == sum(widths) and cout_p == cout:
        return gW
    pieces, a = [], 0
    for w in widths:
        pieces.append(gW[:, a:a + w, :cout])
        a += _pad16(w)
    return torch.cat(pieces, 1)


class _SparseConvParts(torch.autograd.Function):
    """``_SparseConv`` on features given in parts (one dtype): the concatenation is never written in the forward pass
    or for the weight gradient; the input gradient is one [n_src, sum C_p] buffer and each part gets its columns."""

    @staticmethod
    def forward(ctx, W, bias, nbr, nbr_t, *parts):
        require_device(W, nbr, nbr_t, *parts)
        ctx.save_for_backward(W, nbr, nbr_t, *parts)
        ctx.has_bias = bias is not None
        return _sparse_conv_apply_parts(parts, nbr, W, bias, nbr.shape[1])

    @staticmethod
    def backward(ctx, gout):
        W, nbr, nbr_t, *parts = ctx.saved_tensors
        gout = gout.contiguous().to(parts[0].dtype)
        gW = gb = None
        gparts = [None] * len(parts)
        if any(ctx.needs_input_grad[4:]):
            gx = _sparse_conv_apply(gout, nbr_t, W, None, parts[0].shape[0], 1)
            a = 0
            for i, p in enumerate(parts):
                if ctx.needs_input_grad[4 + i]:
                    gparts[i] = gx[:, a:a + p.shape[1]]
                a += p.shape[1]
        if ctx.needs_input_grad[0]:
            gW = _sparse_conv_wgrad_parts(parts, nbr, gout, W.shape[2]).to(W.dtype)
        if ctx.has_bias and ctx.needs_input_grad[1]:
            gb = gout.float().sum(0)
        return (gW, gb, None, None, *gparts)


def sparse_conv(x, W, bias, nbr, nbr_t):
    """Sparse convolution over a kernel map pair (see ``voxel_kernel_map``): x [n_src, Cin] (fp32 or bf16),
    W fp32 [K, Cin, Cout], bias [Cout] or None -> [n_dst, Cout].  Under ``torch.autocast`` the features are
    taken in the autocast dtype (the weights stay fp32 masters, rounded to bf16 inside the kernel); the kernels have no fp16
    form, so under autocast(float16) the 3D branch stays fp32 (the fusion concat already promotes to it).

    ``x`` may be a tuple or list of up to 4 tensors on the same voxels: the result is that of the call on
    ``torch.cat(x, 1)`` (bit for bit when every width is a multiple of 16), without that tensor being written.  Parts
    may differ in dtype; each is cast on its own (a bf16 part under autocast(bfloat16) is used as it is)."""
    if isinstance(x, (tuple, list)):
        parts = _parts_common(x, "ops.sparse_conv")
        if len(parts) == 1:
            return _SparseConv.apply(parts[0], W, bias, nbr, nbr_t)
        return _SparseConvParts.apply(W, bias, nbr, nbr_t, *parts)
    if torch.is_autocast_enabled() and x.is_cuda:
        x = x.to(torch.bfloat16 if torch.get_autocast_dtype('cuda') == torch.bfloat16 else torch.float32)
    return _SparseConv.apply(x, W, bias, nbr, nbr_t)


def sparse_conv_feature_dtype(x):
    """The dtype ``sparse_conv`` and ``sparse_conv_fused`` take the features ``x`` in: the autocast rule above."""
    if torch.is_autocast_enabled() and x.is_cuda:
        return torch.bfloat16 if torch.get_autocast_dtype('cuda') == torch.bfloat16 else torch.float32
    return x.dtype


def sparse_conv_parts_dtype(parts):
    """``sparse_conv_feature_dtype`` for features given in parts: the dtype the call on their concatenation runs in."""
    if torch.is_autocast_enabled() and parts[0].is_cuda:
        return torch.bfloat16 if torch.get_autocast_dtype('cuda') == torch.bfloat16 else torch.float32
    dtype = parts[0].dtype
    for p in parts[1:]:
        dtype = torch.promote_types(dtype, p.dtype)
    return dtype


class PackedSparseConvWeights:
    """The constant weights of one sparse convolution as ``sconv_apply_kernel`` reads them (bf16 ``w_hi | w_lo``
    tiles): ``buf`` uint8, with ``K``, ``cin``, ``cout``, the widths padded to 16 ``cin_p`` / ``cout_p`` and the
    feature ``dtype`` the layout was made for.  ``parts``: the widths of the feature parts the input-channel axis was
    packed for (each padded to 16 in place, ``cin_p`` their sum), or None for one tensor."""
    __slots__ = ("buf", "K", "cin", "cout", "cin_p", "cout_p", "dtype", "parts")

    def __init__(self, buf, K, cin, cout, cin_p, cout_p, dtype, parts=None):
        self.buf, self.K, self.cin, self.cout, self.cin_p, self.cout_p, self.dtype = buf, K, cin, cout, cin_p, cout_p, dtype
        self.parts = parts


def sparse_conv_pack(W, dtype, parts=None):
    """Pack W fp32 [K, Cin, Cout] once for ``sparse_conv_fused`` on features of ``dtype`` (fp32 or bf16).  ``parts``:
    the widths of the tensors the features will be given in (they sum to Cin); the input-channel axis is then packed
    with each part's padding to 16 in place."""
    lib = _lib.load()
    require_device(W)
    if W.dim() != 3:
        raise ValueError(f"ops.sparse_conv_pack: W must be [K, Cin, Cout], got {tuple(W.shape)}")
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"ops.sparse_conv_pack: the kernels take fp32 or bf16 features, not {dtype}")
    K, cin, cout = W.shape
    if parts is not None:
        parts = tuple(int(w) for w in parts)
        if not 1 <= len(parts) <= SPARSE_CONV_MAX_PARTS or any(w <= 0 for w in parts) or sum(parts) != cin:
            raise ValueError(f"ops.sparse_conv_pack: parts {parts} are not 1 to {SPARSE_CONV_MAX_PARTS} positive widths "
                             f"that sum to Cin = {cin}")
        if len(parts) == 1:
            parts = None
    cout_p = _pad16(cout)
    if parts is None:
        cin_p = _pad16(cin)
        Wf = W.detach().float()
        if cin_p != cin or cout_p != cout:
            Wf = torch.nn.functional.pad(Wf, (0, cout_p - cout, 0, cin_p - cin))
        Wf = Wf.contiguous()
    else:
        Wf = _parts_weights(W, parts, cout_p)
        cin_p = Wf.shape[1]
    code = _lib.DVA_F32 if dtype == torch.float32 else _lib.DVA_BF16
    buf, nbytes = _lib.workspace("dva_sparse_conv_workspace_bytes", W.device, K, cin_p, cout_p, code)
    with _timed("sparse_conv_pack", K * cin_p * cout_p * 4 + nbytes):
        check(lib.dva_sparse_conv_pack_weights(ptr(Wf), K, cin_p, cout_p, 0, code, ptr(buf), nbytes, stream_of(Wf)),
              "dva_sparse_conv_pack_weights")
    return PackedSparseConvWeights(buf, K, cin, cout, cin_p, cout_p, dtype, parts)


def sparse_conv_fused(x, packed, bias, nbr, residual=None, slope=1.0):
    """Inference form of ``sparse_conv`` over packed constant weights (``sparse_conv_pack``), with the activation and
    the residual sum in the kernel's epilogue: ``out = T(leaky(conv(x) + bias, slope) + residual)``, fp32 steps, one
    rounding.  x [n_src, Cin], bias fp32 [Cout] or None, nbr int32 [K, n_dst], residual [n_dst, Cout] or None ->
    [n_dst, Cout].  No autograd.  The autocast rule of ``sparse_conv`` holds; ``packed`` must be of that dtype.

    ``x`` may be a tuple or list of tensors as in ``sparse_conv``; ``packed`` must then have been made with their
    widths (``sparse_conv_pack(W, dtype, parts=widths)``), else ValueError."""
    lib = _lib.load()
    parts = None
    if isinstance(x, (tuple, list)):
        parts = [p.detach() for p in _parts_common(x, "ops.sparse_conv_fused")]
        if torch.is_grad_enabled() and any(p.requires_grad for p in x):
            raise RuntimeError("ops.sparse_conv_fused has no backward: call it under torch.no_grad() or on detached "
                               "inputs (ops.sparse_conv is the differentiable form)")
        if len(parts) == 1:
            x, parts = parts[0], None
        else:
            x = parts[0]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, bias, residual)):
        raise RuntimeError("ops.sparse_conv_fused has no backward: call it under torch.no_grad() or on detached "
                           "inputs (ops.sparse_conv is the differentiable form)")
    require_device(x, packed.buf, nbr, bias, residual)
    assert nbr.dtype == torch.int32 and nbr.dim() == 2, "nbr is the int32 [K, n_dst] map of voxel_kernel_map"
    nbr = nbr.contiguous()
    if parts is None:
        x = x.detach().to(sparse_conv_feature_dtype(x))
    if x.dtype != packed.dtype:
        raise TypeError(f"ops.sparse_conv_fused: weights packed for {packed.dtype} features, got {x.dtype}")
    K, n_dst = nbr.shape
    assert K == packed.K, f"the kernel map has {K} offsets, the packed weights {packed.K}"
    if parts is not None:
        if packed.parts != _parts_widths(parts):
            raise ValueError(f"ops.sparse_conv_fused: the features come in parts of widths {_parts_widths(parts)}, the "
                             f"weights were packed for {packed.parts or (packed.cin,)} "
                             "(ops.sparse_conv_pack(W, dtype, parts=widths))")
    else:
        assert x.shape[1] == packed.cin, f"features have {x.shape[1]} channels, the kernel expects {packed.cin}"
        if packed.parts is not None and any(w % 16 for w in packed.parts):
            raise ValueError(f"ops.sparse_conv_fused: the weights were packed for parts of widths {packed.parts}, the "
                             "features are one tensor")
    slope = float(slope)
    cout, cin_p, cout_p = packed.cout, packed.cin_p, packed.cout_p
    if residual is not None:
        assert residual.shape == (n_dst, cout), f"residual {tuple(residual.shape)} for an output {(n_dst, cout)}"
        residual = residual.detach().to(x.dtype)
    bias = None if bias is None else bias.detach().float()
    if x.shape[0] == 0 or n_dst == 0:
        v = torch.zeros((n_dst, cout), dtype=torch.float32, device=x.device)
        if bias is not None:
            v = v + bias
        v = torch.where(v >= 0, v, slope * v)
        return (v if residual is None else v + residual.float()).to(x.dtype)
    if parts is not None:
        parts = _parts_padded(parts)
    elif cin_p != packed.cin:
        x = torch.nn.functional.pad(x, (0, cin_p - packed.cin))
    if cout_p != cout:
        bias = None if bias is None else torch.nn.functional.pad(bias, (0, cout_p - cout))
        residual = None if residual is None else torch.nn.functional.pad(residual, (0, cout_p - cout))
    x = x.contiguous()
    bias = None if bias is None else bias.contiguous()
    residual = None if residual is None else residual.contiguous()
    out = torch.empty((n_dst, cout_p), dtype=x.dtype, device=x.device)
    s = x.element_size()
    tag = "sparse_conv_fused" if parts is None else "sparse_conv_fused_parts"
    with _timed(f"{tag}{SPARSE_CONV_TIMER_SHAPES and f'[{K}x{cin_p}->{cout_p}@{n_dst}]' or ''}",
                n_dst * (K * 4 + cout_p * s * (1 if residual is None else 2)) + x.shape[0] * cin_p * s):
        if parts is None:
            check(lib.dva_sparse_conv_apply_packed(ptr(x), ptr(nbr), ptr(packed.buf), packed.buf.numel(), ptr(bias),
                                                   ptr(residual), slope, ptr(out), x.shape[0], n_dst, K, cin_p, cout_p,
                                                   dtype_code(x), stream_of(x)), "dva_sparse_conv_apply_packed")
        else:
            ptrs, wid, P = _parts_table(parts)
            check(lib.dva_sparse_conv_apply_packed_parts(ptrs, wid, P, ptr(nbr), ptr(packed.buf), packed.buf.numel(),
                                                         ptr(bias), ptr(residual), slope, ptr(out), x.shape[0], n_dst,
                                                         K, cout_p, dtype_code(x), stream_of(x)),
                  "dva_sparse_conv_apply_packed_parts")
    return out if cout_p == cout else out[:, :cout].contiguous()


# ---------------------------------------------------------------------------------------------
# neighbourhood-based mapping features (data_transform/multimodal/image.py:431-612)
# ---------------------------------------------------------------------------------------------

def _knn_default_cell(lo, hi, ext, n, k):
    """Grid cell of the K-NN for n search points in the box [lo, hi] of largest extent ext."""
    # a cell that holds a few points of a surface-like cloud: mean spacing x (k/4)^(1/3)
    dims = (hi - lo) > 1e-6 * max(ext, 1e-30)
    nd = int(dims.sum())
    if nd in (1, 2):
        # a PLANAR (or collinear) cloud -- BiasuttiVisibility searches image-plane points (x, y, 0): the volume rule
        # would give a cell far below the point spacing (z extent clamped to 1e-6) and every query would be retried
        # on coarser grids (4 - 6 full launches): mean spacing in the occupied dimensions x (k/4)^(1/nd)
        area = float((hi - lo)[dims].prod())
        return (area / n) ** (1 / nd) * max(1.0, (k / 4) ** (1 / nd))
    vol = float((hi - lo).clamp(min=1e-6).prod())
    return (vol / n) ** (1 / 3) * max(1.0, (k / 4) ** (1 / 3))


def knn(xyz, k, cell=None):
    """Exact k nearest neighbours of every point among all points (itself first): ``(neighbors int32 [n, k],
    dist2 fp32 [n, k])``, ascending by (squared fp32 distance, index)."""
    lib = _lib.load()
    require_device(xyz)
    xyz = xyz.float().contiguous()
    n = xyz.shape[0]
    assert xyz.dim() == 2 and xyz.shape[1] == 3
    if not 0 < k <= 128:
        raise ValueError(f"ops.knn: k = {k} neighbours requested, the kernel keeps at most 128 candidates per query "
                         f"(csrc/knn.hip); the reference's settings are k <= 75")
    nbr = torch.empty((n, k), dtype=torch.int32, device=xyz.device)
    d2 = torch.empty((n, k), dtype=torch.float32, device=xyz.device)
    if n == 0:
        return nbr, d2
    lo, hi = xyz.min(0).values, xyz.max(0).values
    bbox = torch.cat([lo, hi]).contiguous()
    ext = float((hi - lo).max())                   # host sync: this is a preprocessing transform
    if cell is None:
        cell = _knn_default_cell(lo, hi, ext, n, k)
    cell = max(float(cell), ext / (1 << 19), 1e-12)
    ws, nbytes = _lib.workspace("dva_knn_workspace_bytes", xyz.device, n)
    done = torch.zeros(n, dtype=torch.uint8, device=xyz.device)
    # levels: a query that is not provably complete within 2 shells of cells (sparse region, outlier) is
    # retried on a 4x coarser grid; the last level covers the whole cloud
    shells = 2
    with _timed("knn", n * (12 + k * 8)):
        while True:
            last = cell * shells >= ext + cell
            check(lib.dva_knn(ptr(xyz), n, ptr(bbox), float(cell), int(k), (1 << 30) if last else shells, ptr(done),
                              ptr(nbr), ptr(d2), ptr(ws), int(nbytes), stream_of(xyz)), "dva_knn")
            if last:
                break
            cell *= 4.0
    return nbr, d2


def knn_query(query, search, k, cell=None):
    """Exact k nearest neighbours in ``search`` [m, 3] of every point of ``query`` [n, 3]: ``(neighbors int32 [n, k]
    indexing ``search``, dist2 fp32 [n, k])``, ascending by (squared fp32 distance, search index).  The reference's
    KeOps ``argKmin`` of PCAComputePointwise (core/data_transform/features.py:423-436).  With ``query`` the same
    cloud as ``search`` this equals ``knn``.  ``cell`` defaults to the rule of ``knn`` on the search cloud's density;
    queries may lie outside the search cloud's box."""
    lib = _lib.load()
    require_device(query, search)
    query = query.float().contiguous()
    search = search.float().contiguous()
    assert query.dim() == 2 and query.shape[1] == 3 and search.dim() == 2 and search.shape[1] == 3
    n, m = query.shape[0], search.shape[0]
    if not 0 < k <= 128:
        raise ValueError(f"ops.knn_query: k = {k} neighbours requested, the kernel keeps at most 128 candidates per "
                         f"query (csrc/knn.hip)")
    if m < k:
        raise ValueError(f"ops.knn_query: k = {k} neighbours requested from a search cloud of {m} points")
    nbr = torch.empty((n, k), dtype=torch.int32, device=query.device)
    d2 = torch.empty((n, k), dtype=torch.float32, device=query.device)
    if n == 0:
        return nbr, d2
    s_lo, s_hi = search.min(0).values, search.max(0).values
    lo, hi = torch.minimum(s_lo, query.min(0).values), torch.maximum(s_hi, query.max(0).values)
    bbox = torch.cat([lo, hi]).contiguous()        # the grid's origin and extent cover both clouds
    ext = float((hi - lo).max())                   # host sync: this is a preprocessing transform
    if cell is None:
        cell = _knn_default_cell(s_lo, s_hi, float((s_hi - s_lo).max()), m, k)
    cell = max(float(cell), ext / (1 << 19), 1e-12)
    ws, nbytes = _lib.workspace("dva_knn_query_workspace_bytes", query.device, n, m)
    done = torch.zeros(n, dtype=torch.uint8, device=query.device)
    # the level loop of knn: queries not provably complete within 2 shells are retried on a 4x coarser grid
    shells = 2
    with _timed("knn_query", n * (12 + k * 8) + m * 12):
        while True:
            last = cell * shells >= ext + cell
            check(lib.dva_knn_query(ptr(query), n, ptr(search), m, ptr(bbox), float(cell), int(k),
                                    (1 << 30) if last else shells, ptr(done), ptr(nbr), ptr(d2), ptr(ws), int(nbytes),
                                    stream_of(query)), "dva_knn_query")
            if last:
                break
            cell *= 4.0
    return nbr, d2


def pointwise_pca(search, neighbors):
    """PCA of the neighbourhood of every query point (the reference's ``batch_pca`` over ``search[neighbors]``,
    core/data_transform/features.py:307-329): ``(eigenvalues fp32 [n, 3] ascending, eigenvectors fp32 [n, 9])``, the
    eigenvectors as rows [v0 | v1 | v2] so that ``[:, :3]`` is the normal.  ``neighbors`` int [n, k] indexes ``search``
    [m, 3].  A neighbourhood with NaN coordinates gets eigenvalues 1 and the identity; the sign of every eigenvector
    makes its largest-magnitude component positive (include/dva.h)."""
    lib = _lib.load()
    require_device(search, neighbors)
    search = search.float().contiguous()
    assert search.dim() == 2 and search.shape[1] == 3 and neighbors.dim() == 2
    n, k = neighbors.shape
    m = search.shape[0]
    if not 0 < k <= 128:
        raise ValueError(f"ops.pointwise_pca: neighbourhoods of k = {k} points, the kernel takes 1 <= k <= 128")
    if m < k:
        raise ValueError(f"ops.pointwise_pca: neighbourhoods of k = {k} points in a cloud of {m} points")
    evals = torch.empty((n, 3), dtype=torch.float32, device=search.device)
    evecs = torch.empty((n, 9), dtype=torch.float32, device=search.device)
    if n == 0:
        return evals, evecs
    if int(neighbors.min()) < 0 or int(neighbors.max()) >= m:      # host sync: a preprocessing transform
        raise ValueError(f"ops.pointwise_pca: neighbour indices outside [0, {m})")
    nbr = neighbors.to(torch.int32).contiguous()
    with _timed("pointwise_pca", n * (k * 16 + 48)):
        check(lib.dva_pointwise_pca(ptr(search), m, ptr(nbr), n, int(k), ptr(evals), ptr(evecs), stream_of(search)),
              "dva_pointwise_pca")
    return evals, evecs


# ---------------------------------------------------------------------------------------------
# voxel-grid subsampling (core/data_transform/grid_transform.py:24-191, GridSampling3D)
# ---------------------------------------------------------------------------------------------

class GridClusters:
    """Result of ``grid_cluster``: ``coords`` int32 [M, 3] (the voxels' integer coordinates), ``cluster`` int64 [N]
    (voxel of every point), ``rep`` int64 [M] (representative point of every voxel), ``order`` int64 [N] (the points
    sorted by voxel, ascending point index within a voxel) and ``offsets`` int64 [M + 1] (voxel v holds
    ``order[offsets[v]:offsets[v + 1]]``).  Voxels are numbered in ascending (batch, z, y, x)."""

    def __init__(self, coords, cluster, rep, order, offsets):
        self.coords, self.cluster, self.rep, self.order, self.offsets = coords, cluster, rep, order, offsets

    @property
    def num_points(self):
        return self.cluster.shape[0]

    @property
    def num_voxels(self):
        return self.rep.shape[0]

    def __repr__(self):
        return f"GridClusters(num_points={self.num_points}, num_voxels={self.num_voxels})"


def grid_cluster(pos, size, batch=None, rank=None):
    """Voxel clustering of ``pos`` [N, 3] (fp32 or fp64) on a grid of ``size``: the reference's
    ``coords = round(pos / size)`` (division correctly rounded in the dtype of ``pos``, ties to even), torch_cluster's
    ``grid_cluster`` / torch_geometric's ``voxel_grid`` (with ``batch`` int [N] as the slowest coordinate) and
    ``consecutive_cluster``.  The representative of a voxel is its member of largest ``rank`` (int [N], values in
    [0, 2^31); the point's position in the reference's shuffle) or, without ``rank``, of largest index.  Returns
    ``GridClusters``.  Raises ValueError for N = 0, non-finite positions, ``|pos / size| >= 2^24`` or a key of more
    than 63 bits.  Two host reads: the coordinate ranges (the sort's bit count) and the voxel count."""
    lib = _lib.load()
    require_device(pos, batch, rank)
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"ops.grid_cluster: pos must be [N, 3], got {tuple(pos.shape)}")
    if pos.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"ops.grid_cluster: pos must be float32 or float64, got {pos.dtype}")
    size = float(size)
    if not size > 0 or size == float("inf"):
        raise ValueError(f"ops.grid_cluster: the grid size must be a positive finite number, got {size}")
    n = pos.shape[0]
    if n == 0:
        raise ValueError("ops.grid_cluster: an empty point cloud (N = 0) has no voxels")
    if n >= 1 << 31:
        raise ValueError(f"ops.grid_cluster: N = {n} points, the kernels take N < 2^31")
    dev = pos.device
    pos = pos.contiguous()
    if batch is not None:
        batch = batch.to(torch.int64).reshape(-1).contiguous()
        if batch.shape[0] != n:
            raise ValueError(f"ops.grid_cluster: batch has {batch.shape[0]} entries for {n} points")
    if rank is not None:
        rank = rank.to(torch.int64).reshape(-1).contiguous()
        if rank.shape[0] != n:
            raise ValueError(f"ops.grid_cluster: rank has {rank.shape[0]} entries for {n} points")
    ws, nbytes = _lib.workspace("dva_grid_workspace_bytes", dev, n, 0)
    coords = torch.empty((n, 3), dtype=torch.int32, device=dev)
    stats = torch.empty(9, dtype=torch.int64, device=dev)
    s = stream_of(pos)
    code = _lib.DVA_GRID_F32 if pos.dtype == torch.float32 else _lib.DVA_GRID_F64
    with _timed("grid_quantize", n * (3 * pos.element_size() + 12)):
        check(lib.dva_grid_quantize(ptr(pos), code, n, size, ptr(batch), ptr(coords), ptr(stats), ptr(ws), nbytes, s),
              "dva_grid_quantize")
    st = stats.tolist()                                   # host read: the sort's bit count
    if st[8] & 1:
        raise ValueError("GridSampling3D: pos holds non-finite coordinates (NaN or inf)")
    if st[8] & 2:
        raise ValueError(f"GridSampling3D: |pos / size| >= 2^24 at size = {size}: the reference's float grid "
                         f"arithmetic is inexact there; use a larger voxel size or centre the cloud")
    if rank is not None and n > 0:
        lo, hi = torch.aminmax(rank)
        if int(lo) < 0 or int(hi) >= 1 << 31:
            raise ValueError("ops.grid_cluster: rank values must lie in [0, 2^31)")
    span = 1
    for d in range(4):
        span *= st[4 + d] - st[d] + 1
    end_bit = max((span - 1).bit_length(), 1)
    if end_bit > 63:
        raise ValueError(f"GridSampling3D: the voxel key (batch, z, y, x) spans {span} values, more than 2^63; "
                         f"use a larger voxel size")
    order = torch.empty(n, dtype=torch.int64, device=dev)
    cluster = torch.empty(n, dtype=torch.int64, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    rep = torch.empty(n, dtype=torch.int64, device=dev)
    vcoords = torch.empty((n, 3), dtype=torch.int32, device=dev)
    n_voxels = torch.empty(1, dtype=torch.int64, device=dev)
    with _timed("grid_cluster", n * 80):
        check(lib.dva_grid_cluster(ptr(coords), ptr(batch), ptr(rank), n, ptr(stats), end_bit, ptr(order),
                                   ptr(cluster), ptr(offsets), ptr(rep), ptr(vcoords), ptr(n_voxels), ptr(ws), nbytes,
                                   s), "dva_grid_cluster")
    m = int(n_voxels)                                     # host read: the output shapes
    return GridClusters(vcoords[:m], cluster, rep[:m], order, offsets[:m + 1])


_GRID_DTYPES = {torch.float32: _lib.DVA_GRID_F32, torch.float64: _lib.DVA_GRID_F64, torch.int32: _lib.DVA_GRID_I32,
                torch.int64: _lib.DVA_GRID_I64}


def grid_mean(src, clusters):
    """Per-voxel mean of ``src`` [N, ...] over ``clusters`` (``grid_cluster``): torch_scatter's CPU ``scatter_mean``
    bit for bit -- the sum of the voxel's rows in the dtype of ``src``, accumulated sequentially in ascending point
    index, divided by the count in that dtype.  float32, float64, int32 and int64 in the kernel; for integers the sum
    wraps and the quotient is rounded toward zero (floor and truncation differ only for negative means).  Other
    integer dtypes are averaged in int64 and cast back (no wrap-around of the narrow type); bool is the integer mean
    floored, i.e. True when every member is True."""
    lib = _lib.load()
    require_device(src, clusters.order)
    n, m = clusters.num_points, clusters.num_voxels
    if src.shape[0] != n:
        raise ValueError(f"ops.grid_mean: src has {src.shape[0]} rows for {n} points")
    if src.dtype == torch.bool:
        return grid_mean(src.to(torch.int32), clusters).bool()
    if src.dtype not in _GRID_DTYPES:
        if src.is_floating_point() or src.is_complex():
            raise TypeError(f"ops.grid_mean: {src.dtype} rows are not supported (float32, float64, integers, bool)")
        return grid_mean(src.to(torch.int64), clusters).to(src.dtype)
    shape = tuple(src.shape[1:])
    C = 1
    for d in shape:
        C *= d
    out = torch.empty((m,) + shape, dtype=src.dtype, device=src.device)
    if C == 0:
        return out
    x = src.contiguous()
    ws, nbytes = _lib.workspace("dva_grid_workspace_bytes", src.device, n, C * x.element_size())
    with _timed("grid_mean", 2 * n * C * x.element_size() + n * 8 + m * C * x.element_size()):
        check(lib.dva_grid_mean(ptr(x), _GRID_DTYPES[src.dtype], n, C, ptr(clusters.order), ptr(clusters.offsets), m,
                                ptr(out), ptr(ws), nbytes, stream_of(x)), "dva_grid_mean")
    return out


def grid_majority(labels, clusters):
    """Per-voxel majority label, int64 [M]: the reference's ``one_hot(labels - labels.min())`` + ``scatter_add`` +
    ``argmax`` (ties to the smallest label; -1 ignore labels count like any other value)."""
    lib = _lib.load()
    require_device(labels, clusters.cluster)
    n, m = clusters.num_points, clusters.num_voxels
    if labels.dim() != 1 or labels.shape[0] != n:
        raise ValueError(f"ops.grid_majority: labels must be [N = {n}], got {tuple(labels.shape)}")
    if labels.is_floating_point() or labels.is_complex():
        raise TypeError(f"ops.grid_majority: labels must be integers, got {labels.dtype}")
    lab = labels.to(torch.int64).contiguous()
    lo, hi = torch.aminmax(lab)
    lo, hi = int(lo), int(hi)                             # host read: the label range sizes the sort
    n_labels = hi - lo + 1
    if n_labels > 1 << 32:
        raise ValueError(f"ops.grid_majority: labels span {n_labels} values, at most 2^32 are supported")
    end_bit = max((m * n_labels - 1).bit_length(), 1)
    if end_bit > 63:
        raise ValueError(f"ops.grid_majority: {m} voxels x {n_labels} labels do not fit a 63-bit key")
    out = torch.empty(m, dtype=torch.int64, device=lab.device)
    ws, nbytes = _lib.workspace("dva_grid_workspace_bytes", lab.device, n, 0)
    with _timed("grid_majority", n * 56):
        check(lib.dva_grid_majority(ptr(lab), n, ptr(clusters.cluster), m, lo, n_labels, end_bit, ptr(out), ptr(ws),
                                    nbytes, stream_of(lab)), "dva_grid_majority")
    return out


def view_occlusion(csr_idx, images, neighbors, k_list, n_images):
    """fp32 [V, len(k_list)]: ratio of the k nearest neighbours (and the point itself) seen by the view's image."""
    lib = _lib.load()
    require_device(csr_idx, images, neighbors)
    V, N, k = images.shape[0], csr_idx.shape[0] - 1, neighbors.shape[1]
    kl = torch.tensor(sorted(int(x) for x in k_list), dtype=torch.int32, device=images.device)
    assert int(kl[-1]) <= k
    out = torch.empty((V, kl.shape[0]), dtype=torch.float32, device=images.device)
    if V == 0:
        return out
    vp = csr_expand(csr_idx, V)
    bits = torch.empty(N * ((n_images + 63) // 64), dtype=torch.int64, device=images.device)
    check(lib.dva_view_occlusion(ptr(vp), ptr(images.contiguous()), V, N, int(n_images), ptr(neighbors.contiguous()),
                                 k, ptr(kl), kl.shape[0], ptr(bits), ptr(out), stream_of(images)),
          "dva_view_occlusion")
    return out


# ---------------------------------------------------------------------------------------------
# exact radius query (core/data_transform/transforms.py:99-232, :301-405: KDTree.query_radius)
# ---------------------------------------------------------------------------------------------

_RADIUS_TABLE_BYTES = 256 << 20      # budget of the per-(tile, centre) count table of one launch


def _radius_centres(centres, dims):
    """Centres as a float64 CPU tensor [B, dims]: a numpy array or a tensor of any float dtype, [dims] or [B, dims]."""
    c = centres if torch.is_tensor(centres) else torch.as_tensor(np.asarray(centres))
    if c.is_complex() or c.dtype == torch.bool:
        raise TypeError(f"ops.radius_query: centres must be real numbers, got {c.dtype}")
    c = c.detach().to(torch.float64)
    if c.dim() == 1:
        c = c.unsqueeze(0) if c.shape[0] else c.reshape(0, dims)
    if c.dim() != 2 or c.shape[1] != dims:
        raise ValueError(f"ops.radius_query: centres must be [B, {dims}] for dims = {dims}, got {tuple(c.shape)}")
    return c.contiguous()


def radius_query(pos, centres, radius, dims=3):
    """All points of ``pos`` fp32 [n, 3] within ``radius`` of every centre: ``(ptr int64 [B + 1], idx int64
    [ptr[B]])`` on the current HIP device (``pos`` is moved there when it lives elsewhere); the members of centre b are
    ``idx[ptr[b]:ptr[b + 1]]`` in ascending point index.  ``dims = 3`` is the sphere, ``dims = 2`` the cylinder along z (centres [B, 2]).  ``centres`` is a numpy
    array or a tensor of any float dtype and is converted to float64, as scikit-learn's tree does; ``radius`` is one
    number or one per centre.  The membership test is scikit-learn's leaf test, exactly: ``d <= r * r`` with
    ``d = ((dx dx) + dy dy) + dz dz`` in float64, ``dx = float64(p.x) - c.x``, each operation rounded on its own, the
    boundary included; a point with a non-finite coordinate is never a member.  Brute force over all pairs
    (csrc/ball.hip), no atomics: the same call gives the same bytes.  The centres are split so that the count table
    of one launch stays within ``_RADIUS_TABLE_BYTES``; one host read per split (the size of ``idx``)."""
    lib = _lib.load()
    if dims not in (2, 3):
        raise ValueError(f"ops.radius_query: dims must be 2 (cylinder) or 3 (sphere), got {dims}")
    if not torch.is_tensor(pos):
        raise TypeError("ops.radius_query: pos must be a tensor")
    if pos.dtype == torch.float64:
        raise TypeError("ops.radius_query: pos is float64; the reference's clouds are float32 and the membership "
                        "test is defined on float32 coordinates widened to float64: cast pos to float32")
    if pos.dtype != torch.float32:
        raise TypeError(f"ops.radius_query: pos must be float32, got {pos.dtype}")
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"ops.radius_query: pos must be [N, 3], got {tuple(pos.shape)}")
    n = pos.shape[0]
    if n >= 1 << 31:
        raise ValueError(f"ops.radius_query: N = {n} points, the kernels take N < 2^31")
    cen = _radius_centres(centres, dims)
    B = cen.shape[0]
    radii = None
    if torch.is_tensor(radius) or isinstance(radius, np.ndarray):
        r = torch.as_tensor(radius).detach().to(torch.float64).cpu().reshape(-1)
        if r.numel() == 1:
            radius = float(r)
        elif r.numel() != B:
            raise ValueError(f"ops.radius_query: {r.numel()} radii for {B} centres")
        else:
            radii = r
    if radii is None:
        radius = float(radius)
        if not radius >= 0:
            raise ValueError(f"ops.radius_query: the radius must be a non-negative number, got {radius}")
    elif B and not bool((radii >= 0).all()):
        raise ValueError("ops.radius_query: every radius must be a non-negative number")
    dev = torch.device("cuda", torch.cuda.current_device())
    pos = pos.detach().to(dev).contiguous()
    if B == 0 or n == 0:
        return torch.zeros(B + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    cen = cen.to(dev)
    if radii is not None:
        radii = radii.to(dev)
    tiles = (n + 511) // 512
    step = max(1, min(B, _RADIUS_TABLE_BYTES // (4 * tiles)))
    s = stream_of(pos)
    ptrs, idxs, total = [], [], 0
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        c = cen[b0:b0 + nb]
        rr = None if radii is None else radii[b0:b0 + nb]
        ws, nbytes = _lib.workspace("dva_radius_query_workspace_bytes", dev, n, nb)
        ptr_b = torch.empty(nb + 1, dtype=torch.int64, device=dev)
        rad = 0.0 if radii is not None else radius
        with _timed("radius_count", n * 12 + tiles * nb * 12):
            check(lib.dva_radius_count(ptr(pos), n, ptr(c), nb, int(dims), rad, ptr(rr), ptr(ptr_b), ptr(ws),
                                       int(nbytes), s), "dva_radius_count")
        m = int(ptr_b[nb])                                # host read: the size of idx
        idx_b = torch.empty(m, dtype=torch.int64, device=dev)
        with _timed("radius_fill", n * 12 + tiles * nb * 4 + m * 8):
            check(lib.dva_radius_fill(ptr(pos), n, ptr(c), nb, int(dims), rad, ptr(rr), ptr(ptr_b), ptr(idx_b), m,
                                      ptr(ws), int(nbytes), s), "dva_radius_fill")
        ptrs.append(ptr_b[:nb] + total)
        idxs.append(idx_b)
        total += m
    ptrs.append(torch.tensor([total], dtype=torch.int64, device=dev))
    return torch.cat(ptrs), (idxs[0] if len(idxs) == 1 else torch.cat(idxs))


# ---------------------------------------------------------------------------------------------
# elastic distortion (core/data_transform/grid_transform.py:194-256, ElasticDistortion)
# ---------------------------------------------------------------------------------------------

def _current_device():
    return torch.device("cuda", torch.cuda.current_device())


def _elastic_volume(volume, what):
    """A [Dx, Dy, Dz, 3] float32 volume (tensor or numpy array) as a contiguous tensor on the current HIP device."""
    v = volume if torch.is_tensor(volume) else torch.as_tensor(np.ascontiguousarray(volume))
    if v.dtype != torch.float32:
        raise TypeError(f"ops.{what} must be float32, got {v.dtype}")
    if v.dim() != 4 or v.shape[3] != 3 or min(v.shape[:3]) < 1:
        raise ValueError(f"ops.{what} must be [Dx, Dy, Dz, 3] with Dx, Dy, Dz >= 1, got {tuple(v.shape)}")
    if v.numel() >= 1 << 31:
        raise ValueError(f"ops.{what} has {v.numel()} elements, the kernels take fewer than 2^31")
    return v.detach().to(_current_device()).contiguous()


def _elastic_pos(pos, what):
    if not torch.is_tensor(pos):
        raise TypeError(f"ops.{what}: pos must be a tensor")
    if pos.dtype != torch.float32:
        raise TypeError(f"ops.{what}: pos must be float32 (the reference's clouds are), got {pos.dtype}")
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"ops.{what}: pos must be [N, 3], got {tuple(pos.shape)}")
    if pos.numel() >= 1 << 31:
        raise ValueError(f"ops.{what}: N = {pos.shape[0]} points, the kernels take 3 N < 2^31")
    return pos.detach().to(_current_device()).contiguous()


def elastic_smooth(noise):
    """The reference's smoothing of an ElasticDistortion noise volume ``noise`` float32 [Dx, Dy, Dz, 3] (tensor or
    numpy array): two rounds of ``scipy.ndimage.convolve`` with the 3-tap box kernels along axes 0, 1, 2
    (``mode="constant"``, ``cval=0``), bit for bit -- float64 accumulation over the taps in ascending order with
    ``w = float64(float32(1) / 3)``, every pass stored as float32.  Returns a new float32 tensor of the same shape on
    the current HIP device; ``noise`` is not modified.  Six launches of one kernel (csrc/elastic.hip)."""
    lib = _lib.load()
    vol = _elastic_volume(noise, "elastic_smooth: noise")
    dx, dy, dz = (int(d) for d in vol.shape[:3])
    ws, nbytes = _lib.workspace("dva_elastic_workspace_bytes", vol.device, dx, dy, dz)
    out = torch.empty_like(vol)
    with _timed("elastic_smooth", 6 * 2 * vol.numel() * 4):
        check(lib.dva_elastic_smooth(ptr(vol), dx, dy, dz, ptr(out), ptr(ws), int(nbytes), stream_of(vol)),
              "dva_elastic_smooth")
    return out


def elastic_displace(pos, field, axes, magnitude):
    """``pos + interp(pos) * magnitude`` of the reference's ElasticDistortion: ``pos`` float32 [N, 3], ``field``
    float32 [Dx, Dy, Dz, 3] (the smoothed noise), ``axes`` the three ascending float64 knot vectors of lengths Dx, Dy,
    Dz (at least 2 knots each; numpy arrays or tensors), ``magnitude`` a number.  ``interp`` is scipy's
    ``RegularGridInterpolator(axes, field, bounds_error=0, fill_value=0)`` bit for bit: trilinear in float64, the cell
    of a coordinate is the last knot not above it, 0 outside the axes; the sum is rounded to float32 once, at the end.
    Returns float32 [N, 3] on the current HIP device.  One thread per point (csrc/elastic.hip); non-finite ``pos`` is
    not supported."""
    lib = _lib.load()
    p = _elastic_pos(pos, "elastic_displace")
    f = _elastic_volume(field, "elastic_displace: field")
    if len(axes) != 3:
        raise ValueError(f"ops.elastic_displace: axes must be three knot vectors, got {len(axes)}")
    knots = []
    for d, a in zip(f.shape[:3], axes):
        a = (a.detach().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(torch.float64).reshape(-1)
        if a.shape[0] != d or d < 2:
            raise ValueError(f"ops.elastic_displace: an axis of {a.shape[0]} knots for a field of shape "
                             f"{tuple(f.shape)} (every axis needs its dimension's length, at least 2)")
        if not bool((a[1:] > a[:-1]).all()):
            raise ValueError("ops.elastic_displace: the knots of an axis must be strictly ascending")
        knots.append(a)
    ax = torch.cat(knots).to(p.device)
    n = p.shape[0]
    out = torch.empty_like(p)
    if n == 0:
        return out
    dx, dy, dz = (int(d) for d in f.shape[:3])
    with _timed("elastic_displace", n * 24 + f.numel() * 4):
        check(lib.dva_elastic_displace(ptr(p), n, ptr(f), ptr(ax), dx, dy, dz, float(magnitude), ptr(out),
                                       stream_of(p)), "dva_elastic_displace")
    return out


def minmax3(pos):
    """Column minima and maxima of ``pos`` float32 [N, 3], N >= 1: float32 [6] on the current HIP device (the three
    minima, then the three maxima).  Exact; one pass over ``pos``."""
    lib = _lib.load()
    p = _elastic_pos(pos, "minmax3")
    if p.shape[0] == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    ws, nbytes = _lib.workspace("dva_minmax3_workspace_bytes", p.device)
    out = torch.empty(6, dtype=torch.float32, device=p.device)
    with _timed("minmax3", p.numel() * 4):
        check(lib.dva_minmax3_f32(ptr(p), p.shape[0], ptr(out), ptr(ws), nbytes, stream_of(p)), "dva_minmax3_f32")
    return out


def elastic_distortion(pos, granularity, magnitude, noise=None):
    """One level of the reference's ``ElasticDistortion.elastic_distortion(coords, granularity, magnitude)``, bit for
    bit, for ``pos`` float32 [N, 3] on any device; returns float32 [N, 3] on the current HIP device.

    The bounds of ``pos`` are reduced on the device and read back (six floats, the one host synchronisation); the
    shape of the noise volume and its knot axes are then computed on the host with the reference's own numpy
    expressions, whose promotion rules decide their bits.  ``noise`` float32 ``[*noise_dim, 3]`` is drawn from numpy's
    global generator when it is not given, exactly as the reference draws it (``np.random.seed`` gives the same
    sample), and uploaded; a ``noise`` of another shape raises ValueError.  Smoothing and interpolation are
    ``elastic_smooth`` and ``elastic_displace``.  An empty cloud raises as numpy's reduction does; non-finite ``pos``
    is not supported."""
    p = _elastic_pos(pos, "elastic_distortion")
    bounds = minmax3(p).cpu().numpy()                      # host read: the volume's shape follows from the bounds
    coords_min = bounds[:3]
    # fp32(x - min) is monotone in x, so this is the reference's (coords - coords_min).max(0)
    extent = bounds[3:] - coords_min
    noise_dim = (extent // granularity).astype(int) + 3
    shape = tuple(int(d) for d in noise_dim) + (3,)
    if 3 * int(noise_dim[0]) * int(noise_dim[1]) * int(noise_dim[2]) >= 1 << 31:
        raise ValueError(f"ops.elastic_distortion: a noise volume of shape {shape} at granularity {granularity}; "
                         f"the kernels take fewer than 2^31 elements")
    if noise is None:
        noise = np.random.randn(*noise_dim, 3).astype(np.float32)
    elif tuple(noise.shape) != shape:
        raise ValueError(f"ops.elastic_distortion: noise of shape {tuple(noise.shape)}, the bounds of pos at "
                         f"granularity {granularity} need {shape}")
    ax = [
        np.linspace(d_min, d_max, d)
        for d_min, d_max, d in zip(coords_min - granularity, coords_min + granularity * (noise_dim - 2), noise_dim)
    ]
    return elastic_displace(p, elastic_smooth(noise), ax, magnitude)


# ---------------------------------------------------------------------------------------------
# the image tail (core/data_transform/multimodal/image.py:1195-1282: ColorJitter, RandomHorizontalFlip, ToFloatImage,
# Normalize; csrc/image_tail.hip)
# ---------------------------------------------------------------------------------------------

JITTER_CODE = {"brightness": 0, "contrast": 1, "saturation": 2}      # DVA_JITTER_*
IMAGE_MAX_CHANNELS = 64                                               # DVA_IMAGE_MAX_CHANNELS


def _image_tail_stats(mean, std, channels, what="ops.image_tail"):
    """``mean`` / ``std`` as two ctypes float arrays of ``channels`` entries, or (None, None)."""
    import ctypes
    if mean is None and std is None:
        return None, None
    if mean is None or std is None:
        raise ValueError(f"{what}: mean and std go together")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != channels or len(std) != channels:
        raise ValueError(f"{what}: {len(mean)} means and {len(std)} stds for {channels} channels")
    if channels > IMAGE_MAX_CHANNELS:
        raise ValueError(f"{what}: {channels} channels, the kernel normalises at most {IMAGE_MAX_CHANNELS}")
    arr = ctypes.c_float * channels
    std_f32 = arr(*std)
    if any(v == 0 for v in std_f32):
        raise ValueError(f"{what}: std evaluated to zero after conversion to float32: {std}")
    return arr(*mean), std_f32


def _image_jitter_ops(jitter, what="ops.image_tail"):
    """The ``(name, factor)`` list of a call, checked: ``(names, int32 codes, double factors)`` for the C ABI."""
    import ctypes
    jitter = [(str(name), float(factor)) for name, factor in jitter]
    names = [name for name, _ in jitter]
    for name, factor in jitter:
        if name not in JITTER_CODE:
            raise ValueError(f"{what}: unknown jitter op {name!r} (one of {sorted(JITTER_CODE)})")
        if not (0.0 <= factor < float("inf")):
            raise ValueError(f"{what}: the {name} factor must be a finite number >= 0, got {factor}")
    if len(set(names)) != len(names):
        raise ValueError(f"{what}: every jitter op at most once, got {names}")
    codes = (ctypes.c_int32 * len(jitter))(*[JITTER_CODE[name] for name in names])
    factors = (ctypes.c_double * len(jitter))(*[factor for _, factor in jitter])
    return names, codes, factors


def image_tail(x, jitter=(), flip=False, to_float=False, mean=None, std=None):
    """The per-pixel tail of the image transform chains in one pass: the ``jitter`` ops, the horizontal ``flip``,
    ``ToFloatImage`` (``to_float``) and ``Normalize`` (``mean`` / ``std``), in that order, whichever are asked for.

    ``x`` uint8 ``[B, 3, H, W]``: ``jitter`` is a sequence of ``(name, factor)`` with the names ``brightness``,
    ``contrast``, ``saturation``, each at most once, applied in the given order with ``factor >= 0``.  Returns uint8
    ``[B, 3, H, W]`` without ``to_float`` and float32 with it; ``mean`` / ``std`` (three numbers each) need
    ``to_float``.  ``x`` float32 ``[B, C, H, W]``: ``mean`` / ``std`` (C numbers each, C <= 64) alone.

    The contract is this arithmetic, restated from torchvision 0.8.2's ``ColorJitter.forward`` and
    ``functional_tensor`` (the reference's transforms wrap that package; parity with it is unpinned, no fixture of it
    exists) -- float32 throughout, every operation rounded on its own, true division, ``u8`` = truncation:
    ``gray = u8((f32(0.2989) r + f32(0.587) g) + f32(0.114) b)``; ``blend(p, q, f) = u8(clamp(f32(f) p + f32(1.0 - f)
    q, 0, 255))`` with ``1.0 - f`` taken in double; brightness ``blend(p, 0, f)``, saturation ``blend(p, gray, f)``,
    contrast ``blend(p, m_i, f)`` with ``m_i = f32(S_i) / f32(H W)``, ``S_i`` the exact integer sum of ``gray`` over
    image ``i`` after the ops that precede contrast (where ``H W <= 65793`` this is ``torch.mean`` of the gray image
    bit for bit, beyond it ``torch.mean`` depends on torch's summation order and the integer sum is the definition);
    flip: output column ``w`` takes source column ``W - 1 - w``; ``f32(p) / f32(255)``; ``(v - mean[c]) / std[c]``.

    One kernel, two with contrast (integer atomics only: the same call gives the same bytes); no host
    synchronisation.  A call that asks for nothing returns ``x`` itself."""
    if not torch.is_tensor(x):
        raise TypeError("ops.image_tail: x must be a tensor")
    dev = require_device(x)
    jitter = [(str(name), float(factor)) for name, factor in jitter]
    if x.dim() != 4:
        raise ValueError(f"ops.image_tail: x must be [B, C, H, W], got {tuple(x.shape)}")
    B, C, H, W = (int(d) for d in x.shape)
    if x.dtype != torch.uint8:
        if jitter:
            raise TypeError(f"ops.image_tail: jitter takes uint8 images, got {x.dtype}")
        if x.dtype != torch.float32:
            raise TypeError(f"ops.image_tail takes uint8 or float32 images, got {x.dtype}")
        if to_float:
            raise TypeError("ops.image_tail: to_float takes uint8 images, x is float32 already")
        if flip:
            raise TypeError("ops.image_tail: the flip is fused into the uint8 pass only, x is float32")
    else:
        if C != 3:
            raise ValueError(f"ops.image_tail: uint8 images must be [B, 3, H, W], got {tuple(x.shape)}")
        if (mean is not None or std is not None) and not to_float:
            raise TypeError("ops.image_tail: Normalize takes float images; pass to_float=True for uint8 input")
    names, codes, factors = _image_jitter_ops(jitter)
    mean_c, std_c = _image_tail_stats(mean, std, C)
    lib = _lib.load()
    if x.dtype == torch.float32:
        if mean_c is None:
            return x
        x = x.contiguous()
        out = torch.empty_like(x)
        if x.numel() == 0:
            return out
        with _timed("image_normalize_f32", 2 * x.numel() * 4):
            check(lib.dva_image_normalize_f32(ptr(x), B, C, H * W, mean_c, std_c, ptr(out), stream_of(x)),
                  "dva_image_normalize_f32")
        return out
    if not jitter and not flip and not to_float:
        return x
    x = x.contiguous()
    out = torch.empty((B, C, H, W), dtype=torch.float32 if to_float else torch.uint8, device=dev)
    if x.numel() == 0:
        return out
    ws, ws_bytes = None, 0
    if "contrast" in names:
        ws, ws_bytes = _lib.workspace("dva_image_tail_workspace_bytes", dev, B)
    pixels = B * H * W
    with _timed("image_tail", pixels * (3 + (3 if ws is not None else 0) + (12 if to_float else 3))):
        check(lib.dva_image_tail_u8(ptr(x), B, H, W, codes, factors, len(jitter), int(bool(flip)), int(bool(to_float)),
                                    mean_c, std_c, ptr(out), ptr(ws), ws_bytes, stream_of(x)), "dva_image_tail_u8")
    return out


def image_window(src, index, rollings=None, offsets=None, size=None, jitter=(), flip=False, to_float=False, mean=None,
                 std=None):
    """``ops.image_tail`` over windows of source images that are never materialised: the deferred roll, crop and image
    selection of the online image chains, folded into the tail's one pass.

    ``src`` uint8 ``[N, 3, H, W]``; ``index`` int64 ``[B]`` picks the source image of every output image, ``rollings``
    int64 ``[B]`` rolls it along W (``None``: no roll), ``offsets`` int64 ``[B, 2]`` holds the (x, y) of the window in
    the rolled image (``None``: zeros) and ``size = (Wc, Hc)`` its size in the project's (W, H) convention (``None``:
    the whole image), ``1 <= Wc <= W``, ``1 <= Hc <= H``::

        win[b, c, y, x] = src[index[b], c, offsets[b, 1] + y, (offsets[b, 0] + x - rollings[b]) mod W]
        out             = image_tail(win, jitter, flip, to_float, mean, std)

    which is ``update_cropping(update_rollings(src[index]))`` of ``SameSettingImageData`` followed by
    ``ops.image_tail``, bit for bit: the flip mirrors window columns, the contrast mean is taken over the window of
    each output image alone.  Returns uint8 ``[B, 3, Hc, Wc]`` without ``to_float`` and float32 with it (always a new
    tensor).  ``index`` / ``rollings`` / ``offsets`` stay on the device and are not read back: an image outside
    ``[0, N)`` or a window row outside the image is the caller's error, clamped by the kernel for memory safety, its
    pixels unspecified.  One kernel, two with contrast; no host synchronisation."""
    what = "ops.image_window"
    if not torch.is_tensor(src) or not torch.is_tensor(index):
        raise TypeError(f"{what}: src and index must be tensors")
    dev = require_device(src, index, rollings, offsets)
    if src.dim() != 4 or src.shape[1] != 3:
        raise ValueError(f"{what}: uint8 images must be [N, 3, H, W], got {tuple(src.shape)}")
    if src.dtype != torch.uint8:
        raise TypeError(f"{what} takes uint8 images, got {src.dtype}")
    N, _, H, W = (int(d) for d in src.shape)
    if index.dim() != 1 or index.dtype != torch.int64:
        raise TypeError(f"{what}: index must be int64 [B], got {index.dtype} {tuple(index.shape)}")
    B = int(index.shape[0])
    if rollings is not None and (rollings.dtype != torch.int64 or tuple(rollings.shape) != (B,)):
        raise TypeError(f"{what}: rollings must be int64 [{B}], got {rollings.dtype} {tuple(rollings.shape)}")
    if offsets is not None and (offsets.dtype != torch.int64 or tuple(offsets.shape) != (B, 2)):
        raise TypeError(f"{what}: offsets must be int64 [{B}, 2], got {offsets.dtype} {tuple(offsets.shape)}")
    Wc, Hc = (W, H) if size is None else (int(size[0]), int(size[1]))
    if not (1 <= Wc <= W and 1 <= Hc <= H):
        raise ValueError(f"{what}: the window (W, H) = {(Wc, Hc)} does not fit the images {(W, H)}")
    if (mean is not None or std is not None) and not to_float:
        raise TypeError(f"{what}: Normalize takes float images; pass to_float=True for uint8 input")
    names, codes, factors = _image_jitter_ops(jitter, what)
    mean_c, std_c = _image_tail_stats(mean, std, 3, what)
    lib = _lib.load()
    out = torch.empty((B, 3, Hc, Wc), dtype=torch.float32 if to_float else torch.uint8, device=dev)
    if B == 0:
        return out
    if N == 0:
        raise ValueError(f"{what}: {B} images asked of an empty source")
    src, index = src.contiguous(), index.contiguous()
    rollings = torch.zeros(B, dtype=torch.int64, device=dev) if rollings is None else rollings.contiguous()
    offsets = torch.zeros((B, 2), dtype=torch.int64, device=dev) if offsets is None else offsets.contiguous()
    ws, ws_bytes = None, 0
    if "contrast" in names:
        ws, ws_bytes = _lib.workspace("dva_image_window_workspace_bytes", dev, B)
    pixels = B * Hc * Wc
    with _timed("image_window", pixels * (3 + (3 if ws is not None else 0) + (12 if to_float else 3))):
        check(lib.dva_image_window_u8(ptr(src), N, H, W, ptr(index), ptr(rollings), ptr(offsets), B, Wc, Hc, codes,
                                      factors, len(names), int(bool(flip)), int(bool(to_float)), mean_c, std_c, ptr(out),
                                      ptr(ws), ws_bytes, stream_of(src)), "dva_image_window_u8")
    return out


# ---------------------------------------------------------------------------------------------
# loading images: SameSettingImageData.read_images after the decode (core/multimodal/image.py:1059-1099: PIL resize,
# roll, crop or box resize) and NonStaticMask's comparison (core/data_transform/multimodal/image.py:130-154);
# csrc/image_load.hip
# ---------------------------------------------------------------------------------------------

IMAGE_RESAMPLE_BITS = 22                                                              # Pillow's PRECISION_BITS


def image_resample_tables(in_size, in0, in1, out_size):
    """The coefficient table of one axis of Pillow's 8-bit BICUBIC resample (``Image.resize`` on an RGB image): input
    length ``in_size``, box ``[in0, in1)``, output length ``out_size``.  Returns ``(coeffs, bounds)``: int32
    ``[out_size, ksize]`` fixed-point weights (22 fractional bits, zero beyond a row's ``xmax``) and int32
    ``[out_size, 2]`` rows ``(xmin, xmax)``.  Everything is float64, every operation rounded on its own, in the order of
    the C source (include/dva.h states the expressions); the weight sum ``ww`` is the sequential one."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"image_resample_tables: sizes must be positive, got {in_size} -> {out_size}")
    in0, in1 = float(in0), float(in1)
    if not (0 <= in0 < in1 <= in_size):
        raise ValueError(f"image_resample_tables: the box [{in0}, {in1}) does not lie in [0, {in_size}]")
    scale = (in1 - in0) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = in0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    arg = np.abs((((x + xmin[:, None]).astype(np.float64) - center[:, None]) + 0.5) * ss)
    with np.errstate(invalid='ignore', over='ignore'):
        near = ((1.5 * arg - 2.5) * arg) * arg + 1
        far = (((arg - 5) * arg + 8) * arg - 4) * -0.5
    w = np.where(arg < 1.0, near, np.where(arg < 2.0, far, 0.0))
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                      # x = 0, 1, ... in order; the zeros beyond xmax add nothing
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    one = float(1 << IMAGE_RESAMPLE_BITS)
    coeffs = np.trunc(np.where(w < 0, -0.5 + w * one, 0.5 + w * one)).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    return coeffs, bounds


def _image_identity_table(n):
    """The table of a pass that copies: one tap of weight 1 at the output's own index (``(2^21 + p 2^22) >> 22 = p``)."""
    coeffs = np.full((n, 1), 1 << IMAGE_RESAMPLE_BITS, dtype=np.int32)
    bounds = np.stack([np.arange(n), np.ones(n, dtype=np.int64)], axis=1).astype(np.int32)
    return coeffs, bounds


class _ResamplePass:
    """One launch of ``dva_image_resample_u8``: its axis, its tables (one per distinct box), the output size, and the
    per-image table index, shifts and periods (``_lib.SIGNATURES`` / include/dva.h)."""

    def __init__(self, axis, tables, table_index, out_hw, B):
        self.axis = axis
        self.coeffs = np.stack([t[0] for t in tables])
        self.bounds = np.stack([t[1] for t in tables])
        self.table_index = np.asarray(table_index, dtype=np.int32).reshape(B)
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.shifts = np.zeros((B, 3), dtype=np.int32)
        self.periods = [0, 0, 0]                              # out, src, other


def _image_box_pass(axis, in_size, starts, length, out_size, out_hw, B):
    """The pass along ``axis`` that resamples ``[start, start + length)`` of ``in_size`` pixels to ``out_size``, one
    table per distinct start (the border clamp and the rounding of the centres differ between them)."""
    distinct, inverse = np.unique(np.asarray(starts, dtype=np.int64), return_inverse=True)
    tables = [image_resample_tables(in_size, int(s), int(s) + length, out_size) for s in distinct]
    return _ResamplePass(axis, tables, inverse, out_hw, B)


def _image_run_passes(src, passes, what):
    """Run the passes over ``src`` uint8 ``[B, Hs, Ws, 3]``: every table, table index and shift goes up in one copy, every
    pass but the last writes an HWC intermediate, the last writes the planar ``[B, 3, H, W]`` result."""
    lib = _lib.load()
    dev = src.device
    B, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    Ho, Wo = passes[-1].out_hw
    out = torch.empty((B, 3, Ho, Wo), dtype=torch.uint8, device=dev)
    if B == 0 or Ho == 0 or Wo == 0:
        return out
    parts, offsets, at = [], [], 0
    for p in passes:
        mine = []
        for a in (p.coeffs, p.bounds, p.table_index, p.shifts):
            mine.append(at)
            parts.append(np.ascontiguousarray(a, dtype=np.int32).reshape(-1))
            at += parts[-1].size
        offsets.append(mine)
    plan = torch.from_numpy(np.concatenate(parts)).to(dev)
    base = plan.data_ptr()
    cur, strides = src, (h * w * 3, w * 3, 3, 1)
    keep = [plan]
    for p, (o_coeffs, o_bounds, o_index, o_shifts) in zip(passes, offsets):
        ho, wo = p.out_hw
        if p is passes[-1]:
            dst, dstrides = out, (3 * ho * wo, wo, 1, ho * wo)
        else:
            dst, _ = _lib.workspace("dva_image_resample_workspace_bytes", dev, B, ho, wo)
            dstrides = (ho * wo * 3, wo * 3, 3, 1)
            keep.append(dst)
        n_tables, rows, ksize = (int(d) for d in p.coeffs.shape)
        taps = int(p.bounds[..., 1].max())
        with _timed("image_resample", B * ho * wo * 3 * (1 + taps)):
            check(lib.dva_image_resample_u8(
                ptr(cur), B, h, w, *strides, ptr(dst), ho, wo, *dstrides, p.axis,
                ctypes.c_void_p(base + 4 * o_coeffs), ctypes.c_void_p(base + 4 * o_bounds), n_tables, rows, ksize,
                ctypes.c_void_p(base + 4 * o_index), ctypes.c_void_p(base + 4 * o_shifts), *p.periods,
                stream_of(src)), f"dva_image_resample_u8 ({what})")
        cur, strides, h, w = dst, dstrides, ho, wo
    return out


def _image_sources(src, what):
    if not torch.is_tensor(src):
        raise TypeError(f"{what}: src must be a tensor")
    dev = require_device(src)
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f"{what}: decoded images must be [N, H, W, 3], got {tuple(src.shape)}")
    if src.dtype != torch.uint8:
        raise TypeError(f"{what} takes uint8 images, got {src.dtype}")
    if src.shape[0] > 0 and (src.shape[1] < 1 or src.shape[2] < 1):
        raise ValueError(f"{what}: empty images {tuple(src.shape)}")
    return src.contiguous(), dev


def _image_size(size, what, name="size"):
    size = tuple(int(v) for v in size)
    if len(size) != 2 or size[0] < 1 or size[1] < 1:
        raise ValueError(f"{what}: {name} must be a positive (W, H), got {size}")
    return size


def image_resample(src, size, box=None):
    """``PIL.Image.resize(size, box=box)`` (BICUBIC, Pillow's 8-bit fixed-point resample) of a batch of decoded RGB
    images, bit for bit: ``src`` uint8 ``[N, Hs, Ws, 3]`` on the device, ``size = (W, H)``, ``box = (left, top, right,
    bottom)`` in source pixels (``None``: the whole image; fractions allowed, as in Pillow).  Returns uint8
    ``[N, 3, H, W]``.  A horizontal pass into a uint8 intermediate, then a vertical pass; a pass whose axis keeps its
    length with the box covering it is skipped, as in Pillow, and with both skipped the one launch is a copy into the
    planar layout.  The coefficient tables are computed on the host (``image_resample_tables``) and uploaded in one
    copy; nothing is read back."""
    what = "ops.image_resample"
    src, dev = _image_sources(src, what)
    N, Hs, Ws = (int(d) for d in src.shape[:3])
    W, H = _image_size(size, what)
    if N == 0:
        return torch.empty((0, 3, H, W), dtype=torch.uint8, device=dev)
    x0, y0, x1, y1 = (0, 0, Ws, Hs) if box is None else (float(v) for v in box)
    if x0 < 0 or y0 < 0 or x1 > Ws or y1 > Hs:
        raise ValueError(f"{what}: box can't exceed original image size")
    if x1 <= x0 or y1 <= y0:
        raise ValueError(f"{what}: box can't be empty")
    passes = []
    if W != Ws or x0 != 0 or x1 != Ws:
        passes.append(_ResamplePass(0, [image_resample_tables(Ws, x0, x1, W)], np.zeros(N), (Hs, W), N))
    if H != Hs or y0 != 0 or y1 != Hs:
        passes.append(_ResamplePass(1, [image_resample_tables(Hs, y0, y1, H)], np.zeros(N), (H, W), N))
    if not passes:
        passes.append(_ResamplePass(0, [_image_identity_table(W)], np.zeros(N), (H, W), N))
    return _image_run_passes(src, passes, what)


def _host_int64(value, shape, what, name):
    """A per-image integer argument as a host int64 array (a device tensor is read back once, before any launch)."""
    if torch.is_tensor(value):
        if value.dtype != torch.int64:
            raise TypeError(f"{what}: {name} must be int64, got {value.dtype}")
        value = value.detach().cpu().numpy()
    value = np.asarray(value, dtype=np.int64)
    if value.shape != shape:
        raise ValueError(f"{what}: {name} must have shape {shape}, got {value.shape}")
    return value


def read_images_u8(src, size, rollings=None, crop_size=None, crop_offsets=None, downscale=None):
    """``SameSettingImageData.read_images`` after the decode (reference core/multimodal/image.py:1059-1099), bit for
    bit over Pillow's BICUBIC: every image of ``src`` (uint8 ``[N, Hs, Ws, 3]`` on the device, the decoded files) is
    resized to ``size = (W, H)``, rolled along the width (``new[x] = old[(x + rollings[i] mod W) mod W]``), and then,
    with ``downscale`` ``None``, cropped to ``crop_size = (w, h)`` at ``crop_offsets[i] = (left, top)``, otherwise
    resized to ``(int(w / downscale), int(h / downscale))`` from that box.  ``crop_size`` and ``crop_offsets`` come
    together or not at all (the whole image).  Returns uint8 ``[N, 3, H', W']``.

    One to four launches of the resample pass (``dva_image_resample_u8``): the passes Pillow would run, skipped under
    Pillow's rule, with the roll and the crop folded into them as per-image shifts -- into the passes of the second
    resize, or into the last pass of the first one when no second resize happens (then an unchanged size is one copy
    pass).  No rolled or cropped image is written.  ``rollings`` and ``crop_offsets`` are HOST values (int64 tensors,
    arrays or sequences): a box resize needs one coefficient table per distinct offset, computed on the host; a device
    tensor is read back once before the first launch.  Nothing else synchronises."""
    what = "ops.read_images_u8"
    src, dev = _image_sources(src, what)
    N, Hs, Ws = (int(d) for d in src.shape[:3])
    passes, (end_h, end_w) = _read_images_plan(N, Hs, Ws, size, rollings, crop_size, crop_offsets, downscale, what)
    if N == 0:
        return torch.empty((0, 3, end_h, end_w), dtype=torch.uint8, device=dev)
    return _image_run_passes(src, passes, what)


def _read_images_plan(N, Hs, Ws, size, rollings, crop_size, crop_offsets, downscale, what="ops.read_images_u8"):
    """The passes of ``read_images_u8`` over ``N`` sources of ``Hs x Ws`` pixels and the ``(H, W)`` of its result: host
    work only (argument checks, tables, shifts)."""
    W1, H1 = _image_size(size, what)
    if bool(crop_size) != bool(crop_offsets is not None):
        raise ValueError(f"{what}: if either 'crop_size' or 'crop_offsets' is specified, both must be specified")
    roll = np.zeros(N, dtype=np.int64) if rollings is None else _host_int64(rollings, (N,), what, "rollings")
    roll = roll % W1                                             # non-negative, as Python's and the reference's
    if crop_size is not None:
        w, h = _image_size(crop_size, what, "crop_size")
        if w > W1 or h > H1:
            raise ValueError(f"{what}: expected crop_size to be smaller than size but got size={(W1, H1)} and "
                             f"crop_size={(w, h)} instead")
        offs = _host_int64(crop_offsets, (N, 2), what, "crop_offsets")
        if N and (offs.min() < 0 or (offs[:, 0] + w).max() > W1 or (offs[:, 1] + h).max() > H1):
            raise ValueError(f"{what}: a crop box leaves the resized image {(W1, H1)}")
    else:
        w, h = W1, H1
        offs = np.zeros((N, 2), dtype=np.int64)
    if downscale is not None:
        if not downscale >= 1:
            raise ValueError(f"{what}: expected scalar larger than 1 but got {downscale} instead")
        end_w, end_h = int(w / downscale), int(h / downscale)
        if end_w < 1 or end_h < 1:
            raise ValueError(f"{what}: height and width must be > 0, got {(end_w, end_h)}")
    else:
        end_w, end_h = w, h
    if N == 0:
        return [], (end_h, end_w)
    left, top = offs[:, 0], offs[:, 1]

    passes = []
    if Ws != W1:
        passes.append(_ResamplePass(0, [image_resample_tables(Ws, 0, Ws, W1)], np.zeros(N), (Hs, W1), N))
    if Hs != H1:
        passes.append(_ResamplePass(1, [image_resample_tables(Hs, 0, Hs, H1)], np.zeros(N), (H1, W1), N))
    second_h = downscale is not None and (end_w != W1 or w != W1)     # w == W1 leaves left = 0 only
    second_v = downscale is not None and (end_h != H1 or h != H1)
    if second_h:
        p = _image_box_pass(0, W1, left, w, end_w, (H1, end_w), N)
        p.shifts[:, 1], p.periods[1] = roll, W1                      # its taps read the rolled image
        passes.append(p)
    if second_v:
        p = _image_box_pass(1, H1, top, h, end_h, (end_h, end_w), N)
        if not second_h:
            p.shifts[:, 2], p.periods[2] = roll, W1                  # the roll runs across this pass
        passes.append(p)
    if not (second_h or second_v):
        # no second resize: the window (roll, then crop) of the first one's result, read by its last pass
        if not passes:
            passes.append(_ResamplePass(0, [_image_identity_table(W1)], np.zeros(N), (H1, W1), N))
        p = passes[-1]
        if p.axis == 0:
            p.shifts[:, 0], p.periods[0] = left + roll, W1
            p.shifts[:, 2] = top
        else:
            p.shifts[:, 0] = top
            p.shifts[:, 2], p.periods[2] = left + roll, W1
        p.out_hw = (h, w)
    return passes, (end_h, end_w)


def image_nonstatic_mask(images):
    """NonStaticMask's comparison (reference core/data_transform/multimodal/image.py:139-154) in one launch:
    ``images`` uint8 ``[n, 3, H, W]``, image 0 the reference view; returns bool ``[W, H]`` (the reference's transposed
    ``proj_size`` orientation) with ``mask[x, y] = any_{i >= 1} all_c images[0, c, y, x] != images[i, c, y, x]``."""
    what = "ops.image_nonstatic_mask"
    if not torch.is_tensor(images):
        raise TypeError(f"{what}: images must be a tensor")
    dev = require_device(images)
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
        raise ValueError(f"{what}: images must be [n >= 1, 3, H, W], got {tuple(images.shape)}")
    if images.dtype != torch.uint8:
        raise TypeError(f"{what} takes uint8 images, got {images.dtype}")
    images = images.contiguous()
    n, _, H, W = (int(d) for d in images.shape)
    mask = torch.empty((W, H), dtype=torch.bool, device=dev)
    with _timed("image_nonstatic_mask", n * 3 * H * W + H * W):
        check(_lib.load().dva_image_nonstatic_mask(ptr(images), n, H, W, ptr(mask), stream_of(images)),
              "dva_image_nonstatic_mask")
    return mask


# ---------------------------------------------------------------------------------------------
# the positional 3D augmentations (core/data_transform/transforms.py:463-563, features.py:30-81: RandomNoise,
# Random3AxisRotation, RandomScaleAnisotropic, RandomSymmetry; torch_geometric's RandomRotate and Center;
# csrc/cloud_augment.hip)
# ---------------------------------------------------------------------------------------------

CLOUD_STEP_CODE = {"noise": 0, "linear": 1, "scale": 2, "flip": 3, "center": 4}      # DVA_CLOUD_*
CLOUD_MAX_STEPS = 16                                                                  # DVA_CLOUD_MAX_STEPS
CLOUD_STEP_PARAMS = 10                                                                # DVA_CLOUD_STEP_PARAMS


def _cloud_floats(value, count, what):
    """``count`` float32 values of a host tensor, array or nested sequence, as Python floats (exact)."""
    flat = torch.as_tensor(value).detach().cpu().to(torch.float32).reshape(-1).tolist()
    if len(flat) != count:
        raise ValueError(f"ops.cloud_augment: {what} takes {count} numbers, got {len(flat)}")
    return flat


def cloud_augment(pos, steps, norm=None, noise=None):
    """An ordered list of positional augmentation steps in one pass over ``pos`` float32 [N, 3] and, when given, ``norm``
    float32 [N, 3]; returns ``(pos_out, norm_out, consts)``, new tensors (``norm_out`` is ``norm`` itself when no step
    touches it, None without ``norm``).  The random draws are the caller's; ``steps`` holds the drawn values, at most
    16 of:

    ``("noise",)``                 ``p_c = p_c + e_c``, ``e`` the point's row of ``noise`` float32 [N, 3] on the device
    ``("linear", M, with_norm)``   ``q_i = ((p_0 M_i0 + p_1 M_i1) + p_2 M_i2)``, ``M`` 3 x 3 host values; the same for
                                   ``norm`` when ``with_norm``.  This is ``pos @ M.T``.
    ``("scale", s)``               ``p_c = p_c * s_c``, ``s`` 3 host values; with ``norm``: ``n_c = n_c / s_c``,
                                   ``l = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2)``, ``n_c = n_c / max(l, 1e-12)``
    ``("flip", mask)``             on every axis flagged in ``mask`` (3 bools, at least one set): ``p_c = m_c - p_c``,
                                   ``m_c`` the exact maximum of ``p_c`` over the points at this stage
    ``("center",)``                ``p_c = p_c - mu_c``, ``mu_c = f32(S_c / N)``, ``S_c`` the float64 sum of the stage's
                                   float32 values, the division in float64

    float32 throughout, every operation rounded on its own, divisions and square roots correctly rounded.  ``consts``
    float32 [number of flip and center steps, 3] holds the ``m`` / ``mu`` rows that were used, in step order, 0 on the
    axes a flip leaves alone.  One apply kernel, and in front of it one reduction launch per flip / center step; no
    atomics, the same call gives the same bytes; no host synchronisation.  ``N = 0`` launches nothing.  ``3 N >= 2^31``
    raises ``DvaError`` with code ``DVA_ERR_UNSUPPORTED``.

    Against the torch composition of the reference's lines: noise, scale on ``pos`` and flip are its results bit for
    bit; linear differs from a BLAS ``matmul`` within ``6 * 2^-24 * sum_j |p_j| |M_ij|`` (each side lies within half of
    that of the exact value); center subtracts the correctly rounded mean where torch's float32 ``mean`` carries its
    summation error."""
    import ctypes
    if not torch.is_tensor(pos):
        raise TypeError("ops.cloud_augment: pos must be a tensor")
    dev = require_device(pos, norm, noise)
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3:
        raise TypeError(f"ops.cloud_augment: pos must be float32 [N, 3], got {pos.dtype} {tuple(pos.shape)}")
    n = int(pos.shape[0])
    for name, t in (("norm", norm), ("noise", noise)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (n, 3)):
            raise TypeError(f"ops.cloud_augment: {name} must be float32 [{n}, 3], got {t.dtype} {tuple(t.shape)}")
    steps = [tuple(s) for s in steps]
    if len(steps) > CLOUD_MAX_STEPS:
        raise ValueError(f"ops.cloud_augment: {len(steps)} steps, the kernel takes at most {CLOUD_MAX_STEPS}")
    codes = (ctypes.c_int32 * max(len(steps), 1))()
    params = (ctypes.c_float * (max(len(steps), 1) * CLOUD_STEP_PARAMS))()
    n_reduce, with_norm, with_noise = 0, False, False
    for k, step in enumerate(steps):
        name, args = step[0], step[1:]
        if name not in CLOUD_STEP_CODE:
            raise ValueError(f"ops.cloud_augment: unknown step {name!r} (one of {sorted(CLOUD_STEP_CODE)})")
        codes[k] = CLOUD_STEP_CODE[name]
        row = [0.0] * CLOUD_STEP_PARAMS
        if name == "noise":
            if noise is None:
                raise ValueError("ops.cloud_augment: a noise step needs the noise tensor")
            with_noise = True
        elif name == "linear":
            row[:9] = _cloud_floats(args[0], 9, "a linear step's matrix")
            if len(args) > 1 and args[1]:
                if norm is None:
                    raise ValueError("ops.cloud_augment: a linear step with_norm needs norm")
                row[9], with_norm = 1.0, True
        elif name == "scale":
            row[:3] = _cloud_floats(args[0], 3, "a scale step")
            if norm is not None:
                row[9], with_norm = 1.0, True
        elif name == "flip":
            mask = [bool(a) for a in args[0]]
            if len(mask) != 3 or not any(mask):
                raise ValueError(f"ops.cloud_augment: a flip step takes three flags, at least one set, got {args[0]}")
            row[:3] = [float(a) for a in mask]
            n_reduce += 1
        else:
            n_reduce += 1
        params[k * CLOUD_STEP_PARAMS:(k + 1) * CLOUD_STEP_PARAMS] = row
    if 3 * n >= 1 << 31:
        raise _unsupported("cloud_augment", f"{n} points; the kernels take 3 N < 2^31")
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    norm_out = norm if not with_norm else torch.empty((n, 3), dtype=torch.float32, device=dev)
    consts = torch.empty((n_reduce, 3), dtype=torch.float32, device=dev)
    if n == 0:
        return out, norm_out, consts
    lib = _lib.load()
    pos = pos.contiguous()
    norm_in = norm.contiguous() if with_norm else None
    noise_in = noise.contiguous() if with_noise else None
    ws, ws_bytes = None, 0
    if n_reduce:
        ws, ws_bytes = _lib.workspace("dva_cloud_augment_workspace_bytes", dev, n, n_reduce)
    # every launch reads pos (and noise); the apply launch also reads norm and writes pos_out (and norm_out)
    with _timed("cloud_augment", n * 12 * ((n_reduce + 1) * (1 + bool(with_noise)) + 1 + 2 * bool(with_norm))):
        check(lib.dva_cloud_augment_f32(ptr(pos), ptr(norm_in), ptr(noise_in), n, codes, params, len(steps), ptr(out),
                                        ptr(norm_out) if with_norm else None, ptr(consts), ptr(ws), ws_bytes,
                                        stream_of(pos)), "dva_cloud_augment_f32")
    return out, norm_out, consts


# ---------------------------------------------------------------------------------------------
# the tail of the segmentation step (csrc/segloss.hip): log-softmax + weighted NLL, Lovasz-softmax, confusion counts
# ---------------------------------------------------------------------------------------------

SEG_MAX_CLASSES = 64
LOVASZ_TILE = 1024      # sorted elements per block of the segmented Lovasz pass (DVA_LOVASZ_TILE; tests size their cases by it)


def _seg_inputs(what, scores, labels, dtypes):
    """``scores`` [P, C] and ``labels`` [P] on one HIP device, within the kernels' limits; labels as contiguous int64."""
    if not torch.is_tensor(scores) or not torch.is_tensor(labels):
        raise TypeError(f"ops.{what} takes tensors")
    require_device(scores, labels)
    if scores.dtype not in dtypes:
        raise TypeError(f"ops.{what}: [P, C] input of dtype {scores.dtype}; supported: {', '.join(str(d) for d in dtypes)}")
    if scores.dim() != 2:
        raise ValueError(f"ops.{what}: the scores must be [P, C], got {tuple(scores.shape)}")
    P, C = int(scores.shape[0]), int(scores.shape[1])
    if labels.dim() != 1 or labels.shape[0] != P:
        raise ValueError(f"ops.{what}: labels must be [P] = [{P}], got {tuple(labels.shape)}")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise TypeError(f"ops.{what}: labels must be integers, got {labels.dtype}")
    if not 1 <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"ops.{what}: C = {C} classes; the kernels take 1 <= C <= {SEG_MAX_CLASSES}")
    if P * C >= 1 << 31:
        raise ValueError(f"ops.{what}: P * C = {P} * {C} elements; the kernels take fewer than 2^31")
    return P, C, labels.detach().to(torch.int64).contiguous()


_SEG_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


class _LogSoftmaxNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index):
        lib = _lib.load()
        x = logits.detach().contiguous()
        P, C = x.shape
        dev = x.device
        logp = torch.empty((P, C), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        numden = torch.empty(2, dtype=torch.float64, device=dev)
        ws, nbytes = _lib.workspace("dva_seg_nll_workspace_bytes", dev)
        with _timed("seg_logsoftmax_nll_fwd", x.numel() * (x.element_size() + 4)):
            check(lib.dva_seg_logsoftmax_nll_fwd(ptr(x), dtype_code(x), ptr(labels), ptr(weight), int(ignore_index), P, C,
                                                 ptr(logp), ptr(loss), ptr(numden), ptr(ws), nbytes, stream_of(x)),
                  "dva_seg_logsoftmax_nll_fwd")
        ctx.save_for_backward(logp, labels, weight, numden)
        ctx.ignore_index = int(ignore_index)
        ctx.dtype = x.dtype
        ctx.set_materialize_grads(False)
        return logp, loss.reshape(())

    @staticmethod
    def backward(ctx, g_logp, g_loss):
        logp, labels, weight, numden = ctx.saved_tensors
        if g_logp is None and g_loss is None:
            return None, None, None, None
        lib = _lib.load()
        P, C = logp.shape
        if g_logp is not None:
            g_logp = g_logp.to(torch.float32).contiguous()
        if g_loss is not None:
            g_loss = g_loss.to(torch.float32).reshape(1).contiguous()
        out = torch.empty((P, C), dtype=ctx.dtype, device=logp.device)
        with _timed("seg_logsoftmax_nll_bwd", logp.numel() * (8 + out.element_size())):
            check(lib.dva_seg_logsoftmax_nll_bwd(ptr(logp), ptr(labels), ptr(weight), ptr(numden), ptr(g_loss), ptr(g_logp),
                                                 ctx.ignore_index, P, C, ptr(out), dtype_code(out), stream_of(logp)),
                  "dva_seg_logsoftmax_nll_bwd")
        return out, None, None, None


def log_softmax_nll(logits, labels, weight=None, ignore_index=-1):
    """``F.log_softmax(logits, -1)`` and ``F.nll_loss(., labels, weight=weight, ignore_index=ignore_index)`` in one pass
    over ``logits`` [P, C] (float32, bfloat16 or float16; upcast exactly): returns ``(log_probs, loss)``, float32
    [P, C] and a float32 scalar, both differentiable (one backward kernel takes both upstream gradients and writes
    the logits gradient in the logits' dtype).  The loss is ``sum w[y] (-logp[y]) / sum w[y]`` over the rows whose
    label is not ``ignore_index``, reduced in float64 in a fixed order (bitwise reproducible); NaN when every label is
    ignored, as torch.  A label outside [0, C) that is not ``ignore_index`` takes no part (torch asserts on it).
    1 <= C <= 64 and P C < 2^31.  No host synchronisation."""
    P, C, lab = _seg_inputs("log_softmax_nll", logits, labels, _SEG_DTYPES)
    if weight is not None:
        require_device(logits, weight)
        if weight.dim() != 1 or weight.shape[0] != C:
            raise ValueError(f"ops.log_softmax_nll: weight must be [C] = [{C}], got {tuple(weight.shape)}")
        weight = weight.detach().to(torch.float32).contiguous()
    return _LogSoftmaxNLL.apply(logits, lab, weight, int(ignore_index))


# ---------------------------------------------------------------------------------------------
# the tail of the image-only models (models/segmentation/multimodal/no3d.py:102-154): csrc/nearest_seen.hip,
# csrc/view_loss.hip
# ---------------------------------------------------------------------------------------------

NEAREST_SEEN_LEVELS = 4     # grids of a search, cell x4 each; the last one walks every shell, so any cell is exact


def _nearest_seen(what, pos, seen, x, cell):
    lib = _lib.load()
    if not torch.is_tensor(pos) or not torch.is_tensor(seen):
        raise TypeError(f"ops.{what} takes tensors")
    require_device(pos, seen, x)
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"ops.{what}: pos must be [N, 3], got {tuple(pos.shape)}")
    n = int(pos.shape[0])
    if seen.dtype not in (torch.bool, torch.uint8) or seen.dim() != 1 or seen.shape[0] != n:
        raise ValueError(f"ops.{what}: seen must be bool or uint8 [N] = [{n}], got {seen.dtype} {tuple(seen.shape)}")
    pos = pos.detach().float().contiguous()
    seen8 = seen.detach().contiguous().view(torch.uint8)
    dev = pos.device
    filled, K, code = None, 0, 0
    if x is not None:
        if x.dim() != 2 or x.shape[0] != n or x.shape[1] < 1:
            raise ValueError(f"ops.{what}: x must be [N, K] = [{n}, K >= 1], got {tuple(x.shape)}")
        x = x.detach().contiguous()
        K, code = int(x.shape[1]), dtype_code(x)
        filled = torch.empty_like(x)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    any_seen = torch.zeros(1, dtype=torch.bool, device=dev)
    if n == 0:
        return src, any_seen, filled
    lo, hi = pos.min(0).values, pos.max(0).values
    bbox = torch.cat([lo, hi]).contiguous()
    ext = None
    if cell is None:
        box = bbox.cpu()                               # the one host read: the extent that sizes the cell
        ext = float((box[3:] - box[:3]).max())
        cell = _knn_default_cell(box[:3], box[3:], ext, n, 1) if ext > 0 else 1.0
    cell = max(float(cell), 1e-12)
    ws, nbytes = _lib.workspace("dva_nearest_seen_workspace_bytes", dev, n)
    done = torch.zeros(n, dtype=torch.uint8, device=dev)
    shells = 2
    with _timed(what, n * (13 + 4 + 2 * K * (x.element_size() if x is not None else 0))):
        for level in range(NEAREST_SEEN_LEVELS):
            last = level == NEAREST_SEEN_LEVELS - 1 or (ext is not None and cell * shells >= ext + cell)
            check(lib.dva_nearest_seen(ptr(pos), ptr(seen8), n, ptr(bbox), float(cell), shells, int(last), ptr(done),
                                       ptr(src), ptr(any_seen), ptr(x) if last else None, K, code,
                                       ptr(filled) if last else None, ptr(ws), int(nbytes), stream_of(pos)),
                  "dva_nearest_seen")
            if last:
                break
            cell *= 4.0
    return src, any_seen, filled


def nearest_seen(pos, seen, cell=None):
    """``(src int32 [N], any_seen bool [1])``: ``src[i] = i`` for a seen point, and for an unseen point the index of the
    seen point with the smallest fp32 squared distance ``((dx*dx + dy*dy) + dz*dz)`` (each operation rounded on its own,
    ties to the lowest index): the KeOps ``argmin`` of the reference's eval forward
    (models/segmentation/multimodal/no3d.py:119-122), mapped back to the numbering of ``pos``.  With no seen point
    ``src[i] = i`` everywhere and ``any_seen`` is False.  ``pos`` fp32 [N, 3], ``seen`` bool or uint8 [N].

    As in the reference the whole batch is ONE cloud: a point may take its neighbour from another sample of the batch.
    The mask is never compacted and the number of seen points is never read back.  The search is exact for any
    ``cell`` (it affects time only); with ``cell=None`` the extent of ``pos`` is read once to size it (the only host
    read), with a ``cell`` there is none.  Bitwise reproducible."""
    src, any_seen, _ = _nearest_seen("nearest_seen", pos, seen, None, cell)
    return src, any_seen


def fill_unseen(x, pos, seen, cell=None):
    """``(filled [N, K] in x.dtype, any_seen bool [1])`` with ``filled[i] = x[src[i]]`` for ``src`` of ``nearest_seen``:
    every unseen point takes the row of its nearest seen point (reference no3d.py:105-125), the rows copied as bits in
    the launch that finishes the search.  ``x`` [N, K] float32, bfloat16 or float16.  With no seen point ``filled``
    equals ``x``.  The whole batch is one cloud, as in the reference (no ``batch=``).  NOT differentiable: the
    reference applies it in eval mode only, ``x`` is detached.  Host reads as for ``nearest_seen``."""
    if not torch.is_tensor(x):
        raise TypeError("ops.fill_unseen takes tensors")
    _, any_seen, filled = _nearest_seen("fill_unseen", pos, seen, x, cell)
    return filled, any_seen


class _ViewNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, row_idx, labels, csr_idx, weight, ignore_index):
        lib = _lib.load()
        x = rows.detach().contiguous()
        R, K = x.shape
        dev = x.device
        V = R if row_idx is None else int(row_idx.shape[0])
        N = int(labels.shape[0])
        cnt = torch.empty((R, K), dtype=torch.int32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        numden = torch.empty(2, dtype=torch.float64, device=dev)
        ws, nbytes = _lib.workspace("dva_view_nll_workspace_bytes", dev)
        with _timed("view_nll_fwd", V * 4 + N * 16 + R * K * (8 + x.element_size())):
            check(lib.dva_view_nll_counts(ptr(row_idx), V, ptr(csr_idx), ptr(labels), N, int(ignore_index), R, K, ptr(cnt),
                                          stream_of(x)), "dva_view_nll_counts")
            check(lib.dva_view_nll_fwd(ptr(x), dtype_code(x), ptr(cnt), ptr(weight), R, K, ptr(loss), ptr(numden), ptr(ws),
                                       nbytes, stream_of(x)), "dva_view_nll_fwd")
        ctx.save_for_backward(x, cnt, weight, numden)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        x, cnt, weight, numden = ctx.saved_tensors
        lib = _lib.load()
        R, K = x.shape
        g_loss = g_loss.to(torch.float32).reshape(1).contiguous()
        out = torch.empty_like(x)
        with _timed("view_nll_bwd", R * K * (4 + 2 * x.element_size())):
            check(lib.dva_view_nll_bwd(ptr(x), dtype_code(x), ptr(cnt), ptr(weight), ptr(numden), ptr(g_loss), R, K,
                                       ptr(out), stream_of(x)), "dva_view_nll_bwd")
        return out, None, None, None, None, None


def view_nll(x_view, labels, csr_idx, weight=None, ignore_index=-1):
    """The view-level loss of the image-only models (reference no3d.py:145-154):
    ``F.nll_loss(F.log_softmax(x_view, -1), labels.repeat_interleave(csr_idx[1:] - csr_idx[:-1]), weight, ignore_index)``
    up to summation order, as a float32 scalar, without the [V, K] tensor and without the repeated labels.

    ``x_view`` is a ``GatheredFeatures`` (the lazy gather of an exact mapping, the identity gather that
    an atomic ``gather_segment_reduce`` returns, or a ``GatheredFeatures.cat``) or a plain [V, K] tensor (rows under the identity
    index); rows float32, bfloat16 or float16, upcast exactly, 1 <= K <= 64.  ``labels`` integer [N], ``csr_idx`` int64
    [N + 1].  Every view of a map row has that row's log-softmax, so the loss is a function of the per-row label
    counts (exact integers): ``sum w[y_v] (-logp_v[y_v]) / sum w[y_v]`` over the views whose point's label is not
    ``ignore_index``; a label outside [0, K) takes no part; NaN when no view takes part, as torch.  Reduced in float64
    in a fixed order: bitwise reproducible.  The gradient flows to the rows only, in their dtype.  No host
    synchronisation."""
    if isinstance(x_view, GatheredFeatures):
        rows, row_idx = x_view.rows, x_view.row_idx
    elif torch.is_tensor(x_view):
        rows, row_idx = x_view, None
    else:
        raise TypeError(f"ops.view_nll takes a GatheredFeatures or a [V, K] tensor, got {type(x_view).__name__}")
    if not torch.is_tensor(labels) or not torch.is_tensor(csr_idx):
        raise TypeError("ops.view_nll takes tensors")
    require_device(rows, row_idx, labels, csr_idx, weight)
    if rows.dtype not in _SEG_DTYPES:
        raise TypeError(f"ops.view_nll: rows of dtype {rows.dtype}; supported: {', '.join(str(d) for d in _SEG_DTYPES)}")
    if rows.dim() != 2:
        raise ValueError(f"ops.view_nll: the rows must be [R, K], got {tuple(rows.shape)}")
    R, K = int(rows.shape[0]), int(rows.shape[1])
    if not 1 <= K <= SEG_MAX_CLASSES:
        raise ValueError(f"ops.view_nll: K = {K} classes; the kernels take 1 <= K <= {SEG_MAX_CLASSES}")
    if R * K >= 1 << 31:
        raise ValueError(f"ops.view_nll: R * K = {R} * {K} elements; the kernels take fewer than 2^31")
    if labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise TypeError(f"ops.view_nll: labels must be integers [N], got {labels.dtype} {tuple(labels.shape)}")
    csr_idx = _check_ptr(csr_idx)
    if csr_idx.shape[0] != labels.shape[0] + 1:
        raise ValueError(f"ops.view_nll: csr_idx must be [N + 1] = [{labels.shape[0] + 1}], got {tuple(csr_idx.shape)}")
    if row_idx is not None:
        row_idx = row_idx.detach().to(torch.int32).contiguous()
    if weight is not None:
        if weight.dim() != 1 or weight.shape[0] != K:
            raise ValueError(f"ops.view_nll: weight must be [K] = [{K}], got {tuple(weight.shape)}")
        weight = weight.detach().to(torch.float32).contiguous()
    return _ViewNLL.apply(rows, row_idx, labels.detach().to(torch.int64).contiguous(), csr_idx, weight,
                          int(ignore_index))


class _LovaszSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, probas, labels, class_mask, present_only, ignore):
        lib = _lib.load()
        p = probas.detach().contiguous()
        P, C = p.shape
        dev = p.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        grad = torch.empty((P, C), dtype=torch.float32, device=dev)
        ws, nbytes = _lib.workspace("dva_lovasz_workspace_bytes", dev, P, C)
        with _timed("lovasz_softmax", p.numel() * 32):
            check(lib.dva_lovasz_softmax(ptr(p), ptr(labels), P, C, 0 if ignore is None else int(ignore),
                                         0 if ignore is None else 1, ptr(class_mask), int(bool(present_only)), ptr(loss),
                                         ptr(grad), ptr(ws), int(nbytes), stream_of(p)), "dva_lovasz_softmax")
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return grad * g, None, None, None, None      # the Jaccard increments are the gradient: backward is a scale


def lovasz_softmax_flat(probas, labels, classes="present", ignore=None):
    """The reference's ``lovasz_softmax_flat(*flatten_probas(probas, labels, ignore), classes=classes)`` for ``probas``
    float32 [P, C] (any values) and ``labels`` [P]: a float32 scalar with a gradient to ``probas``.

    ``classes``: ``'present'`` (classes some non-ignored point carries), ``'all'``, or a list of class numbers.  Per class
    the errors ``|fg - p_c|`` (float32, as the reference forms them) are sorted descending -- ties in ascending point
    order, where torch's sort leaves them unspecified -- and the Jaccard values come from integer counts in float64, so
    the gradient keeps its precision at any P (the reference differences two float32 values close to 1).  The loss is
    the mean over the classes taking part; 0, with a zero gradient, when there is none (every point ignored, an empty
    list): the shape quirks of the reference for that case live in ``deepviewagg_amd.metrics.lovasz_loss``.  All sizes
    are static: ignored points are sorted into a sentinel segment, nothing is read back.  1 <= C <= 64, P C < 2^31."""
    P, C, lab = _seg_inputs("lovasz_softmax_flat", probas, labels, (torch.float32,))
    mask = None
    if isinstance(classes, str):
        if classes not in ("present", "all"):
            raise ValueError(f"ops.lovasz_softmax_flat: classes must be 'present', 'all' or a list, got {classes!r}")
    else:
        wanted = sorted({int(c) for c in classes})
        if any(c < 0 or c >= C for c in wanted):
            raise IndexError(f"ops.lovasz_softmax_flat: classes {wanted} for C = {C}")
        mask = torch.zeros(C, dtype=torch.uint8, device=probas.device)
        for c in wanted:                                     # fills, no host-to-device copy (which would synchronise)
            mask[c:c + 1].fill_(1)
    if P == 0:
        return probas.sum() * 0.
    return _LovaszSoftmax.apply(probas, lab, mask, classes == "present" if isinstance(classes, str) else False, ignore)


def confusion_counts(outputs, labels, num_classes, ignore_index=-1, out=None):
    """Adds the confusion counts of ``outputs`` [P, C] (float32, bfloat16 or float16 scores of any kind) against
    ``labels`` [P] into ``out`` int64 [C, C] (row = label, column = ``argmax`` as numpy's: first maximum, a NaN is the
    maximum); a new zero matrix when ``out`` is None.  Rows whose label is ``ignore_index`` are skipped; rows with
    another label outside [0, C) are counted in ``n_bad`` instead.  Returns ``(counts, n_bad)``, int64 [C, C] and int64
    [1], both on the device; no host synchronisation.  Replaces the full device-to-host copy of the outputs in
    ``SegmentationTracker._compute_metrics``."""
    P, C, lab = _seg_inputs("confusion_counts", outputs, labels, _SEG_DTYPES)
    if int(num_classes) != C:
        raise ValueError(f"ops.confusion_counts: outputs have {C} columns for num_classes = {num_classes}")
    dev = outputs.device
    if out is None:
        out = torch.zeros((C, C), dtype=torch.int64, device=dev)
    else:
        require_device(outputs, out)
        if out.dtype != torch.int64 or tuple(out.shape) != (C, C) or not out.is_contiguous():
            raise ValueError(f"ops.confusion_counts: out must be a contiguous int64 [{C}, {C}] tensor")
    n_bad = torch.zeros(1, dtype=torch.int64, device=dev)
    x = outputs.detach().contiguous()
    lib = _lib.load()
    with _timed("confusion_counts", x.numel() * x.element_size()):
        check(lib.dva_confusion_counts(ptr(x), dtype_code(x), ptr(lab), int(ignore_index), P, C, ptr(out), ptr(n_bad),
                                       stream_of(x)), "dva_confusion_counts")
    return out, n_bad


# ---------------------------------------------------------------------------------------------
# voting on the raw cloud and K-NN interpolation of the votes (csrc/vote.hip)
# ---------------------------------------------------------------------------------------------

KNN_INTERPOLATE_CHUNK = 1 << 22     # queries per K-NN call: bounds the K-NN workspace and the [chunk, k] tables


def vote_slots(num_points, device):
    """The int32 slot array ``vote_add`` works in (one slot per raw point, all -1): created once per accumulator."""
    nbytes = _lib.workspace_bytes("dva_vote_workspace_bytes", int(num_points))
    return torch.full((nbytes // 4,), -1, dtype=torch.int32, device=device)


def vote_add(votes, counts, ids, outputs, slots):
    """``votes[ids] += outputs; counts[ids] += 1`` in place on the device, for ``votes`` float32 [N, C], ``counts`` int32
    [N], ``ids`` [P] (integers) and ``outputs`` [P, C] (float32, bfloat16 or float16; widened exactly).  An id that
    occurs several times in ``ids`` is counted once, as in the reference, and it is always the LAST occurrence (torch
    leaves open which one).  ``slots`` comes from ``vote_slots(N, device)`` and reads all -1 before and after the call.
    An id outside [0, N) writes nothing and is counted in the returned ``n_bad`` (int64 [1], on the device).  No float
    atomics, so two runs give the same bits; no host synchronisation.  1 <= C <= 64."""
    for t in (votes, counts, ids, outputs, slots):
        if not torch.is_tensor(t):
            raise TypeError("ops.vote_add takes tensors")
    dev = require_device(votes, counts, ids, outputs, slots)
    if votes.dim() != 2 or votes.dtype != torch.float32 or not votes.is_contiguous():
        raise ValueError("ops.vote_add: votes must be a contiguous float32 [N, C] tensor")
    N, C = int(votes.shape[0]), int(votes.shape[1])
    if counts.dtype != torch.int32 or tuple(counts.shape) != (N,) or not counts.is_contiguous():
        raise ValueError(f"ops.vote_add: counts must be a contiguous int32 [{N}] tensor")
    if slots.dtype != torch.int32 or slots.dim() != 1 or not slots.is_contiguous():
        raise ValueError("ops.vote_add: slots must come from ops.vote_slots")
    if not 1 <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"ops.vote_add: C = {C} classes; the kernels take 1 <= C <= {SEG_MAX_CLASSES}")
    if ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise TypeError(f"ops.vote_add: ids must be integers, got {ids.dtype}")
    if outputs.dtype not in _SEG_DTYPES:
        raise TypeError(f"ops.vote_add: outputs of dtype {outputs.dtype}; supported: float32, bfloat16, float16")
    ids = ids.detach().reshape(-1).to(torch.int64).contiguous()
    P = int(ids.shape[0])
    if tuple(outputs.shape) != (P, C):
        raise ValueError(f"ops.vote_add: outputs must be [P, C] = [{P}, {C}], got {tuple(outputs.shape)}")
    out = outputs.detach().contiguous()
    n_bad = torch.zeros(1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    with _timed("vote_add", P * (16 + C * (out.element_size() + 8))):
        check(lib.dva_vote_add(ptr(votes), ptr(counts), N, C, ptr(ids), ptr(out), dtype_code(out), P, ptr(slots),
                               int(slots.numel()) * 4, ptr(n_bad), stream_of(votes)), "dva_vote_add")
    return n_bad


def _interpolate_inputs(what, x, pos_x, pos_y, k):
    for t in (x, pos_x, pos_y):
        if not torch.is_tensor(t):
            raise TypeError(f"ops.{what} takes tensors")
    require_device(x, pos_x, pos_y)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"ops.{what}: x must be float32 [M, C], got {x.dtype} {tuple(x.shape)}")
    M, C = int(x.shape[0]), int(x.shape[1])
    if pos_x.dim() != 2 or tuple(pos_x.shape) != (M, 3) or pos_y.dim() != 2 or pos_y.shape[1] != 3:
        raise ValueError(f"ops.{what}: pos_x must be [M, 3] = [{M}, 3] and pos_y [n, 3], got {tuple(pos_x.shape)} and "
                         f"{tuple(pos_y.shape)}")
    if not 1 <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"ops.{what}: C = {C} columns; the kernel takes 1 <= C <= {SEG_MAX_CLASSES}")
    if not isinstance(k, int) or isinstance(k, bool) or not 0 < k <= 128:
        raise ValueError(f"ops.{what}: k = {k!r}; the K-NN keeps 1 <= k <= 128 neighbours")
    if k > M:
        raise ValueError(f"ops.{what}: k = {k} neighbours requested from {M} points")
    return (x.detach().contiguous(), pos_x.detach().float().contiguous(), pos_y.detach().float().contiguous(), M, C,
            int(pos_y.shape[0]))


def _interpolate_chunks(x, pos_x, pos_y, k, chunk, own, y, pred, labels, ignore_index, counts, n_bad):
    """One K-NN and one interpolation launch per chunk of queries; every output is written in place."""
    lib = _lib.load()
    M, C = x.shape
    n = int(pos_y.shape[0])
    chunk = KNN_INTERPOLATE_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError(f"ops.knn_interpolate: chunk = {chunk}")
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        nbr, d2 = knn_query(pos_y[a:b], pos_x, k)
        with _timed("knn_interpolate", (b - a) * (k * (8 + 4 * C) + 8)):
            check(lib.dva_knn_interpolate(ptr(x), M, C, ptr(nbr), ptr(d2), b - a, k,
                                          None if own is None else ptr(own[a:b]), None if y is None else ptr(y[a:b]),
                                          None if pred is None else ptr(pred[a:b]),
                                          None if labels is None else ptr(labels[a:b]), int(ignore_index), ptr(counts),
                                          ptr(n_bad), stream_of(x)), "dva_knn_interpolate")


def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3, chunk=None):
    """``torch_geometric.nn.unpool.knn_interpolate(x, pos_x, pos_y, k=k)``: ``y`` float32 [n, C], per query the mean of
    the rows of ``x`` float32 [M, C] at its k nearest points of ``pos_x`` [M, 3], weighted by ``1 / max(d2, 1e-16)``.
    All in float32, every operation rounded on its own, summed in neighbour rank order (``ops.knn_query``: ascending by
    (float32 squared distance, index); torch_cluster's tie order is not defined).  The queries are processed in
    chunks of ``chunk`` (default 2^22) so that the K-NN's tables stay bounded; the result does not depend on it.
    ``batch_x`` / ``batch_y`` are not supported.  The K-NN reads one scalar back per chunk."""
    if batch_x is not None or batch_y is not None:
        raise NotImplementedError("ops.knn_interpolate: batch_x / batch_y are not supported (one cloud per call)")
    x, pos_x, pos_y, M, C, n = _interpolate_inputs("knn_interpolate", x, pos_x, pos_y, k)
    y = torch.empty((n, C), dtype=torch.float32, device=x.device)
    _interpolate_chunks(x, pos_x, pos_y, k, chunk, None, y, None, None, 0, None, None)
    return y


def knn_interpolate_labels(x, pos_x, pos_y, k=1, labels=None, num_classes=None, ignore_index=-1, out=None,
                           keep_counts=None, chunk=None):
    """``knn_interpolate(x, pos_x, pos_y, k=k).argmax(1)`` without the [n, C] tensor: returns ``(pred, counts, n_bad)``.

    ``pred`` int64 [n] is the first maximum of the interpolated row (a NaN is the maximum, as ``ops.confusion_counts``).
    With ``labels`` [n], the pairs ``(labels[i], pred[i])`` whose label is not ``ignore_index`` are added to ``counts``
    int64 [C, C] (``out``, or a new zero matrix) and a label outside [0, C) is counted in ``n_bad`` int64 [1] instead;
    without ``labels`` both are None.  ``keep_counts`` [n] (integers) serves KITTI-360's fill: the queries with a
    positive entry are, in their order, the M points ``x`` and ``pos_x`` were taken from (``x = votes[keep_counts > 0]``),
    and each of them keeps the ``argmax`` of its own row; only the others are interpolated.  Everything stays on the
    device; the K-NN reads one scalar back per chunk of ``chunk`` queries (default 2^22)."""
    x, pos_x, pos_y, M, C, n = _interpolate_inputs("knn_interpolate_labels", x, pos_x, pos_y, k)
    dev = x.device
    if num_classes is not None and int(num_classes) != C:
        raise ValueError(f"ops.knn_interpolate_labels: x has {C} columns for num_classes = {num_classes}")
    counts = n_bad = lab = None
    if labels is not None:
        require_device(x, labels)
        if labels.dim() != 1 or labels.shape[0] != n:
            raise ValueError(f"ops.knn_interpolate_labels: labels must be [n] = [{n}], got {tuple(labels.shape)}")
        if labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise TypeError(f"ops.knn_interpolate_labels: labels must be integers, got {labels.dtype}")
        lab = labels.detach().to(torch.int64).contiguous()
        if out is None:
            out = torch.zeros((C, C), dtype=torch.int64, device=dev)
        else:
            require_device(x, out)
            if out.dtype != torch.int64 or tuple(out.shape) != (C, C) or not out.is_contiguous():
                raise ValueError(f"ops.knn_interpolate_labels: out must be a contiguous int64 [{C}, {C}] tensor")
        counts = out
        n_bad = torch.zeros(1, dtype=torch.int64, device=dev)
    elif out is not None:
        raise ValueError("ops.knn_interpolate_labels: out without labels")
    own = None
    if keep_counts is not None:
        require_device(x, keep_counts)
        if keep_counts.dim() != 1 or keep_counts.shape[0] != n:
            raise ValueError(f"ops.knn_interpolate_labels: keep_counts must be [n] = [{n}]")
        kept = keep_counts > 0
        own = torch.where(kept, torch.cumsum(kept, 0, dtype=torch.int32) - 1, -1).to(torch.int32).contiguous()
    pred = torch.empty(n, dtype=torch.int64, device=dev)
    _interpolate_chunks(x, pos_x, pos_y, k, chunk, own, None, pred, lab, ignore_index, counts, n_bad)
    return pred, counts, n_bad
