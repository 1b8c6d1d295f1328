"""The sparse convolution of a channel concatenation that is never written, on the GPU: ``ops.sparse_conv`` /
``ops.sparse_conv_fused`` on a list of feature tensors (C ABI ``dva_sparse_conv_apply_parts`` / ``_apply_packed_parts`` /
``_wgrad_parts``), the lazy ``snn.cat`` and its consumers (``Conv3d``, ``FoldedConv``, ``ResNetUp``, the concatenation
fusion of ``UnimodalBranch``).

What is held to what:
* part widths that are multiples of 16: output and input gradient have the BITS of the call on ``torch.cat(parts, 1)``
  (the kernel walks the same 16-channel steps in the same order), every part's gradient is its column range; the weight
  gradient is summed with fp32 atomics on both routes and goes through the row gates of tests/sparse_rows.py;
* ragged widths (a part is padded to 16 on its own): the row gates of tests/sparse_rows.py against the float64 yardsticks
  on ``torch.cat``.  fp32 ``out`` / ``grad_x`` are gated with the noise of the float32 evaluation in the kernel's
  accumulation order (``SR.gate_kernel_order``: the gate every stratum of the single-tensor convolution meets; the plain
  gate has the open findings listed in tests/test_gpu_sparseconv.py, which are about that order and not about parts) and
  with the kept whole-tensor statement, 2e-5 of exact float64;
* modules: the switch on against off, through the float64 CPU twin where a gate needs a yardstick (the rules of
  tests/test_gpu_sparse_fold.py: fp32 within max(1e-4 of the scale, 3 x the CPU float32 error); bf16 no more than 2 x the
  error of the materialised route, floored at half a bf16 ulp of the largest value, 2^-8 of the scale).
"""
import contextlib
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, t
from oracle import sparseconv_oracle as O

sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure          # noqa: E402
import sparse_rows as SR    # noqa: E402
from tolerances import Report   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
ALL_STRATA = ("nbr_1", "nbr_2_8", "nbr_9_26", "nbr_27", "tile_edge", "last_tile", "wave_skips", "wave_no_skip")

# kernel size, stride, transposed
FORMS = {"k3s1": (3, 1, False), "k2s2": (2, 2, False), "k3s2": (3, 2, False), "k2s2T": (2, 2, True),
         "k3s2T": (3, 2, True)}
CLOUDS = ("map1", "map63", "map64", "map65", "map129", "strata1500")
# part widths -> output channels: a ragged 64-wide output tile, the 128-wide tile (NT = 4), one full 64-wide tile
ALIGNED = {(16, 32): 48, (64, 64): 128, (16, 16, 32, 64): 64}


def _bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == F32 else torch.int16)


def _tag(dtype):
    return "fp32" if dtype == F32 else "bf16"


@functools.lru_cache(maxsize=None)
def _cloud(name):
    if name.startswith("map"):
        return SR.map_cloud(int(name[3:]), seed=int(name[3:]))[0].contiguous()
    return SR.strata_cloud(1, int(name[6:]))


@functools.lru_cache(maxsize=None)
def _device_maps(cloud, form):
    """(nbr [K, n_dst], nbr_t [K, n_src]) on the device, as Conv3d._maps hands them to ops.sparse_conv."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d.nn import downsample_coords, kernel_offsets
    k, stride, transpose = FORMS[form]
    c = _cloud(cloud).to(DEV)
    dst = c if stride == 1 else downsample_coords(c, stride)
    offs = kernel_offsets(k, 1)
    nbr, nbr_t = ops.voxel_kernel_map(c, dst, offs), ops.voxel_kernel_map(dst, c, -offs)
    return (nbr_t, nbr) if transpose else (nbr, nbr_t)


def _split(x, widths):
    out, a = [], 0
    for w in widths:
        out.append(x[:, a:a + w].contiguous())
        a += w
    return out


def _run(x, W, b, g, nbr, nbr_t, widths=None):
    """(out, grad x, grad W, grad bias) of ops.sparse_conv on the device; ``widths``: x goes in as that list of parts
    (grad x is then the list of the parts' gradients)."""
    from deepviewagg_amd import ops
    Wd = W.to(DEV).requires_grad_(True)
    bd = None if b is None else b.to(DEV).requires_grad_(True)
    if widths is None:
        xd = x.to(DEV).requires_grad_(True)
        out = ops.sparse_conv(xd, Wd, bd, nbr, nbr_t)
    else:
        xd = [p.to(DEV).requires_grad_(True) for p in _split(x, widths)]
        out = ops.sparse_conv(xd, Wd, bd, nbr, nbr_t)
    out.backward(g.to(DEV))
    gx = xd.grad if widths is None else [p.grad for p in xd]
    return out.detach(), gx, Wd.grad, None if bd is None else bd.grad


# ---- bit identity where it must hold -------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("cloud", CLOUDS)
def test_aligned_parts_give_the_bits_of_the_concatenation(cloud, form, dtype):
    """Widths (16, 32), (64, 64), (16, 16, 32, 64), with and without bias: out and grad x equal the materialised route
    with ``torch.equal`` on the bit patterns; each part's gradient is the matching column range, in the part's dtype."""
    nbr, nbr_t = _device_maps(cloud, form)
    K, n_dst, n_src = nbr.shape[0], nbr.shape[1], nbr_t.shape[1]
    assert K == FORMS[form][0] ** 3 and n_src >= 1 and n_dst >= 1
    for widths, cout in ALIGNED.items():
        for bias in (False, True):
            gen = torch.Generator().manual_seed(n_src + 7 * cout + bias)
            cin = sum(widths)
            x = torch.randn(n_src, cin, generator=gen).to(dtype)
            W = torch.randn(K, cin, cout, generator=gen) / np.sqrt(cin * K / 4)
            b = torch.randn(cout, generator=gen) if bias else None
            g = torch.randn(n_dst, cout, generator=gen).to(dtype)
            out_c, gx_c, gW_c, gb_c = _run(x, W, b, g, nbr, nbr_t)
            out_p, gx_p, gW_p, gb_p = _run(x, W, b, g, nbr, nbr_t, widths)
            what = f"{cloud} {form} {_tag(dtype)} {widths} bias={bias}"
            assert out_p.dtype == dtype and out_p.shape == (n_dst, cout), what
            assert torch.equal(_bits(out_p), _bits(out_c)), f"{what}: out"
            a = 0
            for w, gp in zip(widths, gx_p):
                assert gp.dtype == dtype and gp.shape == (n_src, w), what
                assert torch.equal(_bits(gp), _bits(gx_c[:, a:a + w])), f"{what}: grad of the part at column {a}"
                a += w
            assert gW_p.shape == W.shape and gW_p.dtype == F32, what
            if bias:
                assert torch.equal(gb_p, gb_c), what
            # the weight gradient: fp32 atomics on both routes add the same <= 256 per-wavefront partial sums per element
            # in an order that is not fixed: 256 x 2^-24 of the largest sum, rounded up to 1e-5; its row gate is below
            scale = float(gW_c.abs().max()) + 1e-30
            assert float((gW_p - gW_c).abs().max()) <= 1e-5 * scale, f"{what}: grad W"


@functools.lru_cache(maxsize=None)
def _case(name, cloud, widths, cout, form, bias, dtype):
    k, stride, transpose = FORMS[form]
    return SR.conv_case(f"parts {name} {_tag(dtype)}", _cloud(cloud), sum(widths), cout, k=k, stride=stride, bias=bias,
                        transpose=transpose, dtype=dtype, seed=len(name) + sum(widths))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("widths", sorted(ALIGNED), ids=lambda w: "_".join(map(str, w)))
def test_aligned_parts_weight_gradient_meets_the_row_gate(widths, form, dtype):
    """The strata cloud, every form: grad W (fp32 atomics, so no equality) and grad bias through ``SR.gate_case``; out
    and grad x are the bits of the materialised route once more, here on the tensors of the case."""
    cout = ALIGNED[widths]
    name = f"{form}_{'_'.join(map(str, widths))}_{cout}"
    c = _case(name, "strata1500", widths, cout, form, True, dtype)
    nbr, nbr_t = _device_maps("strata1500", form)
    assert torch.equal(nbr.cpu(), c["nbr"]) and torch.equal(nbr_t.cpu(), c["nbr_t"])
    out_p, gx_p, gW_p, gb_p = _run(c["x"], c["W"], c["b"], c["g"], nbr, nbr_t, widths)
    out_c, gx_c, _, _ = _run(c["x"], c["W"], c["b"], c["g"], nbr, nbr_t)
    assert torch.equal(_bits(out_p), _bits(out_c)) and torch.equal(_bits(torch.cat(gx_p, 1)), _bits(gx_c))
    rep = Report(f"sparse convolution in parts: {c['name']}")
    SR.gate_case(rep, c, gW=gW_p, gb=gb_p)
    rep.check()


# ---- ragged widths ---------------------------------------------------------------------------------------------------

# name -> (cloud, part widths, Cout, strata every tensor must fill)
RAGGED = {"r_4_64": ("strata1500", (4, 64), 48, ALL_STRATA),
          "r_5_7_20": ("strata1500", (5, 7, 20), 7, ALL_STRATA),
          "r_4_512": ("strata600", (4, 512), 128, ())}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(RAGGED))
def test_ragged_parts_meet_the_row_gates(name, dtype):
    """Parts that are padded to 16 each on their own: out, the per-part input gradients, dW and db against the float64
    yardsticks on ``torch.cat`` (see the module docstring for the fp32 noise); dW comes back without the padding rows."""
    cloud, widths, cout, require = RAGGED[name]
    c = _case(name, cloud, widths, cout, "k3s1", True, dtype)
    nbr, nbr_t = _device_maps(cloud, "k3s1")
    assert torch.equal(nbr.cpu(), c["nbr"]) and torch.equal(nbr_t.cpu(), c["nbr_t"])
    out, gx_parts, gW, gb = _run(c["x"], c["W"], c["b"], c["g"], nbr, nbr_t, widths)
    n = c["src"].shape[0]
    assert out.dtype == dtype and out.shape == (n, cout)
    assert [tuple(p.shape) for p in gx_parts] == [(n, w) for w in widths] and all(p.dtype == dtype for p in gx_parts)
    assert gW.shape == (27, sum(widths), cout) and gW.dtype == F32 and gb.shape == (cout,)    # padding rows cut
    gx = torch.cat(gx_parts, 1)
    rep = Report(f"sparse convolution in ragged parts: {c['name']}")
    if dtype == F32:
        for tensor, a in (("out", out), ("gx", gx), ("gW", gW), ("gb", gb)):
            err = SR.old_metric(a.reshape(c["exact"][tensor].shape), c["exact"][tensor])
            print(f"{c['name']} {tensor}: {err:.3e} of the scale against exact float64")
            assert err <= 2e-5, f"{c['name']} {tensor}: {err:.3e}"
        masks = SR.conv_strata(c["nbr"], require=require), SR.conv_strata(c["nbr_t"], require=require)
        assert masks
        SR.gate_kernel_order(rep, c, out, gx)
        SR.gate_case(rep, c, gW=gW, gb=gb)
    else:
        SR.gate_case(rep, c, out=out, gx=gx, gW=gW, gb=gb, require=require, require_t=require)
    rep.check()


def test_mixed_dtypes_under_autocast_and_a_list_of_one():
    """autocast(bfloat16): parts (fp32 [n, 4], bf16 [n, 64]) give the bf16 output of the all-bf16 parts (each part is cast
    on its own; the bf16 part is used as it is) and every part its gradient in its own dtype; a list of one is the tensor
    call, bit for bit, with and without autocast."""
    from deepviewagg_amd import ops
    nbr, nbr_t = _device_maps("strata1500", "k3s1")
    n = nbr.shape[1]
    gen = torch.Generator().manual_seed(3)
    a32 = torch.randn(n, 4, generator=gen).to(DEV)
    b16 = torch.randn(n, 64, generator=gen).to(DEV).bfloat16()
    W = (torch.randn(27, 68, 48, generator=gen) / np.sqrt(68 * 27 / 4)).to(DEV).requires_grad_(True)
    bias = torch.randn(48, generator=gen).to(DEV)
    g = torch.randn(n, 48, generator=gen).to(DEV).bfloat16()
    pa, pb = a32.clone().requires_grad_(True), b16.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16):
        mixed = ops.sparse_conv([pa, pb], W, bias, nbr, nbr_t)
        same = ops.sparse_conv([a32.bfloat16(), b16], W, bias, nbr, nbr_t)
        cat = ops.sparse_conv(torch.cat([a32, b16.float()], 1), W, bias, nbr, nbr_t)
    assert mixed.dtype == BF16 and torch.equal(_bits(mixed), _bits(same.detach()))
    scale = float(cat.detach().float().abs().max())
    assert float((mixed.detach().float() - cat.detach().float()).abs().max()) <= 2 ** -8 * scale      # half a bf16 ulp of the largest value
    mixed.backward(g)
    assert pa.grad.dtype == F32 and pa.grad.shape == (n, 4) and pb.grad.dtype == BF16 and pb.grad.shape == (n, 64)
    assert W.grad.shape == W.shape and float(pa.grad.abs().sum()) > 0 and float(pb.grad.float().abs().sum()) > 0
    # without autocast the parts are promoted as torch.cat promotes them: fp32
    assert ops.sparse_conv([a32, b16], W, bias, nbr, nbr_t).dtype == F32
    for amp in (contextlib.nullcontext(), torch.autocast("cuda", dtype=BF16)):
        for x in (b16, b16.float()):
            with amp:
                one, plain = ops.sparse_conv([x], W[:, 4:], bias, nbr, nbr_t), ops.sparse_conv(x, W[:, 4:], bias, nbr, nbr_t)
            assert one.dtype == plain.dtype and torch.equal(_bits(one.detach()), _bits(plain.detach()))
    with pytest.raises(ValueError):
        ops.sparse_conv([b16] * 5, W, bias, nbr, nbr_t)


# ---- fused inference -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("widths,cout", [((16, 32), 48), ((64, 64), 128), ((16, 16, 32, 64), 64), ((4, 64), 48),
                                         ((5, 7, 20), 7)], ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else None)
def test_fused_inference_on_parts(widths, cout, dtype):
    """``sparse_conv_fused(parts, pack(W, dtype, parts=widths), ...)`` against the call on the concatenation: equal bits
    for 16-multiple widths; otherwise the rule of tests/test_gpu_sparse_fold.py -- fp32: the bits of the torch expression
    of the epilogue on the unfused parts convolution, and 2e-5 of the scale against the concatenated route (both are
    within 1e-5 of exact); bf16: within 2^-8 of the largest value of the float64 oracle on the bf16 operands."""
    from deepviewagg_amd import ops
    nbr, nbr_t = _device_maps("strata1500", "k3s1")
    n, cin = nbr.shape[1], sum(widths)
    gen = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(n, cin, generator=gen).to(dtype)
    W = torch.randn(27, cin, cout, generator=gen) / np.sqrt(cin * 27 / 4)
    b = torch.randn(cout, generator=gen)
    res = torch.randn(n, cout, generator=gen).to(dtype)
    slope = 0.2
    parts = [p.to(DEV) for p in _split(x, widths)]
    Wd, bd, rd = W.to(DEV), b.to(DEV), res.to(DEV)
    packed = ops.sparse_conv_pack(Wd, dtype, parts=widths)
    assert packed.parts == tuple(widths) and packed.cin == cin and packed.cin_p == sum((w + 15) // 16 * 16 for w in widths)
    whole = ops.sparse_conv_pack(Wd, dtype)
    with torch.no_grad():
        got = ops.sparse_conv_fused(parts, packed, bd, nbr, residual=rd, slope=slope)
        ref = ops.sparse_conv_fused(x.to(DEV), whole, bd, nbr, residual=rd, slope=slope)
        again = ops.sparse_conv_fused(tuple(parts), packed, bd, nbr, residual=rd, slope=slope)
    assert got.dtype == dtype and got.shape == (n, cout) and torch.equal(_bits(got), _bits(again))
    if all(w % 16 == 0 for w in widths):
        assert torch.equal(_bits(got), _bits(ref))
        with torch.no_grad():                                       # the same layout: one tensor may use that operand
            assert torch.equal(_bits(ops.sparse_conv_fused(x.to(DEV), packed, bd, nbr, residual=rd, slope=slope)), _bits(ref))
    elif dtype == F32:
        with torch.no_grad():
            o = ops.sparse_conv(parts, Wd, bd, nbr, nbr_t)
        expect = torch.where(o >= 0, o, slope * o) + rd
        assert torch.equal(_bits(got), _bits(expect))
        assert SR.old_metric(got, ref.cpu()) <= 2e-5
    else:
        y = O.sparse_conv(x.double(), W.bfloat16().double(), b.double(), nbr.cpu())
        y = torch.where(y >= 0, y, slope * y) + res.double()
        err, scale = float((got.cpu().double() - y).abs().max()), float(y.abs().max())
        print(f"fused parts {widths} bf16: max error {err:.3e}, gate {2 ** -8 * scale:.3e}")
        assert err <= 2 ** -8 * scale
    # mismatched widths raise, as does the one-tensor operand for parts and a ragged parts operand for one tensor
    with pytest.raises(ValueError):
        ops.sparse_conv_fused(parts[::-1] if len(set(widths)) > 1 else parts + parts[:1], packed, bd, nbr)
    with pytest.raises(ValueError):
        ops.sparse_conv_fused(parts, whole, bd, nbr)
    with pytest.raises(ValueError):
        ops.sparse_conv_pack(Wd, dtype, parts=widths[:-1])
    with pytest.raises(TypeError):
        ops.sparse_conv_pack(Wd, torch.float16, parts=widths)
    if any(w % 16 for w in widths):
        with pytest.raises(ValueError):
            ops.sparse_conv_fused(x.to(DEV), packed, bd, nbr)


# ---- modules ---------------------------------------------------------------------------------------------------------

def test_lazy_cat_on_the_device_is_the_cat_and_is_cached():
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    coords = _cloud("strata1500")[:300].to(DEV)
    a = snn.SparseVoxelTensor(torch.randn(300, 32, device=DEV), coords)
    b = a.like(torch.randn(300, 16, device=DEV).bfloat16())
    lazy = snn.cat(a, b, lazy=True)
    assert isinstance(lazy, snn.LazyCatTensor) and lazy._feats is None
    f = lazy.F
    assert torch.equal(f, torch.cat([a.F, b.F], 1)) and f.dtype == F32 and lazy.F is f


@pytest.mark.parametrize("amp", [None, BF16], ids=["fp32", "autocast_bf16"])
def test_1x1x1_on_parts_with_the_split_k_weight_gradient(amp):
    """``Conv3d(kernel_size=1)`` on a lazy tensor at 8401 rows (above the 8192-row threshold of the split-K product and
    no multiple of its 64 splits, so the remainder product runs too): output, both part gradients and the kernel gradient
    against float64 on the CPU -- fp32 by the rule of the twin test, bf16 no more than 2 x the materialised route, floored
    at 2^-8 of the scale."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    n = 8192 + 3 * 64 + 17
    gen = torch.Generator().manual_seed(9)
    coords = torch.cat([torch.arange(n).reshape(-1, 1), torch.zeros(n, 3, dtype=torch.long)], 1).int()
    fa, fb, g = torch.randn(n, 32, generator=gen), torch.randn(n, 16, generator=gen), torch.randn(n, 24, generator=gen)
    conv = snn.Conv3d(48, 24, kernel_size=1, bias=True)

    def run(dev, dt, lazy):
        c = copy.deepcopy(conv).to(dev).to(dt)
        a, b = (f.detach().clone().to(dev).to(dt).requires_grad_(True) for f in (fa, fb))
        ta = snn.SparseVoxelTensor(a, coords.to(dev))
        with (torch.autocast("cuda", dtype=amp) if amp and dev != "cpu" else contextlib.nullcontext()):
            y = c(snn.cat(ta, ta.like(b), lazy=lazy)).F
        y.backward(g.to(dev).to(y.dtype))
        return {"out": y.detach(), "grad a": a.grad, "grad b": b.grad, "grad kernel": c.kernel.grad, "grad bias": c.bias.grad}
    ref, cpu = run("cpu", torch.float64, False), run("cpu", F32, False)
    lz, mt = run(DEV, F32, True), run(DEV, F32, False)
    for what in ref:
        scale = float(ref[what].abs().max())
        e_l, e_m, e_32 = _err(lz[what], ref[what]), _err(mt[what], ref[what]), _err(cpu[what], ref[what])
        gate = max(1e-4 * scale, 3.0 * e_32) if amp is None else max(2.0 * e_m, 2 ** -8 * scale)
        print(f"1x1x1 on parts {'bf16' if amp else 'fp32'} {what}: lazy {e_l:.3e}, materialised {e_m:.3e}, gate {gate:.3e}")
        assert lz[what].shape == ref[what].shape and e_l <= gate, what


def _randomise_norms(module, seed):
    gen = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            c = m.num_features
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(c, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(c, generator=gen) * 1.5 + 0.5)
                m.weight.copy_((torch.rand(c, generator=gen) + 0.5) * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1))
                m.bias.copy_(torch.randn(c, generator=gen) * 0.3)
    return module


def _up_forward(up, down, feats, skip_first, dev, lazy, grads):
    """``up(down(x), skip)`` with the fixed strided ``down`` layer (it puts the k2s2 map into the caches the transposed
    convolution reads); the skip is the fine tensor, or a second coarse tensor when it is concatenated first."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    coords, fx, fskip = feats
    x = snn.SparseVoxelTensor(fx.to(dev), coords.to(dev))
    with torch.no_grad():
        coarse = down(x)
    if skip_first:
        skip = coarse.like(fskip[:coarse.F.shape[0]].to(dev))
    else:
        skip = x.like(fskip.to(dev))
    found = snn.LAZY_CAT
    snn.LAZY_CAT = lazy
    try:
        with torch.set_grad_enabled(grads):
            y = up(coarse.like(coarse.F.detach()), skip)
    finally:
        snn.LAZY_CAT = found
    if not grads:
        return y.F, None
    up.zero_grad()
    y.F.float().square().mean().backward()
    return y.F.detach(), {k: p.grad.clone() for k, p in up.named_parameters()}


@functools.lru_cache(maxsize=None)
def _up_case(skip_first):
    """The stage, its input and the CPU evaluations through the oracle (float32 and float64, training mode: batch
    statistics) with their parameter gradients, and the eval-mode float64 forward for the fold."""
    from deepviewagg_amd.modules.SparseConv3d import ResNetUp
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    coords = _cloud("strata1500")[:300].contiguous()
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(11)
    feats = (coords, torch.randn(300, 8, generator=gen), torch.randn(300, 16, generator=gen))
    down = snn.Conv3d(8, 32, kernel_size=2, stride=2).eval()
    up = ResNetUp(up_conv_nn=[48, 24] if skip_first else [32, 16, 24], N=1, skip_first=skip_first)
    _randomise_norms(up, 13)
    assert up.blocks[0].downsample is not None
    c = dict(feats=feats, down=down, up=up)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(snn, "ops", O.OracleOps)
        m.setattr(snn, "batchnorm_act_rows", O.batchnorm_act_rows)
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            u, d = copy.deepcopy(up).to(dt).train(), copy.deepcopy(down).to(dt)
            f = (coords, feats[1].to(dt), feats[2].to(dt))
            c["eval" + tag] = _up_forward(u.eval(), d, f, skip_first, "cpu", False, False)[0]    # before train() moves
            c["train" + tag] = _up_forward(u.train(), d, f, skip_first, "cpu", False, True)      # the running statistics
    return c


def _err(a, r):
    return float((a.detach().cpu().double() - r.double()).abs().max())


@pytest.mark.parametrize("skip_first", [False, True], ids=["skip_after", "skip_first"])
def test_resnet_up_with_the_switch_on_against_off(skip_first):
    """``ResNetUp`` (N = 1, a ResBlock with a ``downsample``), 300 voxels, training mode: same state-dict keys; outputs and
    every parameter gradient of both routes against the float64 CPU twin -- fp32 within max(1e-4 of the scale, 3 x the CPU
    float32 error); autocast(bfloat16): the lazy route no more than 2 x the materialised route's error, floored at 2^-8 of
    the scale."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    c = _up_case(skip_first)
    up, down = copy.deepcopy(c["up"]).to(DEV).train(), copy.deepcopy(c["down"]).to(DEV)
    keys = list(up.state_dict())
    ref_out, ref_g = c["train64"]
    cpu_out, cpu_g = c["train32"]
    assert set(ref_g) == {k for k, _ in up.named_parameters()}
    for amp in (None, BF16):
        ctx = torch.autocast("cuda", dtype=BF16) if amp else contextlib.nullcontext()
        with ctx:
            out_m, g_m = _up_forward(copy.deepcopy(up), down, c["feats"], skip_first, DEV, False, True)
            lazy_up = copy.deepcopy(up)
            with measure.launch_counter() as launches:
                out_l, g_l = _up_forward(lazy_up, down, c["feats"], skip_first, DEV, True, True)
        assert list(lazy_up.state_dict()) == keys and snn.LAZY_CAT is False
        assert any(name.startswith("sparse_conv_apply_parts") for name in launches.names)
        assert any(name.startswith("sparse_conv_wgrad_parts") for name in launches.names)
        assert out_l.shape == ref_out.shape and out_l.dtype == (BF16 if amp else F32)
        rows = [("out", out_l, out_m, cpu_out, ref_out)] + [(k, g_l[k], g_m[k], cpu_g[k], ref_g[k]) for k in sorted(ref_g)]
        for what, lz, mt, c32, ref in rows:
            scale = float(ref.abs().max()) + 1e-30
            e_l, e_m, e_32 = _err(lz, ref), _err(mt, ref), _err(c32, ref)
            gate = max(1e-4 * scale, 3.0 * e_32) if amp is None else max(2.0 * e_m, 2 ** -8 * scale)
            print(f"ResNetUp skip_first={skip_first} {'bf16' if amp else 'fp32'} {what}: lazy {e_l:.3e}, materialised "
                  f"{e_m:.3e}, cpu fp32 {e_32:.3e}, gate {gate:.3e}")
            assert e_l <= gate, f"{what}: lazy {e_l:.3e} vs gate {gate:.3e} (materialised {e_m:.3e})"


@pytest.mark.parametrize("skip_first", [False, True], ids=["skip_after", "skip_first"])
def test_folded_resnet_up_runs_on_the_lazy_tensor(skip_first):
    """``fold_for_inference`` of the stage on the lazy tensor: the packed operands are keyed by the part widths, the fp32
    output meets the fold test's gate against the float64 eval-mode twin, and the bf16 output rounds no more than 2 x the
    unfolded stage."""
    from deepviewagg_amd.modules.SparseConv3d import FoldedConv, fold_for_inference
    c = _up_case(skip_first)
    up, down = copy.deepcopy(c["up"]).to(DEV).eval(), copy.deepcopy(c["down"]).to(DEV)
    folded = fold_for_inference(up)
    ref, cpu = c["eval64"], c["eval32"]
    scale = float(ref.abs().max())
    with measure.launch_counter() as launches:
        out_l, _ = _up_forward(folded, down, c["feats"], skip_first, DEV, True, False)
    out_m, _ = _up_forward(folded, down, c["feats"], skip_first, DEV, False, False)
    assert any(name.startswith("sparse_conv_fused_parts") for name in launches.names)
    keys = {k for m in folded.modules() if isinstance(m, FoldedConv) for k in m._packed}
    assert any(k[2] == (32, 16) for k in keys) and any(k[2] is None for k in keys)
    e_l, e_m, e_32 = _err(out_l, ref), _err(out_m, ref), _err(cpu, ref)
    print(f"folded ResNetUp skip_first={skip_first} fp32: lazy {e_l:.3e}, materialised {e_m:.3e}, cpu fp32 {e_32:.3e}, "
          f"scale {scale:.3e}")
    assert e_l <= max(1e-4 * scale, 3.0 * e_32)
    assert torch.equal(_bits(out_l), _bits(out_m))                  # parts (32, 16): the same steps in the same order
    with torch.autocast("cuda", dtype=BF16):
        f16, _ = _up_forward(folded, down, c["feats"], skip_first, DEV, True, False)
        u16, _ = _up_forward(up, down, c["feats"], skip_first, DEV, False, False)
    assert f16.dtype == BF16
    e_f, e_u = _err(f16, ref), _err(u16, ref)
    print(f"folded ResNetUp skip_first={skip_first} bf16: folded lazy {e_f:.3e}, unfolded {e_u:.3e}")
    assert e_f <= 2.0 * e_u


# ---- the fusion call site ------------------------------------------------------------------------------------------

def _image_data(g, prefix, x, ref_size, dev):
    from deepviewagg_amd.core.multimodal.image import ImageMapping, SameSettingImageData
    n_pts = len(g[prefix + "pointers"]) - 1
    m = ImageMapping.from_dense(t(g[prefix + "point_ids"], dev), t(g[prefix + "image_ids"], dev),
                                t(g[prefix + "pixels_dense"], dev), t(g[prefix + "map_features_dense"], dev),
                                num_points=n_pts)
    B = x.shape[0]
    sd = SameSettingImageData(path=np.array([f"img_{i}" for i in range(B)]), pos=torch.zeros(B, 3, device=dev),
                              opk=torch.zeros(B, 3, device=dev), ref_size=tuple(int(v) for v in ref_size),
                              proj_upscale=1, mappings=m)
    sd.x = x
    return sd


class _Conv2d(torch.nn.Module):
    def __init__(self, c_in, c_out):
        super().__init__()
        self.conv = torch.nn.Conv2d(c_in, c_out, 3, stride=2, padding=1)

    def forward(self, x, reset=True):
        return torch.relu(self.conv(x))


@pytest.mark.parametrize("amp", [None, BF16], ids=["fp32", "autocast_bf16"])
def test_multimodal_block_down_concatenation_fusion_with_the_switch(amp):
    """``MultimodalBlockDown`` with a concatenation fusion onto a voxel tensor: with the switch on, ``x_3d`` between the
    branch and the second 3D block is a lazy tensor of the parts (x_3d.F, x_mod) whose width is the summed width (the
    branch records it as its ``out_channels``), ``x_seen`` is the same, and the block's output is that of the switch off:
    fp32 within 1e-4 of the scale (the rule of the twin test), bf16 within half a bf16 ulp of the largest value, 2^-8 of the
    scale (the padding of the 8-wide part sits at the end of the channel axis on both routes, so the two convolutions
    walk the same steps and no more than a last-place difference is expected)."""
    from types import SimpleNamespace
    from deepviewagg_amd.core.multimodal.image import ImageData
    from deepviewagg_amd.modules.multimodal import BimodalCSRPool, BimodalFusion, GroupBimodalCSRPool, UnimodalBranch
    from deepviewagg_amd.modules.multimodal.modules import MultimodalBlockDown, multimodal_input
    from deepviewagg_amd.modules.SparseConv3d import ResNetDown
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    g = load_golden("branch_nearest")
    n_set = int(g["n_settings"])
    torch.manual_seed(0)

    def inputs():
        xs = [t(g[f"s{i}_x_img"], DEV) for i in range(n_set)]
        sds = [_image_data(g, f"s{i}_", xs[i], g[f"s{i}_ref_size"], DEV) for i in range(n_set)]
        x_3d = t(g["x_3d"])
        n = x_3d.shape[0]
        side = int(np.ceil(n ** (1 / 3))) + 1
        lin = torch.randperm(side ** 3, generator=torch.Generator().manual_seed(7))[:n]
        coords = torch.stack([lin % side, (lin // side) % side, lin // (side * side)], 1).int()

        class _Batch(SimpleNamespace):
            def to(self, device):
                return self
        return _Batch(x=x_3d, coords=coords, batch=torch.zeros(n, dtype=torch.long), pos=None,
                      modalities={"image": ImageData(sds)})

    nc = int(g["x_3d"].shape[1])
    pool = GroupBimodalCSRPool(in_map=8, in_mod=8, num_groups=4, use_num=True)
    branch = UnimodalBranch(_Conv2d(6, 8), BimodalCSRPool(mode="max"), pool, BimodalFusion(mode="concatenation"))
    enc = MultimodalBlockDown(ResNetDown(down_conv_nn=[nc, 16], N=1),
                              ResNetDown(down_conv_nn=[24, 32], stride=1, kernel_size=3, N=1), image=branch).to(DEV).eval()
    seen = {}

    def run(lazy):
        mm = multimodal_input(inputs(), DEV)
        found = snn.LAZY_CAT
        snn.LAZY_CAT = lazy
        branch._out_channels = None
        try:
            with torch.no_grad(), (torch.autocast("cuda", dtype=amp) if amp else contextlib.nullcontext()):
                mm = MultimodalBlockDown.forward_3d_block_down(mm, enc.block_1)
                mm = enc.image(mm, "image")
                mid = mm["x_3d"]
                seen[lazy] = (type(mid), getattr(mid, "parts", None), mid.F.shape[1], branch.out_channels)
                with measure.launch_counter() as launches:
                    mm = MultimodalBlockDown.forward_3d_block_down(mm, enc.block_2)
                seen[lazy] += (launches.names,)
        finally:
            snn.LAZY_CAT = found
        return mm
    off, on = run(False), run(True)
    assert seen[False][0] is snn.SparseVoxelTensor and seen[False][2:4] == (24, 24)
    assert seen[True][0] is snn.LazyCatTensor and [p.shape[1] for p in seen[True][1]] == [16, 8]
    assert seen[True][2:4] == (24, 24)                              # the summed width, for every reader
    assert any(name.startswith("sparse_conv_apply_parts") for name in seen[True][4])
    assert not any("parts" in name for name in seen[False][4])
    assert torch.equal(on["x_seen"], off["x_seen"]) and on["x_seen"].dtype == off["x_seen"].dtype
    assert torch.equal(on["x_3d"].C, off["x_3d"].C) and on["x_3d"].s == off["x_3d"].s
    a, b = on["x_3d"].F, off["x_3d"].F
    assert a.shape == b.shape and a.shape[1] == 32 and a.dtype == b.dtype
    scale = float(b.float().abs().max())
    err = float((a.float() - b.float()).abs().max())
    gate = 1e-4 * scale if amp is None else 2 ** -8 * scale
    print(f"MultimodalBlockDown {'bf16' if amp else 'fp32'}: switch on against off {err:.3e}, gate {gate:.3e}")
    assert err <= gate


# ---- the tensor is really gone ---------------------------------------------------------------------------------------

def test_the_concatenated_tensor_is_not_allocated():
    """No-grad forward of parts (16, 512) -> 64, bf16, 20000 voxels, K = 27, the weights packed beforehand: over the lazy
    call the peak of allocated memory rises by less than half the bytes of the concatenated [n, 528] tensor (the output is
    2.5 MB), over the materialised call by at least those bytes."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d.nn import kernel_offsets
    coords = SR.surface_part(60000, 80, seed=3, lo=0)[:20000]
    n = coords.shape[0]
    assert n == 20000
    cd = torch.from_numpy(coords.astype(np.int32)).to(DEV)
    nbr = ops.voxel_kernel_map(cd, cd, kernel_offsets(3, 1))
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(n, 16, generator=gen).to(DEV).bfloat16()
    b = torch.randn(n, 512, generator=gen).to(DEV).bfloat16()
    W = (torch.randn(27, 528, 64, generator=gen) / np.sqrt(528 * 27 / 4)).to(DEV)
    packed_parts = ops.sparse_conv_pack(W, BF16, parts=(16, 512))
    packed = ops.sparse_conv_pack(W, BF16)
    cat_bytes = n * 528 * 2

    def lazy():
        return ops.sparse_conv_fused([a, b], packed_parts, None, nbr)

    def materialised():
        return ops.sparse_conv_fused(torch.cat([a, b], 1), packed, None, nbr)
    with torch.no_grad():
        assert torch.equal(_bits(lazy()), _bits(materialised()))    # warm: nothing below is a first-call allocation
        torch.cuda.synchronize()
        rise_lazy, rise_mat = measure.peak_bytes(lazy), measure.peak_bytes(materialised)
    print(f"peak rise: lazy {rise_lazy} B, materialised {rise_mat} B, the concatenated tensor {cat_bytes} B")
    assert rise_lazy < cat_bytes / 2
    assert rise_mat >= cat_bytes
