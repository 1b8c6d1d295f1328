"""The folded sparse-convolution inference path on the GPU: ``ops.sparse_conv_pack`` / ``ops.sparse_conv_fused``
(C ABI ``dva_sparse_conv_pack_weights`` / ``dva_sparse_conv_apply_packed``) and ``fold_for_inference`` over the
residual stages of modules/SparseConv3d.

What is held to what:
* the packed route without activation and residual IS the kernel ``ops.sparse_conv`` runs: equal bits;
* fp32 epilogue: equal bits to ``where(o >= 0, o, slope * o) + res`` in torch on the device (three separately rounded
  fp32 operations, activation before the sum);
* bf16 epilogue: one rounding -- within 2^-8 of the largest value of the float64 oracle on the bf16 operands (half an
  ulp of the largest value, the gate of tests/test_gpu_sparseconv.py);
* folded modules against the float64 CPU evaluation of the unfolded modules (the rule of the twin test there).
"""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import sparseconv_oracle as O

sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


def voxel_cloud(n, extent, seed, batches=2):
    """Unique voxels (x, y, z, b) near the faces of a box: the occupancy of a scanned room."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, extent, size=(n, 3))
    p[np.arange(n), rng.integers(0, 3, n)] = rng.integers(0, 2, n) * (extent - 1)
    c = np.unique(np.concatenate([p, rng.integers(0, batches, size=(n, 1))], 1), axis=0)
    rng.shuffle(c)
    return torch.from_numpy(c.astype(np.int32))


@functools.lru_cache(maxsize=None)
def _coords(n):
    full = voxel_cloud(2200, 18, seed=21)
    assert full.shape[0] >= 1500 and int(full[:, 3].max()) == 1
    return full[:n].contiguous()


@functools.lru_cache(maxsize=None)
def _maps(n, kind):
    """(forward map [K, n_out], its transposed map [K, n_in]) on the device for the voxels ``_coords(n)``."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d.nn import downsample_coords, kernel_offsets
    c = _coords(n).to(DEV)
    if kind == "identity":
        ident = torch.arange(n, dtype=torch.int32, device=DEV).unsqueeze(0)
        return ident, ident
    if kind == "k3s1":
        offs = kernel_offsets(3, 1)
        return ops.voxel_kernel_map(c, c, offs), ops.voxel_kernel_map(c, c, -offs)
    dst = downsample_coords(c, 2)
    offs = kernel_offsets(2, 1)
    down, up = ops.voxel_kernel_map(c, dst, offs), ops.voxel_kernel_map(dst, c, -offs)
    assert 0 < dst.shape[0] < n or n == 1
    return (down, up) if kind == "k2s2" else (up, down)


# name -> (voxels, Cin, Cout, map, bias, residual, slope)
CASES = {
    "k3s1_16_16": (1500, 16, 16, "k3s1", True, True, 0.0),
    "k3s1_32_64": (1500, 32, 64, "k3s1", False, True, 0.2),
    "k3s1_80_48": (1500, 80, 48, "k3s1", True, False, 0.0),
    "k3s1_64_128": (1500, 64, 128, "k3s1", True, True, 0.0),            # the 128-wide tile
    "k3s1_5_7": (1500, 5, 7, "k3s1", True, True, 0.2),                  # channels padded to 16 on the host
    "k2s2_32_64": (1500, 32, 64, "k2s2", True, True, 0.0),
    "k2s2_80_48": (1500, 80, 48, "k2s2", False, True, 1.0),
    "k2s2T_64_128": (1500, 64, 128, "k2s2T", True, True, 0.2),
    "k2s2T_32_64": (1500, 32, 64, "k2s2T", False, False, 0.0),
    "k2s2T_5_7": (1500, 5, 7, "k2s2T", False, True, 0.0),
    "identity_16_16": (1500, 16, 16, "identity", True, True, 0.0),
    "identity_64_128": (1500, 64, 128, "identity", False, True, 1.0),
    "identity_5_7": (1500, 5, 7, "identity", True, False, 0.2),
    "identity_80_48": (1500, 80, 48, "identity", True, True, 0.2),
    "n1": (1, 32, 64, "k3s1", True, True, 0.0),
    "n63": (63, 32, 64, "k3s1", False, True, 0.2),
    "n64": (64, 32, 64, "k3s1", True, True, 0.0),
    "n65": (65, 32, 64, "k3s1", True, True, 0.2),
    "n65_64_128": (65, 64, 128, "k3s1", True, True, 0.0),
}


def _operands(name, dtype):
    n, cin, cout, kind, bias, residual, slope = CASES[name]
    nbr, nbr_t = _maps(n, kind)
    gen = torch.Generator().manual_seed(len(name) + cin + 3 * cout)
    K, n_in, n_out = nbr.shape[0], nbr_t.shape[1], nbr.shape[1]
    x = torch.randn(n_in, cin, generator=gen).to(dtype)
    W = torch.randn(K, cin, cout, generator=gen) / np.sqrt(cin * K / 4)
    b = torch.randn(cout, generator=gen) if bias else None
    res = torch.randn(n_out, cout, generator=gen).to(dtype) if residual else None
    return nbr, nbr_t, x, W, b, res, slope


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_convolution(name, dtype):
    """Checks 1, 2 / 3 and reproducibility of one case."""
    from deepviewagg_amd import ops
    nbr, nbr_t, x, W, b, res, slope = _operands(name, dtype)
    packed = ops.sparse_conv_pack(W.to(DEV), dtype)
    assert (packed.K, packed.cin, packed.cout) == tuple(W.shape) and packed.dtype == dtype
    assert packed.cin_p % 16 == 0 and packed.cout_p % 16 == 0 and packed.buf.dtype == torch.uint8
    xd, bd, rd = x.to(DEV), _dev(b), _dev(res)
    with torch.no_grad():
        plain = ops.sparse_conv(xd, W.to(DEV), bd, nbr, nbr_t)
        o = ops.sparse_conv_fused(xd, packed, bd, nbr)
        out = ops.sparse_conv_fused(xd, packed, bd, nbr, residual=rd, slope=slope)
        again = ops.sparse_conv_fused(xd, packed, bd, nbr, residual=rd, slope=slope)
    assert o.dtype == dtype and o.shape == plain.shape == (nbr.shape[1], W.shape[2])
    assert torch.equal(_bits(o), _bits(plain)), "the packed route is not the kernel ops.sparse_conv runs"
    assert out.dtype == dtype and out.shape == o.shape and torch.equal(_bits(out), _bits(again))
    if dtype == F32:
        expect = torch.where(o >= 0, o, slope * o)
        if rd is not None:
            expect = expect + rd
        assert torch.equal(_bits(out), _bits(expect)), \
            f"fp32 epilogue: {int((_bits(out) != _bits(expect)).sum())} elements differ from the torch expression"
        return
    ref = O.sparse_conv(x.double(), W.bfloat16().double(), None if b is None else b.double(), nbr.cpu())
    ref = torch.where(ref >= 0, ref, slope * ref)
    if res is not None:
        ref = ref + res.double()
    err = float((out.cpu().double() - ref).abs().max())
    scale = float(ref.abs().max()) + 1e-12
    print(f"{name} bf16: max error {err:.3e}, gate {2 ** -8 * scale:.3e}")
    assert err <= 2 ** -8 * scale, f"{err:.3e} vs {2 ** -8 * scale:.3e}"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["k3s1_32_64", "k3s1_64_128", "k2s2T_5_7", "identity_80_48"])
def test_rows_without_neighbours(name, dtype):
    """Destinations whose map columns are all -1 (single rows, and 192 rows in a run so that whole wavefronts skip
    every offset) get exactly act(bias) + residual; every other row keeps its bits."""
    from deepviewagg_amd import ops
    nbr, _, x, W, b, res, slope = _operands(name, dtype)
    if b is None:
        b = torch.randn(W.shape[2], generator=torch.Generator().manual_seed(5))
    n_out = nbr.shape[1]
    cols = torch.zeros(n_out, dtype=torch.bool)
    cols[::7] = True
    cols[130:322] = True
    masked = nbr.clone()
    masked[:, cols.to(DEV)] = -1
    packed = ops.sparse_conv_pack(W.to(DEV), dtype)
    bd, rd = b.to(DEV), _dev(res)
    full = ops.sparse_conv_fused(x.to(DEV), packed, bd, nbr, residual=rd, slope=slope)
    got = ops.sparse_conv_fused(x.to(DEV), packed, bd, masked, residual=rd, slope=slope)
    v = bd.expand(n_out, -1).clone()
    v = torch.where(v >= 0, v, slope * v)
    if rd is not None:
        v = v + rd.float()
    v = v.to(dtype)
    cd = cols.to(DEV)
    assert torch.equal(_bits(got[cd]), _bits(v[cd]))
    assert torch.equal(_bits(got[~cd]), _bits(full[~cd]))
    assert not torch.equal(got[cd].float(), full[cd].float())           # the mask removed something


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_empty_inputs_return_the_stated_rows_without_a_launch(dtype):
    from deepviewagg_amd import ops
    gen = torch.Generator().manual_seed(1)
    W = torch.randn(27, 32, 48, generator=gen).to(DEV)
    b = torch.randn(48, generator=gen).to(DEV)
    packed = ops.sparse_conv_pack(W, dtype)
    for n_src, n_dst in ((0, 40), (40, 0), (0, 0)):
        x = torch.randn(n_src, 32, device=DEV).to(dtype)
        nbr = torch.full((27, n_dst), -1, dtype=torch.int32, device=DEV)
        res = torch.randn(n_dst, 48, device=DEV).to(dtype)
        for bias, residual, slope in ((b, res, 0.0), (None, res, 0.2), (b, None, 0.2), (None, None, 1.0)):
            with measure.launch_counter() as launches:
                out = ops.sparse_conv_fused(x, packed, bias, nbr, residual=residual, slope=slope)
            assert launches.names == [] and out.shape == (n_dst, 48) and out.dtype == dtype
            v = torch.zeros(n_dst, 48, device=DEV) + (bias if bias is not None else 0.0)
            v = torch.where(v >= 0, v, slope * v)
            if residual is not None:
                v = v + residual.float()
            assert torch.equal(_bits(out), _bits(v.to(dtype)))


def test_no_autograd_and_the_autocast_rule():
    from deepviewagg_amd import ops
    nbr, _, x, W, b, res, _ = _operands("k3s1_32_64", F32)
    b = torch.randn(W.shape[2])
    p32, p16 = ops.sparse_conv_pack(W.to(DEV), F32), ops.sparse_conv_pack(W.to(DEV), BF16)
    xd = x.to(DEV)
    for bad in ((xd.clone().requires_grad_(True), b.to(DEV), res.to(DEV)),
                (xd, b.to(DEV).requires_grad_(True), res.to(DEV)),
                (xd, b.to(DEV), res.to(DEV).requires_grad_(True))):
        with pytest.raises(RuntimeError):
            ops.sparse_conv_fused(bad[0], p32, bad[1], nbr, residual=bad[2])
        with torch.no_grad():
            assert not ops.sparse_conv_fused(bad[0], p32, bad[1], nbr, residual=bad[2]).requires_grad
    plain = ops.sparse_conv_fused(xd, p32, b.to(DEV), nbr, residual=res.to(DEV), slope=0.0)
    with torch.autocast("cuda", dtype=BF16):
        out = ops.sparse_conv_fused(xd, p16, b.to(DEV), nbr, residual=res.to(DEV), slope=0.0)
        with pytest.raises(TypeError):
            ops.sparse_conv_fused(xd, p32, None, nbr)                   # packed for the other feature dtype
    assert out.dtype == BF16
    same = ops.sparse_conv_fused(xd.bfloat16(), p16, b.to(DEV), nbr, residual=res.to(DEV).bfloat16(), slope=0.0)
    assert torch.equal(_bits(out), _bits(same))
    with torch.autocast("cuda", dtype=torch.float16):
        out = ops.sparse_conv_fused(xd, p32, b.to(DEV), nbr, residual=res.to(DEV), slope=0.0)
    assert out.dtype == F32 and torch.equal(_bits(out), _bits(plain))
    with pytest.raises(TypeError):
        ops.sparse_conv_pack(W.to(DEV), torch.float16)


# ---- modules ---------------------------------------------------------------------------------------------------

def _randomise_norms(modules, seed):
    gen = torch.Generator().manual_seed(seed)
    for top in modules:
        for m in top.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                c = m.num_features
                with torch.no_grad():
                    m.running_mean.copy_(torch.randn(c, generator=gen) * 0.3)
                    m.running_var.copy_(torch.rand(c, generator=gen) * 1.5 + 0.5)
                    m.weight.copy_((torch.rand(c, generator=gen) + 0.5) * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1))
                    m.bias.copy_(torch.randn(c, generator=gen) * 0.3)


def _forward(mods, feats, coords, dev):
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    down, up = mods
    with torch.no_grad():
        x = snn.SparseVoxelTensor(feats.clone().to(dev), coords.to(dev))
        y = down(x)
        z = up(y, x)
    return x, y, z


@functools.lru_cache(maxsize=None)
def _stage_case(block):
    """The modules, the input and the CPU evaluations (fp32 and float64, through the oracle) of one block type."""
    from deepviewagg_amd.modules.SparseConv3d import ResNetDown, ResNetUp
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    coords = voxel_cloud(2500, 16, seed=11)
    torch.manual_seed(7)
    feats = torch.randn(coords.shape[0], 16)
    down = ResNetDown(down_conv_nn=[16, 32], N=2, block=block).eval()
    up = ResNetUp(up_conv_nn=[32, 16, 24], N=1, block=block).eval()
    _randomise_norms((down, up), seed=13)
    d64, u64 = copy.deepcopy(down).double(), copy.deepcopy(up).double()
    with pytest.MonkeyPatch.context() as m:
        m.setattr(snn, "ops", O.OracleOps)
        m.setattr(snn, "batchnorm_act_rows", O.batchnorm_act_rows)
        _, yc, zc = _forward((down, up), feats, coords, "cpu")
        _, yr, zr = _forward((d64, u64), feats.double(), coords, "cpu")
    return dict(coords=coords, feats=feats, down=down, up=up, cpu32=(yc, zc), ref=(yr, zr))


def _err(a, r):
    return float((a.detach().cpu().double() - r.double()).abs().max())


@pytest.mark.parametrize("block", ["ResBlock", "BottleneckBlock"])
def test_folded_stages_match_the_float64_twin(block):
    from deepviewagg_amd.modules.SparseConv3d import fold_for_inference
    c = _stage_case(block)
    gd, gu = copy.deepcopy(c["down"]).to(DEV), copy.deepcopy(c["up"]).to(DEV)
    fd, fu = fold_for_inference(gd), fold_for_inference(gu)
    _, yf, zf = _forward((fd, fu), c["feats"], c["coords"], DEV)
    _, yg, zg = _forward((gd, gu), c["feats"], c["coords"], DEV)
    for got in ((yf, zf), (yg, zg)):
        assert torch.equal(got[0].C.cpu(), c["ref"][0].C) and torch.equal(got[1].C.cpu(), c["ref"][1].C)
        assert got[0].s == c["ref"][0].s == 2 and got[1].s == c["ref"][1].s == 1
    for what, f, g, c32, r in (("encoder", yf, yg, c["cpu32"][0], c["ref"][0]),
                               ("decoder", zf, zg, c["cpu32"][1], c["ref"][1])):
        assert f.F.dtype == F32 and f.F.shape == r.F.shape
        scale = float(r.F.abs().max()) + 1e-12
        e_f, e_g, e_32 = _err(f.F, r.F), _err(g.F, r.F), _err(c32.F, r.F)
        print(f"{block} {what} fp32: folded {e_f:.3e}, unfolded {e_g:.3e}, cpu fp32 {e_32:.3e}, scale {scale:.3e}")
        assert e_f <= max(1e-4 * scale, 3.0 * e_32), f"{what}: {e_f:.3e} (cpu fp32 {e_32:.3e}, scale {scale:.3e})"
    # a second call (packed operands and maps cached now) gives the same bits
    _, y2, z2 = _forward((fd, fu), c["feats"], c["coords"], DEV)
    assert torch.equal(_bits(y2.F), _bits(yf.F)) and torch.equal(_bits(z2.F), _bits(zf.F))


@pytest.mark.parametrize("block", ["ResBlock", "BottleneckBlock"])
def test_folded_stages_bf16_round_no_more_than_the_unfolded(block):
    """Under autocast(bfloat16): folded 'ResBlock' encoder / decoder errors measured on an MI355X are in
    DESIGN.md (sparse-convolution inference fold)."""
    from deepviewagg_amd.modules.SparseConv3d import fold_for_inference
    c = _stage_case(block)
    gd, gu = copy.deepcopy(c["down"]).to(DEV), copy.deepcopy(c["up"]).to(DEV)
    fd, fu = fold_for_inference(gd), fold_for_inference(gu)
    with torch.autocast("cuda", dtype=BF16):
        _, yf, zf = _forward((fd, fu), c["feats"], c["coords"], DEV)
        _, yg, zg = _forward((gd, gu), c["feats"], c["coords"], DEV)
    for what, f, g, r in (("encoder", yf, yg, c["ref"][0]), ("decoder", zf, zg, c["ref"][1])):
        assert f.F.dtype == BF16 and torch.equal(f.C.cpu(), r.C)
        e_f, e_g = _err(f.F, r.F), _err(g.F, r.F)
        print(f"{block} {what} bf16: folded {e_f:.3e}, unfolded {e_g:.3e}, ratio {e_f / e_g:.2f}, "
              f"scale {float(r.F.abs().max()):.3e}")
        assert e_f <= 2.0 * e_g, f"{what}: folded {e_f:.3e} vs unfolded {e_g:.3e}"


def test_folded_stage_inside_a_multimodal_block_down():
    """forward_3d_block_down with a folded ResNetDown and no modality branch: a SparseVoxelTensor that shares the
    coordinate and kernel-map caches of its input, with the maps the layers built in them."""
    from deepviewagg_amd.modules.SparseConv3d import fold_for_inference
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    from deepviewagg_amd.modules.multimodal.modules import MultimodalBlockDown
    c = _stage_case("BottleneckBlock")
    folded = fold_for_inference(copy.deepcopy(c["down"]).to(DEV))
    x = snn.SparseVoxelTensor(c["feats"].to(DEV), c["coords"].to(DEV))
    seen = torch.ones(x.C.shape[0], dtype=torch.bool, device=DEV)
    with torch.no_grad():
        out = MultimodalBlockDown.forward_3d_block_down({"x_3d": x, "x_seen": seen, "modalities": {}}, folded)
    y = out["x_3d"]
    assert isinstance(y, snn.SparseVoxelTensor) and y.s == 2 and y.F.shape == (c["ref"][0].F.shape[0], 32)
    assert y.coord_maps is x.coord_maps and y.kernel_maps is x.kernel_maps
    assert set(x.coord_maps) == {1, 2} and torch.equal(x.coord_maps[2].cpu(), c["ref"][0].C)
    assert set(x.kernel_maps) == {(1, 2, 2, 1), (2, 3, 1, 1), (2, 1, 1, 1)}
    ident = x.kernel_maps[(2, 1, 1, 1)][0]
    assert torch.equal(ident, torch.arange(y.C.shape[0], dtype=torch.int32, device=DEV).unsqueeze(0))
    assert out["x_seen"].shape == (y.C.shape[0],) and bool(out["x_seen"].all())
    scale = float(c["ref"][0].F.abs().max())
    assert _err(y.F, c["ref"][0].F) <= max(1e-4 * scale, 3.0 * _err(c["cpu32"][0].F, c["ref"][0].F))
