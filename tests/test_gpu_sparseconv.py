"""Sparse 3D convolution on the GPU (C ABI dva_voxel_kernel_map / dva_sparse_conv_apply / dva_sparse_conv_wgrad,
modules/SparseConv3d) against oracle/sparseconv_oracle.py (torchsparse 1.1.0 is not in the reference tree:
parity unpinned for the library itself; the oracle is pinned to torch's dense conv3d in
tests/test_sparseconv_oracle.py).  Kernel maps: bit-exact.  Features: fp32 path within 2e-5 of the fp64
oracle relative to the output scale (3-term bf16 split on the matrix cores), bf16 path within bf16 rounding
of the oracle evaluated on the same bf16-rounded operands."""
import copy

import numpy as np
import pytest
import torch

from oracle import sparseconv_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def surface_cloud(n, extent, seed, batches=1, stride=1, lo=0):
    """Voxels near the faces of a box (the occupancy pattern of scanned rooms), unique rows (x, y, z, b)."""
    rng = np.random.default_rng(seed)
    p = rng.integers(lo, lo + extent, size=(n, 3))
    face = rng.integers(0, 3, n)
    p[np.arange(n), face] = lo + rng.integers(0, 2, n) * (extent - 1)
    b = rng.integers(0, batches, size=(n, 1))
    c = np.unique(np.concatenate([p * stride, b], 1), axis=0)
    rng.shuffle(c)
    return torch.from_numpy(c.astype(np.int32))


@pytest.mark.parametrize("n,extent,k,stride,batches,lo", [(1, 4, 3, 1, 1, 0), (700, 10, 3, 1, 2, -5),
                                                          (900, 12, 2, 2, 2, -3), (500, 9, 3, 2, 1, 0)])
def test_kernel_map_matches_oracle(n, extent, k, stride, batches, lo):
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d.nn import downsample_coords, kernel_offsets
    src = surface_cloud(n, extent, seed=n + k, batches=batches, lo=lo)
    dst = src if stride == 1 else downsample_coords(src.to(DEV), stride).cpu()
    assert torch.equal(dst, src if stride == 1 else O.downsample_coords(src, stride))
    offs = kernel_offsets(k, 1)
    nbr = ops.voxel_kernel_map(src.to(DEV), dst.to(DEV), offs)
    assert nbr.dtype == torch.int32 and torch.equal(nbr.cpu(), O.kernel_map(src, dst, offs))
    nbr_t = ops.voxel_kernel_map(dst.to(DEV), src.to(DEV), -offs)
    assert torch.equal(nbr_t.cpu(), O.kernel_map(dst, src, -offs))


def _maps(coords, k, stride):
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d.nn import downsample_coords, kernel_offsets
    c = coords.to(DEV)
    dst = c if stride == 1 else downsample_coords(c, stride)
    offs = kernel_offsets(k, 1)
    return ops.voxel_kernel_map(c, dst, offs), ops.voxel_kernel_map(dst, c, -offs)


@pytest.mark.parametrize("n,cin,cout,k,stride,bias", [
    (50, 16, 16, 3, 1, False), (1300, 32, 64, 3, 1, True), (777, 5, 7, 3, 1, True), (900, 64, 128, 3, 1, False),
    (600, 80, 48, 3, 1, False), (1500, 32, 32, 2, 2, False), (400, 144, 16, 2, 2, True)])
def test_sparse_conv_fp32_matches_oracle(n, cin, cout, k, stride, bias):
    from deepviewagg_amd import ops
    torch.manual_seed(n + cin)
    coords = surface_cloud(n, 14, seed=n, batches=2)
    nbr, nbr_t = _maps(coords, k, stride)
    x = torch.randn(coords.shape[0], cin)
    W = torch.randn(k ** 3, cin, cout) / np.sqrt(cin * k ** 3 / 4)
    b = torch.randn(cout) if bias else None
    g = torch.randn(nbr.shape[1], cout)
    # oracle in float64
    xr, Wr = x.double().requires_grad_(True), W.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    ref = O.sparse_conv(xr, Wr, br, nbr.cpu())
    ref.backward(g.double())
    xd, Wd = x.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True) if bias else None
    out = ops.sparse_conv(xd, Wd, bd, nbr, nbr_t)
    out.backward(g.to(DEV))

    def close(a, r, what):
        err = float((a.detach().cpu().double() - r).abs().max())
        scale = float(r.abs().max()) + 1e-12
        assert err <= 2e-5 * scale, f"{what}: {err:.3e} vs scale {scale:.3e}"
    close(out, ref.detach(), "out")
    close(xd.grad, xr.grad, "grad x")
    close(Wd.grad, Wr.grad, "grad W")
    if bias:
        close(bd.grad, br.grad, "grad bias")


@pytest.mark.parametrize("n,cin,cout,k,stride", [(1100, 32, 64, 3, 1), (800, 64, 64, 2, 2), (500, 96, 32, 3, 1)])
def test_sparse_conv_bf16_matches_oracle_on_rounded_operands(n, cin, cout, k, stride):
    from deepviewagg_amd import ops
    torch.manual_seed(n)
    coords = surface_cloud(n, 14, seed=n + 1)
    nbr, nbr_t = _maps(coords, k, stride)
    x = torch.randn(coords.shape[0], cin).bfloat16()
    W = torch.randn(k ** 3, cin, cout) / np.sqrt(cin * k ** 3 / 4)
    g = torch.randn(nbr.shape[1], cout).bfloat16()
    xr = x.double().requires_grad_(True)
    Wr = W.bfloat16().double().requires_grad_(True)         # the kernel rounds the fp32 master weights to bf16
    ref = O.sparse_conv(xr, Wr, None, nbr.cpu())
    ref.backward(g.double())
    xd, Wd = x.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
    out = ops.sparse_conv(xd, Wd, None, nbr, nbr_t)
    assert out.dtype == torch.bfloat16
    out.backward(g.to(DEV))
    for a, r, tol in [(out, ref.detach(), 2 ** -8), (xd.grad, xr.grad, 2 ** -8), (Wd.grad, Wr.grad, 1e-5)]:
        err = float((a.detach().cpu().double() - r).abs().max())
        assert err <= tol * (float(r.abs().max()) + 1e-12)    # bf16 outputs: half an ulp of the largest value


def test_sparse_conv_rejects_host_tensors_and_bad_shapes():
    from deepviewagg_amd import ops, _lib
    with pytest.raises(_lib.DvaError):
        ops.voxel_kernel_map(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.int32), [[0, 0, 0]])
    coords = surface_cloud(100, 8, seed=0)
    nbr, nbr_t = _maps(coords, 3, 1)
    with pytest.raises(AssertionError):
        ops.sparse_conv(torch.randn(coords.shape[0], 8, device=DEV), torch.randn(27, 16, 16, device=DEV), None,
                        nbr, nbr_t)


def _twin_forward_backward(mods, feats, coords, dev):
    """ResNetDown -> ResNetUp forward + backward; also returns the ReLU activity patterns of the fused BN-ReLU
    layers (to detect pre-activations that straddle zero between two evaluations)."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    x = snn.SparseVoxelTensor(feats.detach().clone().to(dev).requires_grad_(True), coords.to(dev))
    down, up = mods
    active, handles = [], []
    for top in mods:
        for seq in top.modules():
            if isinstance(seq, snn.Seq):
                layers = list(seq)
                for i, m in enumerate(layers[:-1]):
                    if isinstance(m, snn.BatchNorm) and isinstance(layers[i + 1], snn.ReLU):
                        handles.append(m.register_forward_hook(
                            lambda mod, inp, out: active.append((out.F.detach() > 0).cpu())))
    y = down(x)
    z = up(y, x)
    loss = z.F.float().square().mean() + y.F.float().mean()
    loss.backward()
    for hd in handles:
        hd.remove()
    return x, y, z, active


@pytest.mark.parametrize("block", ["ResBlock", "BottleneckBlock"])
def test_resnet_stages_match_cpu_twin(block, monkeypatch):
    """ResNetDown -> ResNetUp (strided conv, residual blocks, transposed conv, skip concatenation, BatchNorm in
    training mode) on the GPU against the same modules evaluated on the CPU with the oracle convolution in fp64.
    A ReLU whose pre-activation is within rounding of zero may switch between the two evaluations (the 3-term
    split leaves ~1e-5 relative error on the features) and changes the gradient of that unit by 100 %: such
    draws are counted (they must stay rare) and the gradient comparison uses a draw without any."""
    from deepviewagg_amd.modules.SparseConv3d import ResNetDown, ResNetUp
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    coords = surface_cloud(2500, 16, seed=11, batches=2)
    for attempt in range(6):
        torch.manual_seed(3 + attempt)
        feats = torch.randn(coords.shape[0], 16)
        down = ResNetDown(down_conv_nn=[16, 32], N=2, block=block)
        up = ResNetUp(up_conv_nn=[32, 16, 24], N=1, block=block)
        gd, gu = copy.deepcopy(down).to(DEV), copy.deepcopy(up).to(DEV)
        d64, u64 = copy.deepcopy(down).double(), copy.deepcopy(up).double()
        xg, yg, zg, act_g = _twin_forward_backward((gd, gu), feats, coords, DEV)
        with monkeypatch.context() as m:
            m.setattr(snn, "ops", O.OracleOps)
            m.setattr(snn, "batchnorm_act_rows", O.batchnorm_act_rows)
            xc, yc, zc, _ = _twin_forward_backward((down, up), feats, coords, "cpu")             # fp32 on the CPU
            xr, yr, zr, act_r = _twin_forward_backward((d64, u64), feats.double(), coords, "cpu")  # fp64 reference
        assert torch.equal(yg.C.cpu(), yr.C) and torch.equal(zg.C.cpu(), zr.C) and yg.s == 2 and zg.s == 1

        def close(a, c, r, what, tol):
            """GPU error against the fp64 reference: within `tol` of the reference scale, or no worse than 3x
            the error the fp32 CPU evaluation of the same formulas makes."""
            r = r.detach().double()
            err = float((a.detach().cpu().double() - r).abs().max())
            err32 = float((c.detach().double() - r).abs().max())
            assert err <= max(tol * (float(r.abs().max()) + 1e-12), 3.0 * err32), \
                f"{what}: {err:.3e} (cpu fp32 {err32:.3e})"
        close(yg.F, yc.F, yr.F, "encoder features", 1e-4)
        close(zg.F, zc.F, zr.F, "decoder features", 1e-4)
        flips = sum(int((a != b).sum()) for a, b in zip(act_g, act_r))
        assert len(act_g) == len(act_r) > 0 and flips <= 4, f"{flips} ReLU units switched"
        if flips:
            continue
        close(xg.F.grad, xc.F.grad, xr.F.grad, "input gradient", 2e-4)
        names = [n for n, _ in list(gd.named_parameters()) + list(gu.named_parameters())]
        for name, pg, pc, pr in zip(names, list(gd.parameters()) + list(gu.parameters()),
                                    list(down.parameters()) + list(up.parameters()),
                                    list(d64.parameters()) + list(u64.parameters())):
            close(pg.grad, pc.grad, pr.grad, name, 2e-4)
        for (name, bg), bc, br in zip(gd.named_buffers(), down.buffers(), d64.buffers()):
            if name.endswith("num_batches_tracked"):      # the functional oracle does not count; nn.BatchNorm1d does
                assert int(bg) == 1
            else:
                close(bg, bc, br, name, 1e-5)
        return
    pytest.fail("every draw had a ReLU unit within rounding of zero")


def test_sparse_conv_adjoint_property_at_scale():
    """<conv(x), y> == <x, conv^T(y)> on 200k voxels, 64 -> 64 channels (input-gradient kernel against the forward
    kernel) and the weight gradient against the same contraction written with torch index ops on the device."""
    from deepviewagg_amd import ops
    torch.manual_seed(0)
    coords = surface_cloud(400000, 260, seed=5)
    nbr, nbr_t = _maps(coords, 3, 1)
    # both maps come from the device: held to the CPU oracle first, or two maps that miss the same pairs would pass
    ref_map = O.kernel_map_sorted(coords, coords, O.kernel_offsets(3))
    assert torch.equal(nbr.cpu(), ref_map) and torch.equal(nbr_t.cpu(), torch.flip(ref_map, [0]))
    n = coords.shape[0]
    x = torch.randn(n, 64, device=DEV, requires_grad=True)
    W = (torch.randn(27, 64, 64, device=DEV) / 20).requires_grad_(True)
    y = torch.randn(n, 64, device=DEV)
    out = ops.sparse_conv(x, W, None, nbr, nbr_t)
    out.backward(y)
    lhs = float((out.detach().double() * y.double()).sum())
    rhs = float((x.detach().double() * x.grad.double()).sum())
    assert abs(lhs - rhs) <= 2e-5 * abs(lhs) + 1e-3      # both sides carry the ~2^-16 error of the 3-term split
    k = 5
    dst = torch.nonzero(nbr[k] >= 0).flatten()
    ref = x.detach()[nbr[k][dst].long()].double().t() @ y[dst].double()
    # (3-term split: the dropped lo*lo products leave ~2^-16 relative error per term of the 400k-term sums)
    assert float((W.grad[k].double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    assert float((W.grad[13].double() - x.detach().double().t() @ y.double()).abs().max()) \
        <= 1e-4 * float((x.detach().double().t() @ y.double()).abs().max())


# ======================================================================================================================
# Row by row against the split emulation (tests/sparse_rows.py).  fp32 features: the device against the
# float64 evaluation of the 3-term split, per stratum of destination rows, gated by FP32_HEADROOM x the noise of the
# split evaluated in float32; the 2e-5 statement against exact float64 stays beside it.  bf16 features: the device
# against the float64 oracle on the bf16 operands, gated by the noise of bf16(float32 evaluation).  No row tolerance is
# typed in.  Every CPU evaluation of a case is computed once (SR.conv_case) and shared.
# ======================================================================================================================
import rowwise as RW                                            # noqa: E402
import sparse_rows as SR                                        # noqa: E402
from tolerances import Report                                   # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
ALL_STRATA = ("nbr_1", "nbr_2_8", "nbr_9_26", "nbr_27", "tile_edge", "last_tile", "wave_skips", "wave_no_skip")
_section = Report("sparse convolution: rows against the split emulation (fp32) / the float64 oracle on bf16 operands")
_worst = {}

# Open findings: strata of fp32 cases that miss FP32_HEADROOM x the noise of the PLAIN float32 evaluation of the split
# (blocked matrix product per offset, 27 additions) because the kernel keeps ONE fp32 accumulator over K Cin / 8 x 3
# dependent additions.  {case: {(tensor, stratum, "max" | "p99"): measured on an MI355X}}, entered with Report.add_open
# (must still miss, must not grow).  The proof runs in the same test: every stratum meets the same gate with the noise of
# the float32 evaluation in the kernel's accumulation order (SR.gate_kernel_order; device / noise 1.0 .. 1.5 there).
OPEN_CAUSE = ("accumulation order: one fp32 accumulator over all offsets, channels and the three split terms; the same "
              "rows meet the gate against the float32 evaluation in that order")
OPEN = {
    "strata_32_64_bias fp32": {
        ("grad_x", "all", "max"): 7.36e-07, ("grad_x", "nbr_27", "max"): 7.36e-07,
        ("grad_x", "wave_no_skip", "max"): 7.36e-07, ("grad_x", "wave_no_skip", "p99"): 5.86e-07,
    },
    "strata_80_48 fp32": {
        ("out", "all", "max"): 8.57e-07, ("out", "all", "p99"): 5.97e-07, ("out", "nbr_9_26", "max"): 8.57e-07,
        ("out", "nbr_27", "max"): 7.97e-07, ("out", "tile_edge", "max"): 8.57e-07,
        ("out", "wave_no_skip", "max"): 8.57e-07, ("out", "wave_no_skip", "p99"): 6.39e-07,
    },
    "s600_64_128 fp32": {
        ("out", "wave_no_skip", "p99"): 5.28e-07, ("grad_x", "all", "max"): 9.69e-07,
        ("grad_x", "all", "p99"): 7.55e-07, ("grad_x", "nbr_9_26", "p99"): 6.93e-07,
        ("grad_x", "nbr_27", "max"): 9.69e-07, ("grad_x", "wave_no_skip", "max"): 9.69e-07,
        ("grad_x", "wave_no_skip", "p99"): 7.86e-07,
    },
    "s600_256_256 fp32": {
        ("out", "all", "max"): 1.10e-06, ("out", "all", "p99"): 1.02e-06, ("out", "nbr_9_26", "max"): 9.14e-07,
        ("out", "nbr_9_26", "p99"): 8.70e-07, ("out", "nbr_27", "max"): 1.10e-06,
        ("out", "tile_edge", "max"): 1.02e-06, ("out", "wave_skips", "max"): 8.43e-07,
        ("out", "wave_skips", "p99"): 7.38e-07, ("out", "wave_no_skip", "max"): 1.10e-06,
        ("out", "wave_no_skip", "p99"): 1.05e-06, ("grad_x", "all", "max"): 1.08e-06,
        ("grad_x", "all", "p99"): 9.87e-07, ("grad_x", "nbr_9_26", "max"): 9.10e-07,
        ("grad_x", "nbr_9_26", "p99"): 8.42e-07, ("grad_x", "nbr_27", "max"): 1.08e-06,
        ("grad_x", "tile_edge", "max"): 1.07e-06, ("grad_x", "wave_skips", "max"): 8.47e-07,
        ("grad_x", "wave_skips", "p99"): 7.57e-07, ("grad_x", "wave_no_skip", "max"): 1.08e-06,
        ("grad_x", "wave_no_skip", "p99"): 1.03e-06,
    },
    "s6000_80_48 fp32": {
        ("out", "all", "max"): 7.95e-07, ("out", "all", "p99"): 5.24e-07, ("out", "nbr_9_26", "max"): 7.95e-07,
        ("out", "nbr_9_26", "p99"): 5.60e-07, ("out", "nbr_27", "max"): 7.29e-07,
        ("out", "wave_no_skip", "max"): 7.95e-07, ("out", "wave_no_skip", "p99"): 6.44e-07,
        ("grad_x", "wave_no_skip", "p99"): 4.80e-07,
    },
    "s6000_32_64 fp32": {
        ("grad_x", "all", "max"): 8.00e-07, ("grad_x", "nbr_27", "max"): 8.00e-07,
        ("grad_x", "tile_edge", "max"): 8.00e-07, ("grad_x", "wave_no_skip", "max"): 8.00e-07,
        ("grad_x", "wave_no_skip", "p99"): 6.24e-07,
    },
    "n63 fp32": {
        ("grad_x", "all", "max"): 6.85e-07, ("grad_x", "nbr_9_26", "max"): 6.85e-07,
        ("grad_x", "last_tile", "max"): 6.85e-07, ("grad_x", "wave_no_skip", "max"): 6.85e-07,
    },
    "n65 fp32": {
        ("grad_x", "all", "max"): 6.83e-07, ("grad_x", "nbr_9_26", "max"): 6.83e-07,
        ("grad_x", "wave_no_skip", "max"): 6.83e-07,
    },
}


def _open(name):
    return {k: (v, OPEN_CAUSE) for k, v in OPEN.get(name, {}).items()} or None


@pytest.fixture(scope="module", autouse=True)
def _rows_report():
    """One "sparse convolution" section per run in the file DVA_ROWWISE_REPORT names (profiles/rowwise_report.txt)."""
    yield
    if _section.rows:
        for key in sorted(_worst):
            _section.notes.append(f"worst device / noise ratio, {key[0]} {key[1]}: {_worst[key][0]:.2f} ({_worst[key][1]})")
        RW.write_report(_section)


def _finish(rep, c, worst, out=None, gx=None):
    """Close one case: fp32 cases also state every stratum of ``out`` / ``gx`` against the noise of the float32
    evaluation in the kernel's accumulation order (no open entries there: the proof behind the ones in OPEN)."""
    if c["dtype"] == F32 and out is not None:
        for tensor, ratio in SR.gate_kernel_order(rep, c, out, gx).items():
            worst[tensor + " [kernel order]"] = ratio
    _section.rows += rep.rows
    _section.open += rep.open
    kind = "fp32" if c["dtype"] == F32 else "bf16"
    for tensor, ratio in worst.items():
        if ratio > _worst.get((kind, tensor), (0.0, ""))[0]:
            _worst[(kind, tensor)] = (ratio, c["name"])
    rep.check()


def _device_maps(c):
    """The device's kernel map pair of case ``c``, held bit-exact to the oracle's before it is used."""
    from deepviewagg_amd import ops
    nbr = ops.voxel_kernel_map(c["src"].to(DEV), c["dst"].to(DEV), c["offs"])
    nbr_t = ops.voxel_kernel_map(c["dst"].to(DEV), c["src"].to(DEV), -c["offs"])
    assert torch.equal(nbr.cpu(), c["nbr"]) and torch.equal(nbr_t.cpu(), c["nbr_t"])
    return nbr, nbr_t


def _run(c, maps=None, x=None, g=None):
    """(out, grad x, grad W, grad bias) of the device on case ``c`` (``x`` / ``g``: other features / output gradient)."""
    from deepviewagg_amd import ops
    nbr, nbr_t = maps if maps is not None else _device_maps(c)
    xd = (c["x"] if x is None else x).to(DEV).requires_grad_(True)
    Wd = c["W"].to(DEV).requires_grad_(True)
    bd = None if c["b"] is None else c["b"].to(DEV).requires_grad_(True)
    out = ops.sparse_conv(xd, Wd, bd, nbr, nbr_t)
    assert out.dtype == c["dtype"] and out.shape == (c["dst"].shape[0], c["cout"])
    out.backward((c["g"] if g is None else g).to(DEV))
    assert xd.grad.dtype == c["dtype"] and Wd.grad.dtype == F32
    return out.detach(), xd.grad, Wd.grad, None if bd is None else bd.grad


def _exact_gate(c, out, gx, gW, gb):
    """The kept whole-tensor statement of the fp32 path: within 2e-5 of exact float64."""
    for what, a in (("out", out), ("gx", gx), ("gW", gW), ("gb", gb)):
        if a is not None and a.numel():
            err = SR.old_metric(a.reshape(c["exact"][what].shape), c["exact"][what])
            assert err <= 2e-5, f"{c['name']} {what}: {err:.3e}"


def _cloud(spec):
    kind, n = spec
    return SR.strata_cloud(1, n) if kind == "strata" else SR.strata_cloud(1, 0)[:n]


# name -> (cloud, cin, cout, k, stride, bias, transpose, dtypes, strata every tensor must fill)
ROW_CASES = {
    # strata and the skip branch, bias on and off
    "strata_32_64": (("strata", 1500), 32, 64, 3, 1, False, False, (F32, BF16), ALL_STRATA),
    "strata_32_64_bias": (("strata", 1500), 32, 64, 3, 1, True, False, (F32, BF16), ALL_STRATA),
    # ragged channel tiles (bf16: the pad-to-16 path)
    "strata_80_48": (("strata", 1500), 80, 48, 3, 1, False, False, (F32, BF16), ALL_STRATA),
    "strata_5_7_bias": (("strata", 1500), 5, 7, 3, 1, True, False, (F32, BF16), ALL_STRATA),
    # NT = 4 in mode 0, one tile; gridDim.y = 2 with 4 input chunks; 6 input chunks at decoder width
    "s600_64_128": (("strata", 600), 64, 128, 3, 1, False, False, (F32, BF16), ()),
    "s600_256_256": (("strata", 600), 256, 256, 3, 1, False, False, (F32, BF16), ()),
    "s600_384_128": (("strata", 600), 384, 128, 3, 1, True, False, (BF16,), ()),
    "s600_144_16_k2s2": (("strata", 600), 144, 16, 2, 2, True, False, (F32,), ()),
    # weight gradient with gx >= 3 workgroups per offset (n_dst > 4096), ragged tiles
    "s6000_80_48": (("strata", 6000), 80, 48, 3, 1, False, False, (F32, BF16), ()),
    "s6000_32_64": (("strata", 6000), 32, 64, 3, 1, True, False, (F32, BF16), ()),
    # strided and transposed: n_dst != n_src in both directions
    "strata_k2s2": (("strata", 1500), 32, 48, 2, 2, False, False, (F32, BF16), ()),
    "strata_k3s2": (("strata", 1500), 32, 48, 3, 2, True, False, (F32, BF16), ()),
    "strata_k2s2_T": (("strata", 1500), 48, 32, 2, 2, False, True, (F32, BF16), ()),
    "strata_k3s2_T": (("strata", 1500), 48, 32, 3, 2, True, True, (F32, BF16), ()),
    # tiny
    "n1": (("head", 1), 32, 64, 3, 1, True, False, (F32, BF16), ()),
    "n63": (("head", 63), 32, 64, 3, 1, False, False, (F32, BF16), ()),
    "n64": (("head", 64), 32, 64, 3, 1, True, False, (F32, BF16), ()),
    "n65": (("head", 65), 32, 64, 3, 1, False, False, (F32, BF16), ()),
}


def _case(name, dtype):
    cloud, cin, cout, k, stride, bias, transpose, _, _ = ROW_CASES[name]
    tag = "fp32" if dtype == F32 else "bf16"
    return SR.conv_case(f"{name} {tag}", _cloud(cloud), cin, cout, k=k, stride=stride, bias=bias, transpose=transpose,
                        dtype=dtype, seed=len(name) + cin)


@pytest.mark.parametrize("name,dtype", [(n, dt) for n, spec in ROW_CASES.items() for dt in spec[7]],
                         ids=lambda v: v if isinstance(v, str) else str(v).split(".")[-1])
def test_rows_against_split_emulation(name, dtype):
    """Forward, input gradient, weight gradient and bias gradient, stratum by stratum; forward and input gradient are
    reproducible bit for bit (no atomics), the weight gradient (fp32 atomics) is held to its gate twice."""
    require = ROW_CASES[name][8]
    c = _case(name, dtype)
    if name == "s6000_80_48":
        assert c["dst"].shape[0] > 4096                          # >= 3 workgroups per offset in sconv_wgrad_kernel
        SR.wgrad_strata(c["nbr"], c["cin"], require=("pairs_32_2047", "pairs_ge2048"))
    if name == "n1":
        SR.wgrad_strata(c["nbr"], c["cin"], require=("pairs_1_31",))
    if ROW_CASES[name][4] == 2:
        assert c["src"].shape[0] != c["dst"].shape[0]            # strided / transposed: n_dst != n_src
    maps = _device_maps(c)
    out, gx, gW, gb = _run(c, maps)
    out2, gx2, gW2, _ = _run(c, maps)
    assert torch.equal(out, out2) and torch.equal(gx, gx2)
    rep = Report(f"sparse convolution rows: {c['name']}")
    op = _open(c["name"])
    worst = SR.gate_case(rep, c, out=out, gx=gx, gW=gW, gb=gb, require=require, require_t=require, open_findings=op)
    if dtype == F32:
        _exact_gate(c, out, gx, gW, gb)
    _finish(rep, c, worst, out, gx)
    second = Report(f"second weight gradient: {c['name']}")
    SR.gate_case(second, c, gW=gW2, open_findings=op)
    second.check()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_empty_tensors(dtype):
    """n = 0 on either side: zeros plus bias, an all-zero weight gradient, input gradients of the right shape."""
    from deepviewagg_amd import ops
    coords = SR.strata_cloud(1, 0)[:40]
    offs = O.kernel_offsets(3)
    for n_src, n_dst in ((0, 40), (40, 0), (0, 0)):
        src, dst = coords[:n_src].to(DEV), coords[:n_dst].to(DEV)
        nbr = ops.voxel_kernel_map(src, dst, offs)
        nbr_t = ops.voxel_kernel_map(dst, src, -offs)
        assert nbr.shape == (27, n_dst) and nbr_t.shape == (27, n_src) and nbr.dtype == torch.int32
        assert bool((nbr == -1).all()) and bool((nbr_t == -1).all())
        for bias in (False, True):
            x = torch.randn(n_src, 32, device=DEV).to(dtype).requires_grad_(True)
            W = torch.randn(27, 32, 48, device=DEV).requires_grad_(True)
            b = torch.randn(48, device=DEV).requires_grad_(True) if bias else None
            out = ops.sparse_conv(x, W, b, nbr, nbr_t)
            assert out.shape == (n_dst, 48) and out.dtype == dtype
            expect = torch.zeros(n_dst, 48, device=DEV) + (b.detach() if bias else 0.0)
            assert torch.equal(out.detach(), expect.to(dtype))
            g = torch.randn(n_dst, 48, device=DEV).to(dtype)
            out.backward(g)
            assert x.grad.shape == (n_src, 32) and float(x.grad.float().abs().sum()) == 0.0
            assert W.grad.shape == W.shape and float(W.grad.abs().max()) == 0.0
            if bias:
                assert torch.equal(b.grad, g.float().sum(0))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_missing_neighbours_contribute_exactly_nothing(dtype, bad):
    """Masked lanes read row 0 of ``x`` (forward, weight gradient) and of ``grad_out`` (input gradient, weight
    gradient).  With a non-finite row 0 the non-finite output rows are EXACTLY the rows whose oracle map references row
    0, and every other row is bit-identical to the run with a finite row 0 (weight gradient: fp32 atomics, so the other
    offsets are finite and meet their gate)."""
    c = _case("strata_80_48", dtype)
    maps = _device_maps(c)
    nbr, nbr_t = c["nbr"], c["nbr_t"]
    out, gx, gW, _ = _run(c, maps)
    xb, gb_ = c["x"].clone(), c["g"].clone()
    xb[0], gb_[0] = bad, bad
    out_b, _, gW_x, _ = _run(c, maps, x=xb)
    _, gx_b, gW_g, _ = _run(c, maps, g=gb_)

    def rows_check(got, healthy, touched, what):
        nonfinite = ~torch.isfinite(got.float()).all(1).cpu()
        assert torch.equal(nonfinite, touched), f"{what}: {int(nonfinite.sum())} non-finite rows, {int(touched.sum())} touched"
        assert torch.equal(got[~touched.to(got.device)], healthy[~touched.to(got.device)]), what
    touched_out = (nbr == 0).any(0)
    touched_gx = (nbr_t == 0).any(0)
    assert 1 < int(touched_out.sum()) < 28 and 1 < int(touched_gx.sum()) < 28
    rows_check(out_b, out, touched_out, "out")
    rows_check(gx_b, gx, touched_gx, "grad x")
    masks, live = SR.wgrad_strata(nbr, c["cin"])
    for gWb, touched_k, what in ((gW_x, (nbr == 0).any(1), "grad W, x row 0"), (gW_g, nbr[:, 0] >= 0, "grad W, g row 0")):
        assert 0 < int(touched_k.sum()) < 27
        nonfinite_k = ~torch.isfinite(gWb).flatten(1).all(1).cpu()
        assert torch.equal(nonfinite_k, touched_k), what
        all_bad = (~torch.isfinite(gWb)).flatten(1).all(1).cpu()
        assert torch.equal(all_bad, touched_k), what              # every entry of a touched offset, none elsewhere
        keep = live & ~touched_k.repeat_interleave(c["cin"])
        rep = Report(f"{what}: the other offsets")
        clean = torch.where(torch.isfinite(gWb), gWb, torch.zeros_like(gWb)).reshape(-1, c["cout"]).cpu()
        err = RW.row_err(clean, c["gW64"].reshape(-1, c["cout"]), keep)
        noise = RW.row_err(c["gW32"].reshape(-1, c["cout"]), c["gW64"].reshape(-1, c["cout"]), keep)
        RW.gate_rows(rep, c["name"], what, err, noise, {}, keep)
        rep.check()


# ---- kernel maps, bit-exact against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("duplicates", [False, True], ids=["unique", "duplicates"])
def test_kernel_map_table_capacity_edges(duplicates):
    """n_src around the steps of the table capacity (next power of two >= 2 n_src, at least 64: 32 -> 33, 64 -> 65),
    dst != src, destinations without any neighbour, negative coordinates, equal coordinates in two batch items,
    duplicate source rows (the smallest id wins)."""
    from deepviewagg_amd import ops
    offs = O.kernel_offsets(3)
    for n_src in SR.MAP_SIZES:
        src, dst = SR.map_cloud(n_src, seed=n_src, duplicates=duplicates)
        nbr = ops.voxel_kernel_map(src.to(DEV), dst.to(DEV), offs)
        ref = O.kernel_map_sorted(src, dst, offs)
        assert torch.equal(nbr.cpu(), ref), n_src
        assert torch.equal(ops.voxel_kernel_map(dst.to(DEV), src.to(DEV), -offs).cpu(),
                           O.kernel_map_sorted(dst, src, -offs)), n_src
        if n_src >= 31:
            assert bool((ref >= 0).any()) and bool((ref < 0).all(0).any()) and bool((src[:, 3] == 1).any())


@pytest.mark.parametrize("k,ts,dilation", [(3, 2, 1), (3, 4, 1), (2, 2, 1), (2, 4, 1), (3, 1, 2), (3, 2, 2)])
def test_kernel_map_at_tensor_stride_and_dilation(k, ts, dilation):
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d.nn import kernel_offsets
    src, dst = SR.map_cloud(700, seed=k + ts + dilation, stride=ts)
    offs = kernel_offsets(k, ts, dilation)
    assert np.array_equal(offs, O.kernel_offsets(k, ts, dilation)) and int(np.abs(offs).max()) == ts * dilation
    nbr = ops.voxel_kernel_map(src.to(DEV), dst.to(DEV), offs)
    ref = O.kernel_map_sorted(src, dst, offs)
    assert torch.equal(nbr.cpu(), ref) and torch.equal(ref, O.kernel_map(src, dst, offs)) and bool((ref >= 0).any())
    coords = SR.strata_cloud(1, 1500, stride=ts)
    nbr = ops.voxel_kernel_map(coords.to(DEV), coords.to(DEV), offs)
    assert torch.equal(nbr.cpu(), O.kernel_map_sorted(coords, coords, offs))


@pytest.mark.parametrize("s", [1, 2])
def test_conv3d_build_caches_the_flipped_map(s):
    """Conv3d._build at k3 s1 takes ``nbr_t = flip(nbr)`` instead of a second query: equal to the query, and to the
    oracle, also with duplicate-free coordinates at tensor stride 2."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    coords = SR.strata_cloud(1, 1500, stride=s)
    x = snn.SparseVoxelTensor(torch.zeros(coords.shape[0], 4, device=DEV), coords.to(DEV), stride=s)
    key = (s, 3, 1, 1)
    snn.Conv3d._build(x, key, s)
    nbr, nbr_t = x.kernel_maps[key]
    offs = snn.kernel_offsets(3, s, 1)
    assert torch.equal(x.coord_maps[s], x.C)
    assert torch.equal(nbr_t, ops.voxel_kernel_map(x.C, x.C, -offs))
    assert torch.equal(nbr.cpu(), O.kernel_map_sorted(coords, coords, offs))
    assert torch.equal(nbr_t.cpu(), O.kernel_map_sorted(coords, coords, -offs))
    conv = snn.Conv3d(4, 8, kernel_size=3).to(DEV)
    got = conv._maps(x)
    assert got[0] is nbr and got[1] is nbr_t and got[3] == s


def test_kernel_map_200k_sorted_and_shuffled_halves():
    from deepviewagg_amd import ops
    c = SR.surface_part(300000, 200, seed=9, batches=2, lo=-100)
    assert c.shape[0] > 200000
    half = c.shape[0] // 2
    head = c[:half]
    c[:half] = head[np.lexsort((head[:, 0], head[:, 1], head[:, 2], head[:, 3]))]
    coords = torch.from_numpy(c.astype(np.int32))
    offs = O.kernel_offsets(3)
    nbr = ops.voxel_kernel_map(coords.to(DEV), coords.to(DEV), offs)
    ref = O.kernel_map_sorted(coords, coords, offs)
    assert torch.equal(nbr.cpu(), ref) and int((ref >= 0).sum()) > 3 * coords.shape[0]
    dst = O.downsample_coords(coords, 2)
    offs2 = O.kernel_offsets(2)
    assert torch.equal(ops.voxel_kernel_map(coords.to(DEV), dst.to(DEV), offs2).cpu(), O.kernel_map_sorted(coords, dst, offs2))
    assert torch.equal(ops.voxel_kernel_map(dst.to(DEV), coords.to(DEV), -offs2).cpu(),
                       O.kernel_map_sorted(dst, coords, -offs2))


# ---- the module's K = 1 path and the autocast dispatch ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_strided_1x1x1_through_the_module(dtype):
    """Conv3d(kernel_size=1, stride=2): a [Cin, Cout] kernel run at K = 1 over the map of the voxels that sit on the
    coarse grid."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    tag = "fp32" if dtype == F32 else "bf16"
    c = SR.conv_case(f"module_k1s2_48_80 {tag}", SR.strata_cloud(1, 1500), 48, 80, k=1, stride=2, bias=True, dtype=dtype,
                     seed=77)
    assert c["K"] == 1 and 0 < int((c["nbr"] >= 0).sum()) < c["src"].shape[0] and c["dst"].shape[0] < c["src"].shape[0]
    conv = snn.Conv3d(48, 80, kernel_size=1, stride=2, bias=True).to(DEV)
    assert conv.kernel.shape == (48, 80)
    with torch.no_grad():
        conv.kernel.copy_(c["W"][0])
        conv.bias.copy_(c["b"])
    x = snn.SparseVoxelTensor(c["x"].to(DEV).requires_grad_(True), c["src"].to(DEV))
    y = conv(x)
    assert y.s == 2 and torch.equal(y.C.cpu(), c["dst"]) and y.F.dtype == dtype
    nbr, nbr_t = x.kernel_maps[(1, 1, 2, 1)]
    assert torch.equal(nbr.cpu(), c["nbr"]) and torch.equal(nbr_t.cpu(), c["nbr_t"])
    y.F.backward(c["g"].to(DEV))
    rep = Report(f"sparse convolution rows: {c['name']}")
    gW = conv.kernel.grad.unsqueeze(0)
    worst = SR.gate_case(rep, c, out=y.F.detach(), gx=x.F.grad, gW=gW, gb=conv.bias.grad,
                         open_findings=_open(c["name"]))
    if dtype == F32:
        _exact_gate(c, y.F.detach(), x.F.grad, gW, conv.bias.grad)
    _finish(rep, c, worst, y.F.detach(), x.F.grad)


@pytest.mark.parametrize("amp", [BF16, torch.float16], ids=["autocast_bf16", "autocast_fp16"])
def test_autocast_dispatch(amp):
    """fp32 features under autocast(bfloat16) run the bf16 kernels (bf16 output, the bf16 gate); the kernels have no
    fp16 form, so under autocast(float16) the convolution stays fp32 (the fp32 gate)."""
    from deepviewagg_amd import ops
    kind = BF16 if amp == BF16 else F32
    base = _case("strata_32_64_bias", kind)
    c = dict(base, name=f"{base['name']} under autocast({str(amp).split('.')[-1]})")
    nbr, nbr_t = _device_maps(c)
    xd = c["x"].float().to(DEV).requires_grad_(True)            # the bf16 case's features are bf16 values: exact in fp32
    Wd, bd = c["W"].to(DEV).requires_grad_(True), c["b"].to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=amp):
        out = ops.sparse_conv(xd, Wd, bd, nbr, nbr_t)
    assert out.dtype == kind
    out.backward(c["g"].to(DEV))
    assert xd.grad.dtype == F32 and Wd.grad.dtype == F32
    rep = Report(f"sparse convolution rows: {c['name']}")
    worst = SR.gate_case(rep, c, out=out.detach(), gx=xd.grad.to(kind), gW=Wd.grad, gb=bd.grad,
                         open_findings=_open(base["name"]))      # the same numbers as without autocast
    _finish(rep, c, worst, out.detach(), xd.grad.to(kind))
