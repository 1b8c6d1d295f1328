"""CPU tests of the sparse-convolution oracle and of the host logic of modules/SparseConv3d (no GPU):
the gather-GEMM-scatter restatement against torch's dense conv3d on the densified grid, kernel offsets,
coordinate downsampling, state-dict layout of the residual stages."""
import numpy as np
import torch

from oracle import sparseconv_oracle as O


def _cloud(n=300, extent=12, stride=1, seed=0):
    rng = np.random.default_rng(seed)
    xyz = np.unique(rng.integers(0, extent, size=(n, 3)), axis=0) * stride
    return torch.from_numpy(np.concatenate([xyz, np.zeros((xyz.shape[0], 1), dtype=np.int64)], 1).astype(np.int32))


def test_kernel_offsets_layout():
    o3 = O.kernel_offsets(3)
    assert o3.shape == (27, 3) and o3[0].tolist() == [-1, -1, -1] and o3[1].tolist() == [0, -1, -1]
    assert o3[13].tolist() == [0, 0, 0]
    o2 = O.kernel_offsets(2, tensor_stride=2)
    assert o2.tolist() == [[0, 0, 0], [0, 0, 2], [0, 2, 0], [0, 2, 2], [2, 0, 0], [2, 0, 2], [2, 2, 0], [2, 2, 2]]


def test_oracle_matches_dense_conv3d_stride1():
    torch.manual_seed(0)
    coords = _cloud()
    x = torch.randn(coords.shape[0], 5, dtype=torch.float64)
    W = torch.randn(27, 5, 7, dtype=torch.float64)
    nbr = O.kernel_map(coords, coords, O.kernel_offsets(3))
    out = O.sparse_conv(x, W, None, nbr)
    ref, _ = O.dense_reference(x, coords, W, 3)
    assert torch.allclose(out, ref, atol=1e-10)
    # same voxels on both sides + point-symmetric offsets: the transposed map is the map in reverse offset order
    assert torch.equal(O.kernel_map(coords, coords, -O.kernel_offsets(3)), torch.flip(nbr, [0]))


def test_oracle_matches_dense_conv3d_strided_and_transposed():
    torch.manual_seed(1)
    coords = _cloud(seed=3)
    x = torch.randn(coords.shape[0], 4, dtype=torch.float64)
    W = torch.randn(8, 4, 6, dtype=torch.float64)
    oc = O.downsample_coords(coords, 2)
    assert oc.shape[0] < coords.shape[0] and (np.asarray(oc)[:, :3] % 2 == 0).all()
    offs = O.kernel_offsets(2)
    nbr = O.kernel_map(coords, oc, offs)
    assert int((nbr >= 0).sum()) == coords.shape[0]            # every input voxel has exactly one parent slot
    out = O.sparse_conv(x, W, None, nbr)
    ref, oc_ref = O.dense_reference(x, coords, W, 2, stride=2)
    assert torch.equal(oc_ref, oc) and torch.allclose(out, ref, atol=1e-10)
    # transposed convolution back to the fine voxels: the same pairs, source and destination swapped
    Wt = torch.randn(8, 6, 3, dtype=torch.float64)
    nbr_t = O.kernel_map(oc, coords, -offs)
    up = O.sparse_conv(out, Wt, None, nbr_t)
    ref_up, _ = O.dense_reference(out, oc, Wt, 2, stride=2, tensor_stride=2, transpose=True, out_coords=coords)
    assert torch.allclose(up, ref_up, atol=1e-10)
    # the transposed map is the inverse relation of the forward map
    k, j = torch.nonzero(nbr >= 0, as_tuple=True)
    assert torch.equal(nbr_t[k, nbr[k, j].long()].long(), j)


def test_downsample_order_and_module_host_logic():
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    from deepviewagg_amd.modules.SparseConv3d import ResNetDown, ResNetUp, BottleneckBlock
    coords = _cloud(seed=5)
    coords[::3, 3] = 1                                          # two batch items
    a, b = snn.downsample_coords(coords, 4), O.downsample_coords(coords, 4)
    assert torch.equal(a, b)
    assert np.array_equal(snn.kernel_offsets(3, 2), O.kernel_offsets(3, 2))
    assert np.array_equal(snn.kernel_offsets(2, 1), O.kernel_offsets(2, 1))
    down = ResNetDown(down_conv_nn=[16, 32], N=2)
    keys = list(down.state_dict())
    assert keys[0] == "conv_in.0.kernel" and "conv_in.1.bn.running_mean" in keys
    assert "blocks.0.downsample.0.kernel" in keys and "blocks.1.block.3.kernel" in keys
    assert "blocks.1.downsample.0.kernel" not in keys
    assert down.conv_in[0].kernel.shape == (8, 16, 16) and down.blocks[0].block[0].kernel.shape == (27, 16, 32)
    up = ResNetUp(up_conv_nn=[32, 16, 24], N=1)
    assert up.conv_in[0].kernel.shape == (8, 32, 32) and up.blocks[0].block[0].kernel.shape == (27, 48, 24)
    up1 = ResNetUp(up_conv_nn=[[48, 24]], N=0, skip_first=True)
    assert up1.conv_in[0].kernel.shape == (8, 48, 24) and up1.blocks is None
    bt = BottleneckBlock(32, 64, snn.Conv3d)
    assert bt.block[0].kernel.shape == (32, 16) and bt.block[3].kernel.shape == (27, 16, 16)
    try:
        ResNetDown(down_conv_nn=[1, 2, 3])
        assert False
    except AssertionError:
        pass


def test_cpu_twin_of_a_stage_runs_on_the_oracle(monkeypatch):
    """The GPU parity test evaluates the CPU twin of a block by swapping ``ops`` for the oracle inside nn.py;
    check here that this twin works (forward + backward, encoder and decoder)."""
    from deepviewagg_amd.modules.SparseConv3d import nn as snn
    from deepviewagg_amd.modules.SparseConv3d import ResNetDown, ResNetUp
    monkeypatch.setattr(snn, "ops", O.OracleOps)
    monkeypatch.setattr(snn, "batchnorm_act_rows", O.batchnorm_act_rows)
    torch.manual_seed(0)
    coords = _cloud(seed=7)
    x = snn.SparseVoxelTensor(torch.randn(coords.shape[0], 8, requires_grad=True), coords)
    down, up = ResNetDown(down_conv_nn=[8, 16], N=1), ResNetUp(up_conv_nn=[16, 8, 12], N=1)
    y = down(x)
    assert y.s == 2 and y.C.shape[0] == O.downsample_coords(coords, 2).shape[0] and y.F.shape[1] == 16
    z = up(y, x)
    assert z.s == 1 and torch.equal(z.C, coords) and z.F.shape == (coords.shape[0], 12)
    z.F.square().mean().backward()
    assert x.F.grad is not None and down.conv_in[0].kernel.grad.abs().sum() > 0


# ---- the additions the row-wise GPU tests stand on (tests/sparse_rows.py) --------------------------------------------
import pytest                                                   # noqa: E402

import sparse_rows as SR                                        # noqa: E402


@pytest.mark.parametrize("n_src", SR.MAP_SIZES)
@pytest.mark.parametrize("duplicates", [False, True])
def test_sorted_kernel_map_matches_dict_version(n_src, duplicates):
    """src != dst, destinations without any neighbour, negative coordinates, equal coordinates in two batch items,
    duplicate source rows (smallest row wins), both directions."""
    src, dst = SR.map_cloud(n_src, seed=n_src, duplicates=duplicates)
    offs = O.kernel_offsets(3)
    nbr = O.kernel_map_sorted(src, dst, offs)
    assert nbr.dtype == torch.int32 and torch.equal(nbr, O.kernel_map(src, dst, offs))
    assert torch.equal(O.kernel_map_sorted(dst, src, -offs), O.kernel_map(dst, src, -offs))
    if n_src >= 31:
        assert bool((nbr >= 0).any()) and bool((nbr < 0).all(0).any())          # hits, and rows without any
    if duplicates and n_src >= 31:
        assert np.unique(src.numpy(), axis=0).shape[0] < n_src
    if n_src >= 2:                                              # never across the batch column
        k, j = torch.nonzero(nbr >= 0, as_tuple=True)
        assert torch.equal(src[nbr[k, j].long(), 3], dst[j, 3]) and bool((src[:, 3] == 1).any())


@pytest.mark.parametrize("k,stride,ts,dilation", [(3, 1, 1, 1), (2, 2, 1, 1), (3, 2, 1, 1), (3, 1, 2, 1), (2, 2, 4, 1),
                                                   (3, 1, 1, 2)])
def test_sorted_kernel_map_on_the_strata_cloud(k, stride, ts, dilation):
    coords = SR.strata_cloud(1, 1500, stride=ts)
    dst = coords if stride == 1 else O.downsample_coords(coords, ts * stride)
    offs = O.kernel_offsets(k, ts, dilation)
    assert torch.equal(O.kernel_map_sorted(coords, dst, offs), O.kernel_map(coords, dst, offs))
    assert torch.equal(O.kernel_map_sorted(dst, coords, -offs), O.kernel_map(dst, coords, -offs))
    assert torch.equal(O.kernel_map_sorted(coords[:0], dst, offs), torch.full((k ** 3, dst.shape[0]), -1).int())
    assert O.kernel_map_sorted(coords, dst[:0], offs).shape == (k ** 3, 0)


def test_strata_cloud_fills_every_stratum():
    coords = SR.strata_cloud(1, 1500)
    n_struct = SR.structured_part().shape[0]
    head = coords[:n_struct].long()
    key = ((head[:, 3] * 4096 + head[:, 2]) * 4096 + head[:, 1]) * 4096 + head[:, 0]
    assert bool((key[1:] > key[:-1]).all())                     # the structured part is sorted ascending (b, z, y, x)
    _, _, nbr, _ = SR.maps(coords)
    s = SR.conv_strata(nbr, require=("nbr_1", "nbr_2_8", "nbr_9_26", "nbr_27", "tile_edge", "last_tile", "wave_skips",
                                     "wave_no_skip"))
    assert int(s["nbr_1"].sum()) >= 70 and int(s["nbr_27"].sum()) == 128 and not bool(s["nbr_0"].any())
    skipped = SR.skipped_offsets(nbr)
    assert 24 in skipped and 18 in skipped and 0 in skipped     # line, plane, block / surface
    # the surface part alone, shuffled: a block misses a corner offset at most (the earlier clouds hardly reached the
    # branch, and never with most offsets skipped)
    _, _, nbr_s, _ = SR.maps(coords[n_struct:])
    assert max(SR.skipped_offsets(nbr_s)[:-1]) <= 2


@pytest.mark.parametrize("k,stride,transpose", [(3, 1, False), (2, 2, False), (3, 2, True)])
def test_split_statement_is_the_old_gate(k, stride, transpose):
    """float64 evaluation of the 3-term split against exact float64: inside the 2e-5 the GPU tests hold the kernel to
    (now a statement about the algorithm), forward and the explicit statements of the device's backward against
    float64 autograd of the exact oracle."""
    c = SR.conv_case(f"oracle_k{k}s{stride}t{int(transpose)}", SR.strata_cloud(1, 1500), 96, 64, k=k, stride=stride,
                     bias=True, transpose=transpose)
    for key, ex in (("out64", "out"), ("gx64", "gx"), ("gW64", "gW")):
        err = SR.old_metric(c[key], c["exact"][ex])
        assert 1e-7 < err <= 2e-5, (key, err)                   # and it IS a different function: the lo lo term is gone
    assert SR.old_metric(c["gb64"], c["exact"]["gb"]) <= 1e-12


def test_split_bf16_and_autograd():
    t = torch.randn(1000, dtype=torch.float64)
    hi, lo = O.split_bf16(t)
    assert hi.dtype == lo.dtype == torch.float64
    assert torch.equal(hi, t.bfloat16().double()) and torch.equal(lo, (t - hi).bfloat16().double())
    assert float((t - hi - lo).abs().max()) <= 2.0 ** -16 * float(t.abs().max())
    h32, l32 = O.split_bf16(t.float())
    assert h32.dtype == torch.float32 and torch.equal(h32, t.float().bfloat16().float())
    coords = SR.strata_cloud(1, 0)
    _, _, nbr, _ = SR.maps(coords)
    x = torch.randn(coords.shape[0], 8, dtype=torch.float64, requires_grad=True)
    W = torch.randn(27, 8, 4, dtype=torch.float64, requires_grad=True)
    O.sparse_conv_split(x, W, None, nbr).sum().backward()
    assert x.grad is not None and W.grad is not None and float(x.grad.abs().max()) > 0
    a = O.sparse_conv_split(x.detach(), W.detach(), None, nbr)
    b = O.sparse_conv_split(x.detach(), W.detach(), None, nbr, order="hl,lh,hh")
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
