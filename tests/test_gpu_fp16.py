"""-m gpu: float16 storage (DVA_F16) on the gather and view-pooling path, under torch.autocast(float16).

The score chain keeps bf16 operands with fp32 accumulation under fp16 autocast (its gradient rows carry the GradScaler
factor), so the chain is gated with the bf16 yardstick of tests/test_gpu_chain.py: the fp32 oracle, and the oracle's
own error under CPU autocast(bfloat16).  Value rows, pooled features and the rows gradient are fp16; their rounding is
checked bit for bit against torch."""
import ctypes

import pytest
import torch

from oracle import pooling_oracle as O
from test_gpu_chain import (DEV, _oracle_grads, build, check_plan_kind, check_rows_against_autocast, full32,  # noqa: F401
                            make_case, plan_kind, ragged, ragged_long, rel)

pytestmark = pytest.mark.gpu


def run_dev(case, m, dtype, need_grad=True):
    """tests/test_gpu_chain.run_dev with the autocast dtype (and the map stored in it) as a parameter."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    V = case["V"]
    xd = case["x"].to(DEV).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(need_grad)
    packed = ops.pack_gather_index(case["images"].to(DEV), torch.arange(V + 1, device=DEV), case["pixels"].to(DEV))
    with torch.autocast("cuda", dtype=dtype):
        lazy = ops.lazy_gather_nearest(xd, packed, exact=True)
        lazy = P.BimodalCSRPool(mode='max')(None, lazy, None, torch.arange(V + 1, device=DEV))
        out = m(None, lazy, case["x_map"].to(DEV), case["csr"].to(DEV))
    grads = None
    if need_grad:
        grads = torch.autograd.grad((out.float() * case["w"].to(DEV)).sum(), [xd] + list(m.parameters()),
                                    allow_unused=True)
    return out, grads


@pytest.fixture
def chain_calls():
    """Counts the fp16 launches of the chain's view kernels (the chain, not the generic path, must be what ran)."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    calls = {"fwd": 0, "bwd": 0}
    orig = {k: getattr(lib, k) for k in ("dva_chain_attn_fwd_dt", "dva_chain_attn_bwd_dt")}

    def wrap(name, key):
        def f(*a):
            calls[key] += a[-2] == _lib.DVA_F16
            return orig[name](*a)
        return f
    lib.dva_chain_attn_fwd_dt = wrap("dva_chain_attn_fwd_dt", "fwd")
    lib.dva_chain_attn_bwd_dt = wrap("dva_chain_attn_bwd_dt", "bwd")
    try:
        yield calls
    finally:
        for k, v in orig.items():
            setattr(lib, k, v)


def test_gather_nearest_fp16_is_bit_exact():
    from deepviewagg_amd import ops
    gen = torch.Generator().manual_seed(0)
    B, C, H, W, V = 2, 64, 9, 13, 500
    x = (torch.randn(B, C, H, W, generator=gen) * 300).half()
    x.view(-1)[:4] = torch.tensor([65504.0, -65504.0, 6.0e-8, -0.0]).half()
    images = torch.randint(0, B, (V,), generator=gen)
    px = torch.randint(0, W, (V,), generator=gen)
    py = torch.randint(0, H, (V,), generator=gen)
    packed = ops.pack_gather_index(images.to(DEV), torch.arange(V + 1, device=DEV),
                                   torch.stack([px, py], 1).short().to(DEV))
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    got = ops.gather_nearest(xd, packed)
    want = x.permute(0, 2, 3, 1)[images, py, px]
    assert got.dtype == torch.float16
    assert torch.equal(got.cpu().view(torch.int16), want.contiguous().view(torch.int16))


def test_chain_rows_gradient_rounds_once_to_nearest_even(plan_kind, chain_calls):
    """Gating off, every point has one view and every map row is read by exactly two points: the attention is exactly 1
    and the gradient of the value rows is a + b summed in fp32 and rounded once -- torch's (a.float() + b.float()).half()
    bit for bit, ties to even and overflow to +inf included.  The chain is called on the rows themselves (fused_chain.chain_pool:
    the value rows are E_mod's output in the module), so the map gradient IS the chain's rows gradient."""
    from deepviewagg_amd import fused_chain, ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    C, G, H, W = 64, 4, 16, 40            # 640 map rows: inside the split plan's range (512, 2^18]
    R = H * W
    gen = torch.Generator().manual_seed(1)
    N = V = 2 * R
    perm = torch.randperm(R, generator=gen)
    row = torch.cat([perm, perm])[torch.randperm(V, generator=gen)]          # each row twice, shuffled
    pixels = torch.stack([row % W, row // W], 1).short()
    m = P.GroupBimodalCSRPool(in_map=8, in_mod=C, num_groups=G, use_num=True, gating=False).to(DEV).train()
    x = torch.randn(1, C, H, W, generator=gen).half().to(DEV).contiguous(memory_format=torch.channels_last)
    x.requires_grad_()
    packed = ops.pack_gather_index(torch.zeros(V, dtype=torch.long, device=DEV), torch.arange(V + 1, device=DEV),
                                   pixels.to(DEV))
    with torch.autocast("cuda", dtype=torch.float16):
        lazy = ops.lazy_gather_nearest(x, packed, exact=True)
        out = fused_chain.chain_pool(m, lazy, torch.rand(V, 8, generator=gen).to(DEV), torch.arange(V + 1, device=DEV))
    assert out.dtype == torch.float16
    # the pooled rows are the value rows themselves (attention 1, no gate): the view kernel's fp16 stores
    want_out = x.detach().permute(0, 2, 3, 1).reshape(R, C)[row.to(DEV)]
    assert torch.equal(out.detach().view(torch.int16), want_out.view(torch.int16))
    gout = (torch.randn(N, C, generator=gen) * 4).half()
    pairs = {}
    for v in range(V):
        pairs.setdefault(int(row[v]), []).append(v)
    pairs = list(pairs.values())
    cases = [(1.0, 2.0 ** -11), (1.0 + 2.0 ** -10, 2.0 ** -11), (65504.0, 16.0)]
    for k, (a, b) in enumerate(cases):
        gout[pairs[k][0], :] = a
        gout[pairs[k][1], :] = b
    (g,) = torch.autograd.grad(out, x, grad_outputs=gout.to(DEV))
    check_plan_kind(plan_kind, C)
    assert chain_calls["fwd"] >= 1 and chain_calls["bwd"] >= 1
    assert g.dtype == torch.float16
    want = torch.zeros(R, C, dtype=torch.float32)
    want.index_add_(0, row, gout.float())
    want = want.half()
    got = g.detach().permute(0, 2, 3, 1).reshape(R, C).cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    r0, r1, r2 = (int(row[pairs[k][0]]) for k in range(3))
    assert float(got[r0, 0]) == 1.0                                  # 1 + 2^-11: tie, to even
    assert float(got[r1, 0]) == 1.0 + 2.0 ** -9                      # (1 + 2^-10) + 2^-11: tie, to even
    assert got[r2, 0].isinf() and float(got[r2, 0]) > 0              # 65504 + 16: +inf


def test_segment_max_and_bilinear_gather_fp16_match_their_fp32_upcast():
    """The non-exact gather + atomic max pool (dva_gather_segment_reduce_*) and the bilinear gather (dva_gather_bilinear_*,
    backward through dva_gather_rows_sum) on an fp16 map against the same ops on its fp32 upcast."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    gen = torch.Generator().manual_seed(4)
    B, C, H, W, V = 3, 64, 12, 20, 2000
    atoms = torch.randint(1, 6, (V,), generator=gen)
    atom_ptr = torch.cat([torch.zeros(1, dtype=torch.long), atoms.cumsum(0)]).to(DEV)
    Pn = int(atom_ptr[-1])
    images = torch.randint(0, B, (V,), generator=gen).to(DEV)
    pixels = torch.stack([torch.randint(0, W, (Pn,), generator=gen), torch.randint(0, H, (Pn,), generator=gen)],
                         1).short().to(DEV)
    x16 = torch.randn(B, C, H, W, generator=gen).half().to(DEV).contiguous(memory_format=torch.channels_last)
    w = torch.randn(V, C, generator=gen).to(DEV)
    res = []
    for x0 in (x16, x16.float().contiguous(memory_format=torch.channels_last)):
        x = x0.detach().clone().requires_grad_()
        lazy = ops.lazy_gather_nearest_mapping(x, images, atom_ptr, pixels, 1.0, exact=False)
        pooled = P.BimodalCSRPool(mode='max')(None, lazy, None, atom_ptr)
        assert isinstance(pooled, ops.GatheredFeatures)           # the fused gather + segment max ran
        vals = pooled.materialize()
        (gx,) = torch.autograd.grad((vals.float() * w).sum(), x)
        res.append((vals, gx))
    (vh, gh), (vf, gf) = res
    assert vh.dtype == torch.float16 and gh.dtype == torch.float16
    assert torch.equal(vh.float(), vf)                            # a max selects a value: exact
    assert rel(gh, gf) <= 2e-3
    # bilinear gather, forward + backward
    packed = ops.pack_gather_index(images, torch.arange(V + 1, device=DEV), pixels[:V])
    coords = torch.rand(V, 2, generator=gen).to(DEV)
    res = []
    for x0 in (x16, x16.float().contiguous(memory_format=torch.channels_last)):
        x = x0.detach().clone().requires_grad_()
        y = ops.gather_bilinear(x, packed, coords)
        (gx,) = torch.autograd.grad((y.float() * w).sum(), x)
        res.append((y, gx))
    (yh, gh), (yf, gf) = res
    assert yh.dtype == torch.float16 and gh.dtype == torch.float16
    assert rel(yh, yf) <= 2e-3 and rel(gh, gf) <= 2e-3


def _branch_fp16(name, C_mod):
    """UnimodalBranch of the golden fixture ``name`` (the reference's fp32 run) under autocast(float16)."""
    from conftest import load_golden, state_dict_from, t
    from test_gpu_data import Conv, make_image_data
    from deepviewagg_amd import fused_bilinear, ops
    from deepviewagg_amd.core.multimodal.image import ImageData
    from deepviewagg_amd.modules.multimodal import (UnimodalBranch, BimodalCSRPool, GroupBimodalCSRPool,
                                                    BimodalFusion)
    g = load_golden(name)
    n_set = int(g["n_settings"])
    xs = [t(g[f"s{i}_x_img"], DEV).requires_grad_() for i in range(n_set)]
    sds = [make_image_data(g, f"s{i}_", xs[i], g[f"s{i}_ref_size"], DEV) for i in range(n_set)]
    conv = Conv(6, C_mod)
    conv.load_state_dict(state_dict_from(g, "sd_conv/"))
    pool = GroupBimodalCSRPool(in_map=8, in_mod=C_mod, num_groups=4, use_num=True)
    pool.load_state_dict(state_dict_from(g, "sd_pool/"))
    branch = UnimodalBranch(conv, BimodalCSRPool(mode="max"), pool, BimodalFusion(mode="concatenation"),
                            interpolate="bilinear" in name).to(DEV).train()
    x_3d = t(g["x_3d"], DEV).requires_grad_()
    calls = {"materialize": 0, "fused": 0}
    orig_mat, orig_pool = ops.InterpolatedFeatures.materialize, fused_bilinear.pool

    def mat(self, *a, **k):
        calls["materialize"] += 1
        return orig_mat(self, *a, **k)

    def fpool(*a, **k):
        calls["fused"] += 1
        return orig_pool(*a, **k)
    ops.InterpolatedFeatures.materialize, fused_bilinear.pool = mat, fpool
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            y = branch({"x_3d": x_3d, "x_seen": None, "modalities": {"image": ImageData(sds)}}, "image")["x_3d"]
        grads = torch.autograd.grad((y.float() * t(g["w"], DEV)).sum(), xs + [x_3d])
    finally:
        ops.InterpolatedFeatures.materialize, fused_bilinear.pool = orig_mat, orig_pool
    return g, y, grads, calls


@pytest.mark.parametrize("name,C_mod", [("branch_nearest", 8), ("branch_bilinear", 8), ("branch_bilinear_c32", 32)])
def test_unimodal_branch_generic_paths_under_fp16_autocast(name, C_mod):
    """The generic HIP paths under autocast(float16) against the reference's fp32 run: BimodalCSRPool + GroupBimodalCSRPool
    on the nearest gather (C = 8: no chain instantiation), the bilinear gather with the fused path not applicable (fp16
    rows), two settings concatenated by InterpolatedFeatures.cat (branch_bilinear_c32).  Gates: output 2e-2, gradients 5e-2
    relative L2 (the bf16 floors of DESIGN section 2)."""
    g, y, grads, calls = _branch_fp16(name, C_mod)
    assert calls["fused"] == 0
    if "bilinear" in name:
        assert calls["materialize"] >= 1
    assert rel(y, torch.as_tensor(g["out"])) <= 2e-2
    n_set = int(g["n_settings"])
    for i in range(n_set):
        assert torch.isfinite(grads[i]).all()
        assert rel(grads[i], torch.as_tensor(g[f"s{i}_grad_x_img"])) <= 5e-2, i
    assert rel(grads[-1], torch.as_tensor(g["grad_x_3d"])) <= 5e-2


@pytest.mark.parametrize("cls_name", ["QKVBimodalCSRPool", "BimodalCSRPool"])
def test_lazy_pools_under_fp16_autocast_match_oracle(cls_name):
    """QKVBimodalCSRPool (its key kernel is bf16-only: under float16 the compatibilities come from the generic path) and the
    view-level BimodalCSRPool('max') on a lazily gathered fp16 map, against the fp32 oracle at the bf16 gates."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    gen = torch.Generator().manual_seed(3)
    N, C, B, H, W = 3000, 32, 3, 12, 20
    sizes = torch.randint(0, 7, (N,), generator=gen)
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    V = int(csr[-1])
    images = torch.randint(0, B, (V,), generator=gen)
    pixels = torch.stack([torch.randint(0, W, (V,), generator=gen), torch.randint(0, H, (V,), generator=gen)], 1).short()
    x = torch.randn(B, C, H, W, generator=gen).half().float()
    x_map = torch.rand(V, 8, generator=gen)
    x_main = torch.randn(N, 6, generator=gen)
    w = torch.randn(N, C, generator=gen)
    if cls_name == "QKVBimodalCSRPool":
        kwargs = dict(in_map=8, in_mod=C, num_groups=4, use_num=True, in_main=6, nc_qk=4)
        ref = O.QKVBimodalCSRPool(**kwargs)
        with torch.no_grad():
            for p in ref.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.4)
        m = P.QKVBimodalCSRPool(**kwargs)
        m.load_state_dict(ref.state_dict(), strict=True)
        m = m.to(DEV).train()
    else:
        ref, m = torch.nn.Module(), P.BimodalCSRPool(mode='max')
        ref.forward = lambda x_main_, x_mod, x_map_, csr_: O.bimodal_csr_pool(x_mod, csr_, mode='max')

    def oracle(autocast):
        xr = x.clone().requires_grad_()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            out = ref(x_main, O.gather_nearest(xr, images, pixels), x_map, csr)
        params = [p for p in ref.parameters()]
        return out, torch.autograd.grad((out.float() * w).sum(), [xr] + params, allow_unused=True)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    out_ref, g_ref = oracle(False)
    ref.load_state_dict(sd)
    out_amp, g_amp = oracle(True)
    xd = x.to(DEV).half().contiguous(memory_format=torch.channels_last).requires_grad_()
    packed = ops.pack_gather_index(images.to(DEV), torch.arange(V + 1, device=DEV), pixels.to(DEV))
    with torch.autocast("cuda", dtype=torch.float16):
        lazy = ops.lazy_gather_nearest(xd, packed, exact=True)
        lazy = P.BimodalCSRPool(mode='max')(None, lazy, None, torch.arange(V + 1, device=DEV))
        out = m(x_main.to(DEV), lazy, x_map.to(DEV), csr.to(DEV))
    if isinstance(out, ops.GatheredFeatures):
        out = out.materialize()
    g = torch.autograd.grad((out.float() * w.to(DEV)).sum(), [xd] + list(m.parameters()), allow_unused=True)
    assert out.dtype == torch.float16
    assert rel(out, out_ref) <= max(2e-2, 1.5 * rel(out_amp, out_ref))
    names = ["x"] + [n for n, _ in ref.named_parameters()]
    bad = []
    for n, a, b, c in zip(names, g, g_ref, g_amp):
        if b is None:
            continue
        ours, amp = rel(a, b), rel(c, b)
        if ours > max(4.0 * amp, 5e-2):
            bad.append((n, ours, amp))
    assert not bad, bad


def test_multimodal_encoder_decoder_fp16_amp_training_step():
    """After dropin.install(): the multimodal encoder (ResNetDown HIP stage, UnimodalBranch, MultimodalBlockDown) and the
    decoder stage, one training step under autocast(float16) with GradScaler: finite loss, finite gradients, a step taken."""
    from types import SimpleNamespace
    import numpy as np
    from conftest import load_golden, t
    from test_gpu_data import Conv, make_image_data
    from deepviewagg_amd import dropin
    from deepviewagg_amd.core.multimodal.image import ImageData
    from deepviewagg_amd.modules.multimodal import (UnimodalBranch, BimodalCSRPool, GroupBimodalCSRPool,
                                                    BimodalFusion)
    from deepviewagg_amd.modules.multimodal.modules import MultimodalBlockDown, multimodal_input
    from deepviewagg_amd.modules.SparseConv3d import ResNetDown, ResNetUp
    dropin.install()
    g = load_golden("branch_nearest")
    n_set = int(g["n_settings"])
    torch.manual_seed(0)
    xs = [t(g[f"s{i}_x_img"], DEV).requires_grad_() for i in range(n_set)]
    sds = [make_image_data(g, f"s{i}_", xs[i], g[f"s{i}_ref_size"], DEV) for i in range(n_set)]
    x_3d = t(g["x_3d"])
    n = x_3d.shape[0]
    side = int(np.ceil(n ** (1 / 3))) + 1
    lin = torch.randperm(side ** 3, generator=torch.Generator().manual_seed(7))[:n]
    coords = torch.stack([lin % side, (lin // side) % side, lin // (side * side)], 1).int()

    class _Batch(SimpleNamespace):
        def to(self, device):
            return self
    data = _Batch(x=x_3d, coords=coords, batch=torch.zeros(n, dtype=torch.long), pos=None,
                  modalities={"image": ImageData(sds)})
    nc = int(g["x_3d"].shape[1])
    branch = UnimodalBranch(Conv(6, 8), BimodalCSRPool(mode="max"),
                            GroupBimodalCSRPool(in_map=8, in_mod=8, num_groups=4, use_num=True),
                            BimodalFusion(mode="concatenation"))
    enc = MultimodalBlockDown(ResNetDown(down_conv_nn=[nc, 16], N=1),
                              ResNetDown(down_conv_nn=[24, 32], stride=1, kernel_size=3, N=1), image=branch).to(DEV).train()
    dec = ResNetUp(up_conv_nn=[32, nc, 12], N=1).to(DEV).train()
    params = list(enc.parameters()) + list(dec.parameters())
    opt = torch.optim.SGD(params, lr=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    before = [p.detach().clone() for p in params]
    with torch.autocast("cuda", dtype=torch.float16):
        mm = multimodal_input(data, DEV)
        skip = mm["x_3d"]
        out = enc(mm)
        y = dec(out["x_3d"], skip)
        loss = y.F.float().square().mean()
    assert torch.isfinite(loss)
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    for p in params:
        assert p.grad is None or torch.isfinite(p.grad).all()
    assert all(torch.isfinite(x_.grad).all() for x_ in xs)
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 2.0 ** 16                       # nothing overflowed: the step was taken
    assert any(not torch.equal(b, p.detach()) for b, p in zip(before, params))


def _generic_case(seed, N=700, C=64, G=4):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(0, 7, (N,), generator=gen)
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    V = int(csr[-1])
    R = 300
    rows = torch.randn(R, C, generator=gen)
    row_idx = torch.randint(0, R, (V,), generator=gen).int()
    compat = torch.randn(V, G, generator=gen)
    return rows, row_idx, compat, csr


def test_generic_ops_fp16_match_their_fp32_upcast():
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal.pooling import batchnorm_act_rows
    rows, row_idx, compat, csr = _generic_case(2)
    rh = rows.half().to(DEV)
    rf = rh.float()
    cs = csr.to(DEV)
    vals_h, vals_f = rh[row_idx.long().to(DEV)], rf[row_idx.long().to(DEV)]
    for reduce in ("sum", "mean", "max"):
        a, b = ops.segment_csr(vals_h, cs, reduce=reduce), ops.segment_csr(vals_f, cs, reduce=reduce)
        assert a.dtype == torch.float16
        assert rel(a, b) <= 2e-3, reduce
    # view_gather_attention forward and backward (fp16 rows, fp32 scores)
    res = []
    for r in (rh, rf):
        r = r.clone().requires_grad_()
        c = compat.to(DEV).requires_grad_()
        gw = torch.full((4,), 1.1, device=DEV, requires_grad=True)
        gb = torch.full((4,), 0.2, device=DEV, requires_grad=True)
        out = ops.view_gather_attention(r, row_idx.to(DEV), c, cs, gw, gb, scaling=True)[0]
        g = torch.autograd.grad((out.float() * torch.linspace(-1, 1, out.numel(), device=DEV).view_as(out)).sum(),
                                [r, c, gw, gb])
        res.append((out, g))
    (oh, gh), (of, gf) = res
    assert oh.dtype == torch.float16 and gh[0].dtype == torch.float16
    assert rel(oh, of) <= 2e-3
    for a, b in zip(gh, gf):
        assert rel(a, b) <= 2e-3
    # E_mod's BatchNorm + LeakyReLU on the map rows
    bn = torch.nn.BatchNorm1d(64).to(DEV).train()
    yh = rh.clone().requires_grad_()
    yf = rf.clone().requires_grad_()
    oh = batchnorm_act_rows(yh, bn, 0.2)
    bn2 = torch.nn.BatchNorm1d(64).to(DEV).train()
    of = batchnorm_act_rows(yf, bn2, 0.2)
    assert oh.dtype == torch.float16
    assert rel(oh, of) <= 2e-3
    w = torch.randn(oh.shape, device=DEV)
    (gh,) = torch.autograd.grad((oh.float() * w).sum(), yh)
    (gf,) = torch.autograd.grad((of * w).sum(), yf)
    assert rel(gh, gf) <= 2e-3


def _fp16_pair(case, G, train, gating):
    """(chain fp16 error, chain bf16 error, oracle autocast error) of the forward output."""
    ref, m = build(case, G, train, gating=gating)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    out_ref = ref(None, O.gather_nearest(case["x"], case["images"], case["pixels"]), case["x_map"], case["csr"])
    ref.load_state_dict(sd)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        out_amp = ref(None, O.gather_nearest(case["x"], case["images"], case["pixels"]), case["x_map"], case["csr"])
    return ref, sd, m, out_ref, out_amp


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("sizes_fn,N,C,G", [(ragged, 3000, 64, 4), (ragged_long, 2000, 64, 4), (full32, 300, 64, 4),
                                            (ragged_long, 1500, 32, 2), (ragged, 1500, 128, 1),
                                            (ragged_long, 700, 512, 4), (ragged, 900, 256, 4),
                                            (ragged, 1200, 128, 4)])
def test_chain_forward_fp16_matches_oracle(sizes_fn, N, C, G, train, chain_calls):
    case = make_case(3, N, C, sizes_fn)
    _, _, m, out_ref, out_amp = _fp16_pair(case, G, train, True)
    out, _ = run_dev(case, m, torch.float16, need_grad=False)
    assert chain_calls["fwd"] >= 1
    assert out.dtype == torch.float16
    _, _, m2, _, _ = _fp16_pair(case, G, train, True)
    out_bf, _ = run_dev(case, m2, torch.bfloat16, need_grad=False)
    r, r_bf, r_amp = rel(out, out_ref), rel(out_bf, out_ref), rel(out_amp, out_ref)
    print(f"fp16 chain fwd rel err {r:.4f} (bf16 chain {r_bf:.4f}, reference under autocast {r_amp:.4f})")
    assert r < max(2e-2, 1.5 * r_amp), (r, r_amp)
    check_rows_against_autocast(f"fp16 fwd {sizes_fn.__name__} N={N} C={C} G={G} {'train' if train else 'eval'}",
                                out, out_amp, out_ref, case["csr"])
    assert r <= 1.1 * r_bf + 1e-6, (r, r_bf)


@pytest.mark.parametrize("sizes_fn,N,C,G,train,gating", [
    (ragged, 3000, 64, 4, True, True),
    (ragged_long, 2000, 64, 4, True, True),
    (full32, 4096, 64, 4, True, True),
    (ragged, 3000, 64, 4, False, True),
    (ragged_long, 1500, 32, 2, True, True),
    (ragged, 1500, 128, 1, True, False),
    (ragged, 3000, 128, 4, True, True),
    (ragged_long, 700, 512, 4, True, True),
])
def test_chain_backward_fp16_matches_oracle(sizes_fn, N, C, G, train, gating, plan_kind, chain_calls):
    case = make_case(7, N, C, sizes_fn)
    ref, m = build(case, G, train, gating=gating)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    out_ref, g_ref = _oracle_grads(case, ref, autocast=False)
    ref.load_state_dict(sd)
    out_amp, g_amp = _oracle_grads(case, ref, autocast=True)
    out, g = run_dev(case, m, torch.float16)
    check_plan_kind(plan_kind, C)
    assert chain_calls["fwd"] >= 1 and chain_calls["bwd"] >= 1
    assert out.dtype == torch.float16 and g[0].dtype == torch.float16
    assert rel(out, out_ref) < max(2e-2, 1.5 * rel(out_amp, out_ref))
    names = ["x"] + [n for n, _ in ref.named_parameters()]
    amps = sorted(rel(c, b) for n, b, c in zip(names, g_ref, g_amp) if b is not None and n.startswith("E_map"))
    med = amps[len(amps) // 2] if amps else 0.0
    report, bad = [], []
    for n, a, b, c in zip(names, g, g_ref, g_amp):
        if b is None:
            assert a is None or float(a.abs().max()) == 0, n
            continue
        ours, amp = rel(a, b), rel(c, b)
        report.append((n, round(ours, 4), round(amp, 4)))
        if n.startswith("E_map"):
            amp = max(amp, med)
        loose = n.startswith("G.") or n.startswith("E_score")
        if ours > max((4.0 if loose else 2.0) * amp, 5e-2):
            bad.append(report[-1])
    print("fp16 chain bwd rel err (ours, reference under autocast):", report)
    assert not bad, (bad, report)


def test_grad_scaler_step_and_overflow_skip(chain_calls):
    """One fp16 AMP training step through the chain with GradScaler(init_scale=2^16): after unscale_ the gradients lie
    within the bf16 gates of the fp32 oracle and nothing overflowed.  Then the same step with +inf in the upstream
    gradient of one point (the exact-mapping chain path only): the map gradient of that point's views is non-finite,
    the optimizer step is skipped and the scale halves."""
    case = make_case(11, 2000, 64, ragged)
    case["w"] = case["w"] * 1e-3        # a mean-reduced loss: the scaled map gradient stays inside the fp16 range
    ref, m = build(case, 4, True)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    dev_sd = {k: v.clone() for k, v in m.state_dict().items()}
    _, g_ref = _oracle_grads(case, ref, autocast=False)
    ref.load_state_dict(sd)
    _, g_amp = _oracle_grads(case, ref, autocast=True)
    names = ["x"] + [n for n, _ in ref.named_parameters()]

    def step(w):
        from deepviewagg_amd import ops
        from deepviewagg_amd.modules.multimodal import pooling as P
        V = case["V"]
        xd = case["x"].to(DEV).half().contiguous(memory_format=torch.channels_last).requires_grad_()
        opt = torch.optim.SGD(list(m.parameters()), lr=0.1)
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
        packed = ops.pack_gather_index(case["images"].to(DEV), torch.arange(V + 1, device=DEV), case["pixels"].to(DEV))
        with torch.autocast("cuda", dtype=torch.float16):
            lazy = ops.lazy_gather_nearest(xd, packed, exact=True)
            lazy = P.BimodalCSRPool(mode='max')(None, lazy, None, torch.arange(V + 1, device=DEV))
            out = m(None, lazy, case["x_map"].to(DEV), case["csr"].to(DEV))
        opt.zero_grad()
        scaler.scale(out.float()).backward(w.to(DEV))          # upstream gradient = w (what the loss hands back)
        scaler.unscale_(opt)
        finite = all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        before = [p.detach().clone() for p in m.parameters()]
        scaler.step(opt)
        scaler.update()
        after = [p.detach().clone() for p in m.parameters()]
        return xd.grad.float() / (2.0 ** 16), [p.grad for p in m.parameters()], finite, before, after, scaler.get_scale()

    gx, gp, finite, _, _, scale = step(case["w"])
    assert chain_calls["bwd"] >= 1
    assert finite and scale == 2.0 ** 16
    bad = []
    for n, a, b, c in zip(names, [gx] + gp, g_ref, g_amp):
        if b is None:
            continue
        ours, amp = rel(a, b), rel(c, b)
        loose = n.startswith("G.") or n.startswith("E_score") or n.startswith("E_map")
        if ours > max((4.0 if loose else 2.0) * amp, 5e-2):
            bad.append((n, ours, amp))
    assert not bad, bad
    # overflow: +inf in the upstream gradient of one point with views
    m.load_state_dict(dev_sd)
    csr = case["csr"]
    p = int(torch.nonzero(csr[1:] - csr[:-1] > 0)[0])
    w = case["w"].clone()
    w[p, 0] = float("inf")
    gx, _, finite, before, after, scale = step(w)
    assert not finite
    assert scale == 2.0 ** 15
    for b_, a_ in zip(before, after):
        assert torch.equal(b_, a_)
    views = range(int(csr[p]), int(csr[p + 1]))
    rows = gx.permute(0, 2, 3, 1)[case["images"][list(views)], case["pixels"][list(views), 1].long(),
                                  case["pixels"][list(views), 0].long()]
    assert not torch.isfinite(rows).all(dim=1).any()


def test_fp16_refused_by_entries_outside_the_list():
    """Every dtype-taking entry outside the fp16 list returns DVA_ERR_UNSUPPORTED for DVA_F16 (small valid buffers)."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    F16 = _lib.DVA_F16
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    P = ctypes.c_void_p(buf.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dva_plan_split_rows_grad(P, P, 2048, 600, P, 1 << 16, P, 64, 4, F16, _lib.DVA_BF16, st) == -2
    assert lib.dva_plan_split_rows_grad(P, P, 2048, 600, P, 1 << 16, P, 64, 4, _lib.DVA_BF16, F16, st) == -2
    assert lib.dva_anchor_rows_sum(P, P, P, P, P, 4, 8, 64, F16, st) == -2
    assert lib.dva_anchor_fixup(P, P, P, P, P, 4, 1, 2, 2, 64, F16, st) == -2
    assert lib.dva_deepset_fwd_first(P, P, P, P, P, P, 8, 8, 1, F16, st) == -2
    assert lib.dva_deepset_segmax(P, P, P, P, P, 4, 8, F16, st) == -2
    assert lib.dva_deepset_fwd_layer(P, P, P, P, P, P, P, 8, F16, st) == -2
    assert lib.dva_deepset_fwd_score(P, P, P, P, P, 8, 4, F16, st) == -2
    assert lib.dva_deepset_bwd_score(P, P, P, P, P, P, P, P, 8, 4, F16, st) == -2
    assert lib.dva_deepset_bwd_layer(*([P] * 14), 8, 0, 0, F16, st) == -2
    assert lib.dva_deepset_bwd_max(*([P] * 8), 8, F16, st) == -2
    assert lib.dva_deepset_bwd_first(*([P] * 6), 8, 0, F16, st) == -2
    assert lib.dva_concat_cast_fwd(P, P, P, 4, 4, 4, F16, st) == -2
    assert lib.dva_concat_cast_bwd(P, P, P, 4, 4, 4, F16, st) == -2
    assert lib.dva_sparse_conv_workspace_bytes(27, 16, 16, F16) == -2
    assert lib.dva_sparse_conv_apply(P, P, P, P, P, 4, 4, 27, 16, 16, 0, F16, P, 1 << 16, st) == -2
    assert lib.dva_sparse_conv_wgrad(P, P, P, P, 4, 4, 27, 16, 16, F16, st) == -2
    torch.cuda.synchronize()
    assert float(buf.float().abs().max()) == 0.0       # nothing was launched into the buffers
