"""BASELINE-size checks (N = 2^20 points x 32 views, V = 33.5 M) through size-independent properties: the
oracle cannot run at this size in seconds, the properties can."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, VIEWS, C, G, B, H, W = 1 << 20, 32, 64, 4, 32, 64, 128


@pytest.fixture(scope="module")
def scene():
    g = torch.Generator(device=DEV).manual_seed(7)
    V, R = N * VIEWS, B * H * W
    csr = torch.arange(0, V + 1, VIEWS, device=DEV)
    row_idx = torch.randint(0, R, (V,), generator=g, device=DEV, dtype=torch.int32)
    rows = torch.randn(R, C, generator=g, device=DEV).bfloat16()
    compat = torch.randn(V, G, generator=g, device=DEV)
    gw = torch.rand(G, generator=g, device=DEV) + 0.5
    gb = torch.randn(G, generator=g, device=DEV) * 0.1
    return dict(csr=csr, row_idx=row_idx, rows=rows, compat=compat, gw=gw, gb=gb, V=V, R=R)


def test_attention_is_a_convex_combination_and_linear_in_the_values(scene):
    from deepviewagg_amd import ops
    s = scene
    out1, att, gate = ops.view_gather_attention(s["rows"], s["row_idx"], s["compat"], s["csr"], s["gw"], s["gb"])
    # softmax: attentions of a point sum to one per group (eps 1e-12 in the denominator)
    sums = att.view(N, VIEWS, G).sum(1)
    assert float((sums - 1).abs().max()) < 1e-5
    assert float(att.min()) >= 0
    # gate in [0, 1), tanh(relu(.))
    assert float(gate.min()) >= 0 and float(gate.max()) < 1
    # linearity in the value map (bf16 output rounding: 2^-8 relative)
    rows2 = torch.randn_like(s["rows"])
    out2, _, _ = ops.view_gather_attention(rows2, s["row_idx"], s["compat"], s["csr"], s["gw"], s["gb"])
    mix = (0.5 * s["rows"].float() - 2.0 * rows2.float()).bfloat16()
    out3, _, _ = ops.view_gather_attention(mix, s["row_idx"], s["compat"], s["csr"], s["gw"], s["gb"])
    ref = 0.5 * out1.float() - 2.0 * out2.float()
    err = (out3.float() - ref).abs().max() / ref.abs().max()
    assert float(err) < 3e-2
    # a constant value map is reproduced (convex combination), scaled by the gate
    ones = torch.ones_like(s["rows"])
    outc, _, gate = ops.view_gather_attention(ones, s["row_idx"], s["compat"], s["csr"], s["gw"], s["gb"])
    exp = gate.repeat_interleave(C // G, dim=1)
    assert float((outc.float() - exp).abs().max()) < 1e-2


def test_rows_gradient_is_deterministic_and_conserves_mass(scene):
    from deepviewagg_amd import ops
    s = scene
    g = torch.Generator(device=DEV).manual_seed(1)
    w = torch.randn(N, C, generator=g, device=DEV).bfloat16()
    plan = ops.row_plan(s["row_idx"], s["R"], with_counts=True)
    (perm, row_ptr), counts = plan
    assert int(counts.sum()) == s["V"] and int(row_ptr[-1]) == s["V"]
    assert bool((s["row_idx"][perm.long()][1:] >= s["row_idx"][perm.long()][:-1]).all())     # sorted by row

    def grads():
        rows = s["rows"].clone().requires_grad_()
        compat = s["compat"].clone().requires_grad_()
        out, att, gate = ops.view_gather_attention(rows, s["row_idx"], compat, s["csr"], s["gw"], s["gb"],
                                                   plan=(perm, row_ptr))
        out.backward(w)
        return rows.grad, compat.grad, gate

    g1, c1, gate = grads()
    g2, c2, _ = grads()
    assert torch.equal(g1, g2) and torch.equal(c1, c2)                     # no atomics: bit-reproducible
    # sum over map rows of the rows gradient = sum over points of gate * grad_out (attentions sum to one)
    lhs = g1.float().sum(0)
    rhs = (w.float() * gate.repeat_interleave(C // G, dim=1)).sum(0)
    assert float((lhs - rhs).abs().max() / rhs.abs().max()) < 2e-2        # bf16 rounding of 262 k rows
    # softmax backward: the score gradients of a point sum to ~0 per group, except for the gate path through
    # the per-group max (one view per point and group)
    s_c = c1.view(N, VIEWS, G).sum(1)
    assert torch.isfinite(s_c).all()


def test_split_plan_rows_gradient_full_size_equals_index_add(scene):
    """The headline's rows-gradient path -- split plan (`dva_plan_split_build`), pass A on the 16-byte view records,
    `bucket_rows_grad_kernel<64>` (`dva_plan_split_rows_grad`) -- at V = 33.5 M views / R = 2^18 rows against an
    INDEPENDENT sum: the reference's backward of the row gather is an ``index_add`` of the views'
    gradients (core/multimodal/image.py:1262-1287), so an 8-channel slice (two channels of every group) is summed by
    ``torch.index_add_`` in fp32 on the device.  Tolerance 2^-7 of the largest entry: one bf16 rounding of a sum of
    ~128 products (2^-9 relative) plus the fp32 atomics' order."""
    from deepviewagg_amd import ops
    s = scene
    V, R = s["V"], s["R"]
    g = torch.Generator(device=DEV).manual_seed(21)
    point = torch.arange(V, device=DEV, dtype=torch.int32) // VIEWS
    wts = torch.randn(V, 4, generator=g, device=DEV).bfloat16()
    rec = torch.empty(V, 4, dtype=torch.int32, device=DEV)
    rec[:, 0] = point
    rec[:, 1:3] = wts.view(torch.int32)
    rec[:, 3] = s["row_idx"]
    gout = torch.randn(N, C, generator=g, device=DEV).bfloat16()
    assert ops._split_plan_pays(V, R)                       # the threshold selects the split plan by itself here
    plan = ops.row_plan(s["row_idx"], R, with_counts=False)[0]
    assert isinstance(plan, ops.SplitPlan)
    got = plan.rows_grad_fused(gout, rec, C, G, torch.cuda.current_stream().cuda_stream)
    assert got is not None and got.dtype == torch.bfloat16 and got.shape == (R, C)
    chs = torch.tensor([0, 9, 17, 26, 35, 44, 52, 63], device=DEV)
    grp = chs // (C // G)
    ref = torch.zeros(R, chs.numel(), dtype=torch.float32, device=DEV)
    step = V // 8
    for lo in range(0, V, step):                            # 8 chunks of 4.2 M views: 134 MB of products each
        sl = slice(lo, lo + step)
        prod = gout[point[sl].long()][:, chs].float() * wts[sl][:, grp].float()
        ref.index_add_(0, s["row_idx"][sl].long(), prod)
    scale = float(ref.abs().max())
    err = float((got[:, chs].float() - ref).abs().max())
    assert err <= scale * 2 ** -7, (err, scale)
    assert float(ref.abs().max()) > 1.0                      # the sums are not trivially small


def test_deepset_scores_are_equivariant_to_view_permutations():
    """DeepSetFeat pools with a max over the views of a point: permuting the views inside every point permutes
    the scores the same way (fused kernels, bf16 storage, full size)."""
    from deepviewagg_amd.modules.multimodal import pooling as P
    from deepviewagg_amd import fused_deepset
    g = torch.Generator(device=DEV).manual_seed(3)
    V = N * VIEWS
    m = P.GroupBimodalCSRPool(in_map=8, in_mod=C, num_groups=G, use_num=True).to(DEV).eval()
    csr = torch.arange(0, V + 1, VIEWS, device=DEV)
    x_map = torch.rand(V, 8, generator=g, device=DEV)
    perm_in = torch.argsort(torch.rand(N, VIEWS, generator=g, device=DEV), dim=1)
    flat = (perm_in + torch.arange(N, device=DEV).view(-1, 1) * VIEWS).view(-1)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert fused_deepset.applicable(m.E_map, m.E_score, x_map)
        s1 = fused_deepset.deepset_linear(m.E_map, m.E_score, x_map, csr)
        s2 = fused_deepset.deepset_linear(m.E_map, m.E_score, x_map[flat].contiguous(), csr)
    assert torch.equal(s1[flat], s2)      # same arithmetic per view, max is order independent: bit-identical


# ---------------------------------------------------------------------------------------------------------------
# The kernels bench.py times, at the size it times them (VERDICT r2 missing 5): the bf16 recompute chain
# (fused_chain.chain_pool -> dva_chain_*) forward + backward at N = 2^20 points x 32 views, V = 33.5 M (the 32-bit
# buffer offsets of the view-sized arrays reach 2.1 GB here).
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_scene():
    from deepviewagg_amd.modules.multimodal import pooling as P
    g = torch.Generator(device=DEV).manual_seed(11)
    V, R = N * VIEWS, B * H * W
    csr = torch.arange(0, V + 1, VIEWS, device=DEV)
    row_idx = torch.randint(0, R, (V,), generator=g, device=DEV, dtype=torch.int32)
    # a tenth of the map rows is never read: their gradient must come out exactly zero
    unread = torch.rand(R, generator=g, device=DEV) < 0.1
    repl = torch.nonzero(~unread).view(-1)
    row_idx = torch.where(unread[row_idx.long()], repl[row_idx.long() % repl.numel()].int(), row_idx).contiguous()
    rows = torch.randn(R, C, generator=g, device=DEV).bfloat16()
    x_map = torch.rand(V, 8, generator=g, device=DEV)
    w = (torch.randn(N, C, generator=g, device=DEV) / N).bfloat16()
    torch.manual_seed(3)
    m = P.GroupBimodalCSRPool(in_map=8, in_mod=C, num_groups=G, use_num=True).to(DEV).train()
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if "batch_norm.weight" in n_ or n_ == "G.weight":
                p.add_(0.2 * torch.randn_like(p))
            elif "batch_norm.bias" in n_ or n_ == "G.bias":
                p.add_(0.2 * torch.randn_like(p))
    return dict(csr=csr, row_idx=row_idx, rows=rows, x_map=x_map, w=w, m=m, V=V, R=R, unread=unread)


def _chain_step(s, sl=None, chain=True, saved=None):
    """forward + backward of GroupBimodalCSRPool's attention part on value rows that are already E_mod(rows).
    ``sl``: the first ``sl`` points of the scene, or (first point, number of points).  ``saved``: a dict that receives
    the BatchNorm invstd of the folded layers and the scores the forward kernel left for the backward."""
    from deepviewagg_amd import ops, fused_chain, fused_deepset
    rows = s["rows"].clone().requires_grad_()
    if sl is None:
        csr, row_idx, x_map, w = s["csr"], s["row_idx"], s["x_map"], s["w"]
    else:                                      # a run of points of the same scene
        p0, n = (0, sl) if isinstance(sl, int) else sl
        csr = (s["csr"][p0:p0 + n + 1] - s["csr"][p0]).contiguous()
        row_idx = s["row_idx"][p0 * VIEWS:(p0 + n) * VIEWS].contiguous()
        x_map, w = s["x_map"][p0 * VIEWS:(p0 + n) * VIEWS].contiguous(), s["w"][p0:p0 + n].contiguous()
    gf = ops.GatheredFeatures(rows, row_idx, None, True, None)
    m = s["m"]
    params = [p for n_, p in m.named_parameters() if not n_.startswith("E_mod")]
    if chain:
        fused_chain.FORCE = True
        try:
            out = fused_chain.chain_pool(m, gf, x_map, csr)
        finally:
            fused_chain.FORCE = None
        if saved is not None:       # as tests/test_gpu_chain.py::test_chain_matches_bf16_emulation reads them
            sv = out.grad_fn.saved_tensors
            saved["invstd"] = {1: sv[12][1].cpu(), 2: sv[13][1].cpu(), 6: sv[15][1].cpu()}
            saved["scores"] = sv[17].cpu()[:, :G].clone()
    else:
        # the first-generation path: stored-activation DeepSet kernels + the team attention kernels
        compat = fused_deepset.deepset_linear(m.E_map, m.E_score, x_map, csr)
        out, _, _ = ops.view_gather_attention(rows, row_idx, compat, csr, m.G.weight, m.G.bias,
                                              scaling=m.group_scaling)
    grads = torch.autograd.grad(out, [rows] + params, grad_outputs=w, allow_unused=True)
    return out, grads


def test_chain_full_size_properties(chain_scene):
    """Determinism, mass conservation of the rows gradient, zero gradient on unread rows, finite parameter gradients
    of the recompute chain at the headline size (train mode: batch statistics over all 33.5 M views)."""
    s = chain_scene
    state = {k: v.clone() for k, v in s["m"].state_dict().items()}
    out1, g1 = _chain_step(s)
    s["m"].load_state_dict(state)              # the running statistics moved: same start for the second run
    out2, g2 = _chain_step(s)
    s["m"].load_state_dict(state)
    assert out1.dtype == torch.bfloat16 and out1.shape == (N, C)
    assert torch.isfinite(out1.float()).all()
    # the rows gradient is a segmented reduction in plan order (no atomics) and the forward has no atomics on its
    # outputs: bit-reproducible.  Parameter gradients are sums through fp32 / fp64 atomics: reproducible to rounding
    assert torch.equal(out1, out2)
    assert torch.equal(g1[0], g2[0])
    for a, b in zip(g1[1:], g2[1:]):
        assert a is not None and torch.isfinite(a).all()
        assert float((a - b).norm() / (a.norm() + 1e-30)) < 1e-3
    # rows never read by a view receive exactly zero
    assert float(g1[0][s["unread"]].float().abs().max()) == 0.0
    # mass conservation: sum over the map rows of the rows gradient = sum over the points of gate * grad_out
    # (the attentions of a point sum to one per group); the gate is recovered from a constant value map
    from deepviewagg_amd import ops, fused_chain
    ones = torch.ones_like(s["rows"])
    fused_chain.FORCE = True
    try:
        with torch.no_grad():
            gate_c = fused_chain.chain_pool(s["m"], ops.GatheredFeatures(ones, s["row_idx"], None, True, None),
                                            s["x_map"], s["csr"]).float()
    finally:
        fused_chain.FORCE = None
    s["m"].load_state_dict(state)
    lhs = g1[0].float().sum(0)
    rhs = (s["w"].float() * gate_c).sum(0)
    assert float((lhs - rhs).abs().max() / rhs.abs().max()) < 3e-2       # bf16 roundings of gate, rows gradient
    assert float(gate_c.min()) >= 0 and float(gate_c.max()) <= 1.0


def test_chain_full_size_agrees_with_stored_activation_path_on_a_slice(chain_scene):
    """The same kernels on the first 2^16 points of the same scene, in EVAL mode (running statistics: the slice and
    the whole scene then compute the same function per point), against (a) the full-size result restricted to the
    slice -- bit-identical: a point's output depends on its own views only -- and (b) the first-generation
    stored-activation path (fp32-MFMA DeepSet kernels + team attention kernels) on the slice."""
    s = chain_scene
    m = s["m"]
    m.eval()
    try:
        sl = 1 << 16
        out_full, g_full = _chain_step(s)
        out_sl, g_sl = _chain_step(s, sl=sl)
        assert torch.equal(out_full[:sl], out_sl)
        out_b, g_b = _chain_step(s, sl=sl, chain=False)
        rel = lambda a, b: float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))
        assert rel(out_sl, out_b) < 2e-2, rel(out_sl, out_b)
        assert rel(g_sl[0], g_b[0]) < 5e-2, rel(g_sl[0], g_b[0])
        _far_slices_row_wise(s, out_full)
    finally:
        m.train()


def _far_slices_row_wise(s, out_full):
    """Eval mode (the caller set it): 2^12 points at the END of the cloud and 2^12 in the middle that start inside a
    512-view construction chunk, behind view 2^24.  The full-size rows of the slice against (a) a run on the slice alone
    and (b) the float64 emulation of those points on the CPU (131 k views), both row-wise with the gate of
    tests/rowwise.py: FP32_HEADROOM x the float32 emulation's own error against the float64 one on the slice."""
    import rowwise as RW
    from deepviewagg_amd import fused_chain
    from oracle import pooling_oracle as O
    from tolerances import Report
    n = 1 << 12
    ref = O.GroupBimodalCSRPool(in_map=8, in_mod=C, num_groups=G, use_num=True)
    ref.load_state_dict({k: v.cpu() for k, v in s["m"].state_dict().items()})
    ref.eval()
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    rows = s["rows"].cpu()
    for name, p0 in (("end", N - n), ("middle", N // 2 + 5)):
        assert (p0 * VIEWS) % fused_chain.VIEWS_PER_CHUNK != 0 or name == "end"
        saved = {}
        out_sl, _ = _chain_step(s, sl=(p0, n), saved=saved)
        csr = torch.arange(0, n * VIEWS + 1, VIEWS)
        row_idx = s["row_idx"][p0 * VIEWS:(p0 + n) * VIEWS].cpu()
        x_map, w = s["x_map"][p0 * VIEWS:(p0 + n) * VIEWS].cpu(), s["w"][p0:p0 + n].float().cpu()
        ev = RW.emulate_all(ref, sd, rows, row_idx, x_map, csr, w, saved["invstd"], saved["scores"])
        tiles, n_tiles = fused_chain.build_tiles(csr.to(DEV), n * VIEWS)
        masks = RW.strata(csr, tiles[:int(n_tiles)].cpu(), fused_chain.VIEWS_PER_CHUNK)
        live = torch.ones(n, dtype=torch.bool)
        got = out_full[p0:p0 + n]
        label = f"full size, {name} slice [{p0}, {p0 + n})"
        rep = Report("headline scene against the float64 emulation, row-wise: " + label)
        # (a) the slice run: the plain yardstick (both are the device; the slice is tiled on its own)
        p32, p64 = ev[(False, torch.float32)], ev[(False, torch.float64)]
        noise = RW.row_err(RW.as_device_rounds(p32["out"], got), p64["out"], live)
        worst = {"full vs slice": RW.gate_rows(rep, label, "out: full vs slice run", RW.row_err(got, out_sl, live), noise,
                                               masks, live)}
        # (b) the float64 emulation of the slice
        worst.update(RW.gate_chain(rep, label, ev, csr, masks, got, saved["scores"]))
        print(label, "worst ratio to the float32 emulation's own noise:", {k: round(v, 2) for k, v in worst.items()})
        RW.write_report(rep)
        rep.check()


# ---------------------------------------------------------------------------------------------------------------
# The fp32 chain (fused_chain_f32.chain_scores -> dva_chain3_*) at the size `bench.py --dtype f32` times it:
# N = 2^20 points x 32 views, V = 33.5 M -- the fp32 row tensors z2 / z5 / dy5 / dy2 are exactly 4 GiB there (one buffer
# descriptor per tile).
# ---------------------------------------------------------------------------------------------------------------
def test_chain3_full_size_properties():
    import copy
    from deepviewagg_amd.modules.multimodal import pooling as P
    from deepviewagg_amd import fused_chain_f32, fused_deepset
    g = torch.Generator(device=DEV).manual_seed(17)
    V = N * VIEWS
    csr = torch.arange(0, V + 1, VIEWS, device=DEV)
    x_map = torch.rand(V, 8, generator=g, device=DEV)
    torch.manual_seed(5)
    m = P.GroupBimodalCSRPool(in_map=8, in_mod=C, num_groups=G, use_num=True).to(DEV).train()
    assert fused_chain_f32.applicable(m.E_map, m.E_score, x_map, csr)

    def run(mod):
        s = fused_chain_f32.chain_scores(mod.E_map, mod.E_score, x_map, csr)
        # a loss whose score gradients differ per view and per group
        wgt = torch.linspace(-1.0, 1.0, 4 * 97, device=DEV).view(97, 4)[torch.arange(V, device=DEV) % 97]
        grads = torch.autograd.grad((s * wgt).sum() / V, list(mod.E_map.parameters()) + list(mod.E_score.parameters()))
        return s.detach(), grads
    m2 = copy.deepcopy(m)
    s1, g1 = run(m)
    s2, g2 = run(m2)
    assert s1.shape == (V, G) and bool(torch.isfinite(s1).all())
    assert torch.equal(s1, s2)                                   # deterministic statistics: bit-identical forward
    for a, b in zip(g1, g2):
        assert bool(torch.isfinite(a).all())
        # weight gradients go through fp32 atomics of per-wavefront partial sums: equal to rounding
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-7 + 1e-5 * float(a.abs().max()))
    # DeepSetFeat pools with a max: permuting the views inside every point permutes the scores the same way
    m.eval()
    perm_in = torch.argsort(torch.rand(N, VIEWS, generator=g, device=DEV), dim=1)
    flat = (perm_in + torch.arange(N, device=DEV).view(-1, 1) * VIEWS).view(-1)
    with torch.no_grad():
        e1 = fused_chain_f32.chain_scores(m.E_map, m.E_score, x_map, csr)
        e2 = fused_chain_f32.chain_scores(m.E_map, m.E_score, x_map[flat].contiguous(), csr)
        assert torch.equal(e1[flat], e2)
        # against the stored-activation fp32 kernels on a 2^16-point slice of the same scene (eval mode: running statistics)
        n_s = 1 << 16
        sl = slice(0, n_s * VIEWS)
        ref = fused_deepset.deepset_linear(m.E_map, m.E_score, x_map[sl].contiguous(), csr[:n_s + 1].contiguous())
    torch.testing.assert_close(e1[sl], ref, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------
# The fused bilinear path (fused_bilinear._EmodPool -> dva_emod_*, interpolate=True) at the size bench.py times it
# (VERDICT r3 "next 1a"): N = 2^20 points x 32 views = 33.5 M views for 64 -> 64 (z_a / dy_a are exactly 4 GiB there:
# one buffer descriptor per tile) and for the KITTI-360 pair 128 -> 32, and one scene just below the 32-bit limits
# `fused_bilinear.applicable` guards.
# ---------------------------------------------------------------------------------------------------------------
UP = 8


def _bilinear_scene(n_points, C_in, C_out, seed, unseen_frac=0.05):
    from deepviewagg_amd.modules.multimodal import pooling as P
    g = torch.Generator(device=DEV).manual_seed(seed)
    k = torch.full((n_points,), VIEWS, device=DEV, dtype=torch.int64)
    k[torch.rand(n_points, generator=g, device=DEV) < unseen_frac] = 0           # unseen points: output exactly 0
    csr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), k.cumsum(0)])
    V = int(csr[-1])
    images = torch.randint(0, B, (V,), generator=g, device=DEV)
    pixels = torch.stack([torch.randint(0, W * UP, (V,), generator=g, device=DEV),
                          torch.randint(0, H * UP, (V,), generator=g, device=DEV)], 1).to(torch.int16)
    x = torch.randn(B, C_in, H, W, generator=g, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    x_map = torch.rand(V, 8, generator=g, device=DEV)
    w = (torch.randn(n_points, C_out, generator=g, device=DEV) / n_points).bfloat16()
    torch.manual_seed(seed)
    m = P.GroupBimodalCSRPool(in_map=8, in_mod=C_in, out_mod=C_out, num_groups=G, use_num=True).to(DEV).train()
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if "batch_norm" in n_ or n_.startswith("G."):
                p.add_(0.2 * torch.randn_like(p))
    return dict(csr=csr, V=V, N=n_points, images=images, pixels=pixels, x=x, x_map=x_map, w=w, m=m, unseen=(k == 0),
                C_in=C_in, C_out=C_out)


def _bilinear_step(s, sl=None, fused=True, need_grad=True):
    """forward + backward of interpolate=True through the data-flow objects; `sl`: the first `sl` points only."""
    from deepviewagg_amd import ops, fused_chain
    from deepviewagg_amd.modules.multimodal import pooling as P
    if sl is None:
        csr, V, w = s["csr"], s["V"], s["w"]
    else:
        csr = s["csr"][:sl + 1].contiguous()
        V, w = int(csr[-1]), s["w"][:sl].contiguous()
    images, pixels, x_map = s["images"][:V], s["pixels"][:V].contiguous(), s["x_map"][:V].contiguous()
    x = s["x"].clone().requires_grad_(need_grad)
    atom_ptr = torch.arange(V + 1, device=DEV)
    packed = ops.pack_gather_index(images, atom_ptr, pixels)
    res = torch.tensor([[W * UP, H * UP]], dtype=torch.float32, device=DEV)
    coords = (pixels / (res - 1))[:, [1, 0]]
    fused_chain.FORCE = None if fused else False
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lazy = ops.lazy_gather_bilinear(x, packed, coords, exact=True)
            lazy = P.BimodalCSRPool(mode='max')(None, lazy, None, atom_ptr)
            out = s["m"](None, lazy, x_map, csr)
        fn = type(out.grad_fn).__name__ if out.grad_fn is not None else None
        if fused and need_grad:
            assert fn == "_EmodPoolBackward", f"the fused bilinear path must be the one that ran ({fn})"
        grads = None
        if need_grad:
            grads = torch.autograd.grad(out, [x] + list(s["m"].parameters()), grad_outputs=w.to(out.dtype),
                                        allow_unused=True)
    finally:
        fused_chain.FORCE = None
    return out, grads


@pytest.mark.parametrize("C_in,C_out", [(64, 64), (128, 32), (256, 128), (512, 256)])
def test_fused_bilinear_full_size_properties(C_in, C_out):
    """Determinism, exact zeros on unseen points, finite parameter gradients, and the conservation law of the train-mode
    feature-map gradient: BatchNorm_a's backward removes the batch mean of dz_a, the interpolation weights of a view sum
    to one, so the gradient of Y = x W_a^T sums to ~0 over the map rows per channel -- and with it the gradient of x
    (a statement about the anchor plan + Gram-matrix BatchNorm backward at V = 31.9 M)."""
    s = _bilinear_scene(N, C_in, C_out, seed=29)
    if C_out >= 64:
        assert s["V"] * C_out * 2 > (1 << 31), "the view-sized rows of this case need more than 31 offset bits"
    state = {k: v.clone() for k, v in s["m"].state_dict().items()}
    out1, g1 = _bilinear_step(s)
    s["m"].load_state_dict(state)
    out2, g2 = _bilinear_step(s)
    s["m"].load_state_dict(state)
    assert out1.dtype == torch.bfloat16 and out1.shape == (N, C_out)
    assert bool(torch.isfinite(out1.float()).all())
    assert torch.equal(out1, out2)                         # no atomics on the outputs, deterministic statistics
    assert torch.equal(g1[0], g2[0])                       # anchor plan: segmented reduction in a fixed order
    assert float(out1.detach()[s["unseen"]].float().abs().max()) == 0.0
    seen_norm = out1[~s["unseen"]].float().abs().mean()
    assert float(seen_norm) > 1e-3                         # the seen points carry a signal
    for (n_, _), a, b in zip(s["m"].named_parameters(), g1[1:], g2[1:]):
        assert a is not None and bool(torch.isfinite(a).all()), n_
        assert float((a - b).norm() / (a.norm() + 1e-30)) < 1e-3, n_
    gx = g1[0].float()
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().sum()) > 0
    per_channel = gx.sum(dim=(0, 2, 3)).abs() / (gx.abs().sum(dim=(0, 2, 3)) + 1e-30)
    assert float(per_channel.max()) < 2e-3, float(per_channel.max())


@pytest.mark.parametrize("C_in,C_out", [(64, 64), (128, 32), (256, 128)])
def test_fused_bilinear_full_size_slice(C_in, C_out):
    """Eval mode (running statistics: a point's output depends on its own views only): the first 2^16 points of the
    full-size run are bit-identical to a run on that slice alone, and the slice agrees with the materialised dataflow
    (gather_bilinear -> [V, C] -> E_mod rows -> first-generation attention kernels) within 2e-2 / 5e-2."""
    s = _bilinear_scene(N, C_in, C_out, seed=31)
    s["m"].eval()
    sl = 1 << 16
    out_full, g_full = _bilinear_step(s)
    out_sl, g_sl = _bilinear_step(s, sl=sl)
    assert torch.equal(out_full[:sl], out_sl)
    out_b, g_b = _bilinear_step(s, sl=sl, fused=False)
    rel = lambda a, b: float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))
    assert rel(out_sl, out_b) < 2e-2, rel(out_sl, out_b)
    assert rel(g_sl[0], g_b[0]) < 5e-2, rel(g_sl[0], g_b[0])
    assert float(out_full[s["unseen"]].float().abs().max()) == 0.0


def test_fused_bilinear_just_below_the_applicable_limits():
    """`fused_bilinear.applicable` admits V x 64 < 2^32 - 16 (the chain's 64-byte handed rows / 32-byte x_map rows use
    32-bit buffer offsets): a 128 -> 32 scene with V = 2^26 - 32 views runs on the fused path, is deterministic and
    keeps the slice property; one more point and the module takes the materialised path instead of overflowing."""
    from deepviewagg_amd import fused_bilinear, ops
    n = (1 << 21) - 1
    s = _bilinear_scene(n, 128, 32, seed=37, unseen_frac=0.0)
    assert s["V"] == n * VIEWS and s["V"] * 64 < (1 << 32) - 16 and (s["V"] + VIEWS) * 64 >= (1 << 32) - 16
    s["m"].eval()
    out, g = _bilinear_step(s)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(g[0].float()).all())
    sl = 1 << 14
    out_sl, _ = _bilinear_step(s, sl=sl)
    assert torch.equal(out[:sl], out_sl)
    # the last tile of the scene (the highest 32-bit offsets) against a run on the last points alone
    tail = 1 << 12
    t = dict(s)
    V0 = int(s["csr"][n - tail])
    t.update(csr=(s["csr"][n - tail:] - V0).contiguous(), V=s["V"] - V0, N=tail, images=s["images"][V0:],
             pixels=s["pixels"][V0:], x_map=s["x_map"][V0:], w=s["w"][n - tail:])
    out_t, _ = _bilinear_step(t)
    assert torch.equal(out[n - tail:], out_t)
    # the guard itself: this scene is admitted, one more point is not (CPU test of the arithmetic: test_size_limits.py)
    assert fused_bilinear.size_limits_ok(s["V"], B * H * W, n, 32)
    assert not fused_bilinear.size_limits_ok(s["V"] + VIEWS, B * H * W, n + 1, 32)


# ---------------------------------------------------------------------------------------------------------------
# QKVBimodalCSRPool with its keys on the recompute chain (round 4) at the size bench.py times it.
# ---------------------------------------------------------------------------------------------------------------
def test_qkv_chain_full_size_properties():
    """N = 2^20 points x 32 views: two runs bit-identical (output and feature-map gradient), unseen points exactly 0,
    finite parameter gradients; eval mode: the first 2^16 points equal a run on that slice alone bit for bit."""
    from deepviewagg_amd import ops, fused_chain
    from deepviewagg_amd.modules.multimodal import pooling as P
    g = torch.Generator(device=DEV).manual_seed(41)
    k = torch.full((N,), VIEWS, device=DEV, dtype=torch.int64)
    k[torch.rand(N, generator=g, device=DEV) < 0.05] = 0
    csr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), k.cumsum(0)])
    V, R = int(csr[-1]), B * H * W
    row_idx = torch.randint(0, R, (V,), generator=g, device=DEV, dtype=torch.int32)
    rows = torch.randn(R, C, generator=g, device=DEV).bfloat16()
    x_map = torch.rand(V, 8, generator=g, device=DEV)
    x_main = torch.randn(N, 4, generator=g, device=DEV)
    w = (torch.randn(N, C, generator=g, device=DEV) / N).bfloat16()
    torch.manual_seed(9)
    m = P.QKVBimodalCSRPool(in_main=4, in_map=8, in_mod=C, num_groups=G, nc_qk=8, use_num=True).to(DEV).train()
    state = {kk: v.clone() for kk, v in m.state_dict().items()}

    def step(n=None):
        nn_ = N if n is None else n
        c = csr[:nn_ + 1].contiguous()
        v = int(c[-1])
        r = rows.clone().requires_grad_()
        gf = ops.GatheredFeatures(r, row_idx[:v].contiguous(), None, True, None)
        calls = []
        orig = fused_chain.qkv_pool

        def spy(*a, **kw):
            calls.append(1)
            return orig(*a, **kw)
        fused_chain.qkv_pool = spy
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = m(x_main[:nn_].contiguous(), gf, x_map[:v].contiguous(), c)
        finally:
            fused_chain.qkv_pool = orig
        assert calls == [1], "the whole pooling must have run in the chain's view kernel (dva_chain_attn_fwd_keys)"
        grads = torch.autograd.grad(out, [r] + list(m.parameters()), grad_outputs=w[:nn_].to(out.dtype), allow_unused=True)
        return out, grads
    out1, g1 = step()
    m.load_state_dict(state)
    out2, g2 = step()
    m.load_state_dict(state)
    assert out1.dtype == torch.bfloat16 and bool(torch.isfinite(out1.float()).all())
    assert torch.equal(out1, out2) and torch.equal(g1[0], g2[0])
    assert float(out1.detach()[k == 0].float().abs().max()) == 0.0
    for (n_, _), a, b in zip(m.named_parameters(), g1[1:], g2[1:]):
        assert a is not None and bool(torch.isfinite(a).all()), n_
        assert float((a - b).norm() / (a.norm() + 1e-30)) < 1e-3, n_
    m.eval()
    sl = 1 << 16
    out_full, _ = step()
    out_sl, _ = step(sl)
    assert torch.equal(out_full[:sl], out_sl)
