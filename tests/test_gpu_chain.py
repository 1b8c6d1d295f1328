"""-m gpu: the bf16 recompute chain (csrc/chain_*.hip through fused_chain.py) against the CPU oracle.

Tolerances: the chain feeds bf16-rounded operands to the matrix cores (activations AND weights, like the reference's
Linear layers under torch.autocast(bfloat16)) and keeps accumulation / BatchNorm / softmax in fp32; the value rows
are bf16.  Outputs are compared with the fp32 oracle evaluated on the same bf16-rounded value rows: relative L2
error <= 2e-2 (measured ~3e-3), and against the oracle's own autocast error where stated."""
import numpy as np
import pytest
import torch

import rowwise as RW
from oracle import pooling_oracle as O
from rowwise import edges
from tolerances import AUTOCAST_ROW_HEADROOM, Report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def check_rows_against_autocast(label, out, out_amp, out_ref, csr):
    """The tests whose yardstick is the oracle under CPU autocast (whole-tensor: rel L2 <= 1.5 x the autocast oracle's)
    hold it per row as well (tests/rowwise.py): the max -- and the p99 of strata of >= 200 points -- of the device's row
    error against the fp32 oracle, per stratum of points, <= AUTOCAST_ROW_HEADROOM = 1.5 x the same statistic of the
    autocast oracle over all seen points.  Strata from the device's tile table of ``csr``."""
    from deepviewagg_amd import fused_chain
    csr = csr.cpu()
    seen = csr[1:] > csr[:-1]
    tiles, n_tiles = fused_chain.build_tiles(csr.to(DEV), int(csr[-1]))
    masks = RW.strata(csr, tiles[:int(n_tiles)].cpu(), fused_chain.VIEWS_PER_CHUNK)
    rep = Report("row-wise against the fp32 oracle, yardstick = the oracle under autocast: " + label)
    worst = RW.gate_rows(rep, label, "out", RW.row_err(out, out_ref, seen), RW.row_err(out_amp, out_ref, seen), masks, seen,
                         headroom=AUTOCAST_ROW_HEADROOM)
    print(f"{label}: worst row-wise ratio to the autocast oracle {worst:.2f} (gate {AUTOCAST_ROW_HEADROOM})")
    RW.write_report(rep)
    rep.check()


@pytest.fixture(params=["permutation_plan", "split_plan"])
def plan_kind(request):
    """The whole-chain oracle tests run twice: over the permutation plan + `rows_grad_team_kernel`
    (what V < ops.SPLIT_PLAN_MIN_VIEWS = 2^20 selects by itself) and -- threshold forced to 0 -- over the split plan +
    `bucket_rows_grad_kernel` / the two record passes, the code path the 33.5 M-view headline runs.  Yields a call
    counter; `check_plan_kind` asserts that the split path really was the one that ran."""
    from deepviewagg_amd import ops
    calls = {"kind": request.param, "fused": 0, "sorted": 0}
    if request.param == "permutation_plan":
        yield calls
        return
    old = ops.SPLIT_PLAN, ops.SPLIT_PLAN_MIN_VIEWS, ops.SPLIT_FUSED
    orig_fused, orig_sort = ops.SplitPlan.rows_grad_fused, ops.SplitPlan.sort_records

    def fused(self, *a, **k):
        r = orig_fused(self, *a, **k)
        calls["fused"] += r is not None
        return r

    def sort(self, *a, **k):
        calls["sorted"] += 1
        return orig_sort(self, *a, **k)
    ops.SplitPlan.rows_grad_fused, ops.SplitPlan.sort_records = fused, sort
    ops.SPLIT_PLAN, ops.SPLIT_PLAN_MIN_VIEWS, ops.SPLIT_FUSED = True, 0, True
    try:
        yield calls
    finally:
        ops.SplitPlan.rows_grad_fused, ops.SplitPlan.sort_records = orig_fused, orig_sort
        ops.SPLIT_PLAN, ops.SPLIT_PLAN_MIN_VIEWS, ops.SPLIT_FUSED = old


def check_plan_kind(calls, C):
    if calls["kind"] == "split_plan":
        assert calls["sorted"] >= 1, "the split plan's record pass did not run"
        if C in (32, 64):
            assert calls["fused"] >= 1, "bucket_rows_grad_kernel did not run"       # the headline's rows-gradient kernel
    else:
        assert calls["sorted"] == 0 and calls["fused"] == 0


def make_case(seed, N, C, sizes_fn, B=3, H=12, W=20):
    gen = torch.Generator().manual_seed(seed)
    sizes = sizes_fn(N, gen)
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    V = int(csr[-1])
    images = torch.randint(0, B, (V,), generator=gen)
    pixels = torch.stack([torch.randint(0, W, (V,), generator=gen), torch.randint(0, H, (V,), generator=gen)], 1).short()
    x = torch.randn(B, C, H, W, generator=gen).bfloat16().float()
    x_map = torch.rand(V, 8, generator=gen)
    w = torch.randn(N, C, generator=gen)
    return dict(gen=gen, csr=csr, V=V, images=images, pixels=pixels, x=x, x_map=x_map, w=w, N=N, C=C)


def ragged(N, gen):
    return torch.randint(0, 9, (N,), generator=gen)


def ragged_long(N, gen):
    s = torch.randint(0, 7, (N,), generator=gen)
    s[5] = 100
    s[6] = 33
    s[7] = 64
    s[N - 1] = 70
    return s


def full32(N, gen):
    return torch.full((N,), 32, dtype=torch.long)


def build(case, G, train, gating=True, scaling=True, seed=5, wscale=0.3):
    from deepviewagg_amd.modules.multimodal import pooling as P
    gen = torch.Generator().manual_seed(seed)
    kwargs = dict(in_map=8, in_mod=case["C"], num_groups=G, use_num=True, gating=gating, group_scaling=scaling)
    ref = O.GroupBimodalCSRPool(**kwargs)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * wscale)
            if "batch_norm.weight" in n or n == "G.weight":
                p.add_(1.0)                      # BatchNorm / gate scales around their initial value 1
        for n, b in ref.named_buffers():
            if "running_mean" in n:
                b.copy_(torch.randn(b.shape, generator=gen) * 0.1)
            if "running_var" in n:
                b.copy_(torch.rand(b.shape, generator=gen) + 0.5)
    ref.train(train)
    m = P.GroupBimodalCSRPool(**kwargs)
    m.load_state_dict(ref.state_dict(), strict=True)
    return ref, m.to(DEV).train(train)


def run_dev(case, m, chain, need_grad=True):
    from deepviewagg_amd import ops, fused_chain
    from deepviewagg_amd.modules.multimodal import pooling as P
    V = case["V"]
    xd = case["x"].to(DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(need_grad)
    packed = ops.pack_gather_index(case["images"].to(DEV), torch.arange(V + 1, device=DEV), case["pixels"].to(DEV))
    fused_chain.FORCE = chain
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lazy = ops.lazy_gather_nearest(xd, packed, exact=True)
            lazy = P.BimodalCSRPool(mode='max')(None, lazy, None, torch.arange(V + 1, device=DEV))
            out = m(None, lazy, case["x_map"].to(DEV), case["csr"].to(DEV))
        grads = None
        if need_grad:
            grads = torch.autograd.grad((out.float() * case["w"].to(DEV)).sum(), [xd] + list(m.parameters()),
                                        allow_unused=True)
    finally:
        fused_chain.FORCE = None
    return out, grads


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("sizes_fn,N,C,G", [(ragged, 3000, 64, 4), (ragged_long, 2000, 64, 4), (full32, 300, 64, 4),
                                            (ragged_long, 1500, 32, 2), (ragged, 1500, 128, 1),
                                            (ragged_long, 700, 512, 4), (ragged, 900, 256, 4),
                                            (ragged, 1200, 128, 4),         # staged several-points walk, two channels per lane
                                            (ragged, 20000, 64, 4)])       # eval: the single fused launch at N = 20 k
def test_chain_forward_matches_oracle(sizes_fn, N, C, G, train):
    case = make_case(3, N, C, sizes_fn)
    ref, m = build(case, G, train)
    out_ref = ref(None, O.gather_nearest(case["x"], case["images"], case["pixels"]), case["x_map"], case["csr"])
    out, _ = run_dev(case, m, chain=True, need_grad=False)
    assert out.dtype == torch.bfloat16
    r = rel(out, out_ref)
    ref2, _ = build(case, G, train)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        out_amp = ref2(None, O.gather_nearest(case["x"], case["images"], case["pixels"]), case["x_map"], case["csr"])
    r_amp = rel(out_amp, out_ref)
    print(f"chain fwd rel err {r:.4f}  (reference under autocast: {r_amp:.4f})")
    assert r < max(2e-2, 1.5 * r_amp), (r, r_amp)
    # unseen points stay zero
    unseen = (case["csr"][1:] == case["csr"][:-1])
    assert float(out.detach().float().cpu()[unseen].abs().max() if unseen.any() else 0.0) == 0.0
    if train:
        for (k, a), b in zip(m.state_dict().items(), ref.state_dict().values()):
            if "running" in k:
                torch.testing.assert_close(a.cpu(), b, rtol=2e-2, atol=2e-3)
    check_rows_against_autocast(f"chain fwd {sizes_fn.__name__} N={N} C={C} G={G} {'train' if train else 'eval'}",
                                out, out_amp, out_ref, case["csr"])


def test_tile_table_properties():
    from deepviewagg_amd import fused_chain
    gen = torch.Generator().manual_seed(0)
    for sizes in (ragged_long(5000, gen), full32(257, gen), torch.zeros(100, dtype=torch.long),
                  torch.randint(0, 3, (100000,), generator=gen), torch.randint(20, 45, (3000,), generator=gen),
                  # more than 1024 chunks of 512 views: the offset scan runs over several blocks
                  torch.randint(0, 9, (200000,), generator=gen),
                  torch.cat([torch.randint(0, 70, (30000,), generator=gen), torch.full((7,), 5000)])):
        csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).to(DEV)
        V = int(csr[-1])
        tiles, n = fused_chain.build_tiles(csr, V)
        T = int(n)
        t = tiles[:T].cpu().numpy()
        v0, nv, frag = t[:, 0], t[:, 1] & 0xff, t[:, 1] >> 8
        assert (nv >= 1).all() and (nv <= 32).all()
        assert T == 0 or v0[0] == 0
        assert (v0[1:] == v0[:-1] + nv[:-1]).all() and (T == 0 or v0[-1] + nv[-1] == V)   # exact cover, in order
        starts = set(csr.cpu().numpy().tolist())
        for i in range(T):
            if frag[i] == 0:
                assert v0[i] in starts and (v0[i] + nv[i]) in starts
            if frag[i] in (1, 2):
                assert nv[i] == 32 and frag[i + 1] in (2, 3)
            if frag[i] == 1:
                assert v0[i] in starts
            if frag[i] == 3:
                assert (v0[i] + nv[i]) in starts
        # no point of <= 32 views is split: no tile boundary strictly inside it
        ptr = csr.cpu().numpy()
        small = ((ptr[1:] - ptr[:-1]) <= 32) & (ptr[1:] > ptr[:-1])
        lo = np.searchsorted(v0, ptr[:-1], side='right')     # first cut > start
        hi = np.searchsorted(v0, ptr[1:], side='left')       # first cut >= end
        assert (lo[small] == hi[small]).all()
        # greedy: a tile of whole points is closed only when the next (non-empty) point does not fit any more
        if T > 1:
            nxt_end = ptr[np.minimum(np.searchsorted(ptr, v0[1:], side='right'), len(ptr) - 1)]
            first_size = nxt_end - v0[1:]
            whole = frag[:-1] == 0
            # ... except at the chunk boundaries of the construction (chunks are tiled independently)
            n_chunks = max(1, min(1 << 17, -(-V // fused_chain.VIEWS_PER_CHUNK)))
            assert int((nv[:-1][whole] + first_size[whole] <= 32).sum()) <= n_chunks - 1


def _oracle_grads(case, ref, autocast):
    xr = case["x"].clone().requires_grad_()
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = ref(None, O.gather_nearest(xr, case["images"], case["pixels"]), case["x_map"], case["csr"])
    else:
        out = ref(None, O.gather_nearest(xr, case["images"], case["pixels"]), case["x_map"], case["csr"])
    grads = torch.autograd.grad((out.float() * case["w"]).sum(), [xr] + list(ref.parameters()), allow_unused=True)
    return out, grads


@pytest.mark.parametrize("sizes_fn,N,C,G,train,gating", [
    (ragged, 3000, 64, 4, True, True),
    (ragged_long, 2000, 64, 4, True, True),
    (full32, 4096, 64, 4, True, True),          # the headline instantiation: 32 views / point, bf16, C = 64, G = 4
    (ragged, 3000, 64, 4, False, True),
    (ragged_long, 1500, 32, 2, True, True),
    (ragged, 1500, 128, 1, True, False),
    (ragged, 3000, 128, 4, True, True),
    (ragged_long, 700, 512, 4, True, True),
    (ragged, 3000, 128, 2, False, True),
])
def test_chain_backward_matches_oracle(sizes_fn, N, C, G, train, gating, plan_kind):
    """Gradients w.r.t. the feature maps and every parameter against the fp32 oracle; yardstick = the error of
    the reference maths itself under torch.autocast(bfloat16): per tensor, relative L2 error
    <= max(2 x reference-autocast error, 5e-2) (4 x for the gate / score parameters; for the encoder's parameters the
    reference error is floored by its median over them, see below)."""
    case = make_case(7, N, C, sizes_fn)
    ref, m = build(case, G, train, gating=gating)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    out_ref, g_ref = _oracle_grads(case, ref, autocast=False)
    ref.load_state_dict(sd)
    _, g_amp = _oracle_grads(case, ref, autocast=True)
    out, g = run_dev(case, m, chain=True)
    check_plan_kind(plan_kind, C)
    ref.load_state_dict(sd)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        out_amp = ref(None, O.gather_nearest(case["x"], case["images"], case["pixels"]), case["x_map"], case["csr"])
    assert rel(out, out_ref) < max(2e-2, 1.5 * rel(out_amp, out_ref)), (rel(out, out_ref), rel(out_amp, out_ref))
    names = ["x"] + [n for n, _ in ref.named_parameters()]
    report, bad = [], []
    # The autocast error of one parameter is a single draw of a chaotic quantity (LeakyReLU sign and arg-max flips
    # under a 2^-9 perturbation): for the mapping-feature encoder the yardstick is at least the median autocast
    # error over its parameters, so that one lucky draw of the reference does not set the bar.
    amps = sorted(rel(c, b) for n, b, c in zip(names, g_ref, g_amp) if b is not None and n.startswith("E_map"))
    med = amps[len(amps) // 2] if amps else 0.0
    for n, a, b, c in zip(names, g, g_ref, g_amp):
        if b is None:
            assert a is None or float(a.abs().max()) == 0, n
            continue
        assert a is not None, n
        ours, amp = rel(a, b), rel(c, b)
        report.append((n, round(ours, 4), round(amp, 4)))
        if n.startswith("E_map"):
            amp = max(amp, med)
        # gate / score-bias gradients are sums of per-point terms of both signs routed through an arg-max:
        # a handful of arg-max flips under the bf16 perturbation moves them by several % under either scheme
        loose = n.startswith("G.") or n.startswith("E_score")
        if ours > max((4.0 if loose else 2.0) * amp, 5e-2):
            bad.append(report[-1])
    print("chain bwd rel err (ours, reference under autocast):", report)
    assert not bad, (bad, report)


def test_chain_equals_stored_activation_path():
    """A/B against the first-generation fp32-MFMA kernels with bf16 activation storage on the same inputs."""
    case = make_case(11, 5000, 64, ragged)
    ref, m = build(case, 4, True)
    out_a, g_a = run_dev(case, m, chain=True)
    m.load_state_dict(ref.state_dict())
    out_b, g_b = run_dev(case, m, chain=False)
    assert rel(out_a, out_b) < 2e-2
    assert rel(g_a[0], g_b[0]) < 8e-2, rel(g_a[0], g_b[0])          # gradient w.r.t. the feature maps
    # parameter gradients: both are bf16 perturbations of the same fp32 maths (each 10-20 % off the fp32 oracle in
    # train mode, like the reference under autocast): same direction
    for (n, _), a, b in zip(list(m.named_parameters()), g_a[1:], g_b[1:]):
        if a is None or b is None or float(b.norm()) == 0:
            continue
        cos = float((a.flatten() @ b.flatten()) / (a.norm() * b.norm() + 1e-30))
        assert cos > 0.9, (n, cos)


# ---------------------------------------------------------------------------------------------------------------
# Tight parity: the oracle's maths with the chain's operand roundings made explicit (oracle/chain_emulation.py:
# straight-through bf16 rounding of the activations and weights that enter the matrix-core products, BatchNorm folded
# into the rounded operand where the kernels fold it, the first layer's input to 16 bits; everything else fp32).  The
# backward kernels take leaky' from the sign of the same pre-activation the emulation's autograd differentiates.
# Two kinds of DISCRETE decisions are discontinuous functions of quantities that two evaluations can only agree on to
# fp32 rounding, and each flip moves single gradient entries by O(1) (tests/test_oracle_chaos.py pins how chaotic the
# emulation is against itself; tools/debug_chain.py shows the individual flips):
#   * the rounding of the folded operands bf16(0.6 gamma invstd W) -- a function of the batch statistics;
#   * the arg-max view of a point and the branch of the gate tanh(relu(w max + b)) -- functions of the scores.
# The emulation therefore takes these decisions from the device (dev_invstd = the BatchNorm constants the forward saved,
# dev_scores = the scores the fused forward kernel left for the backward; values only, gradients flow through the
# emulation's own quantities): both sides evaluate the same discrete network.  What is compared:
#   forward: output and scores against the emulation's OWN (nothing substituted but the operand roundings);
#   backward: every gradient against the autograd of the emulation evaluated at the device's scores.
# FIXED tolerances (relative L2 per tensor; measured on the eight cases, profiles/r03_emu_report.txt):
#   output 1e-2 (measured 1.4e-3 .. 2.6e-3; 7.7e-3 without group scaling), scores 5e-3 (0.4e-3 .. 1.7e-3),
#   rows gradient 1e-2 (2.7e-3 .. 2.9e-3),
#   parameter gradients: eval mode 3e-2 (max 2.0e-2); train mode 8e-2 per tensor (max 5.7e-2: a set-branch BatchNorm
#   weight, behind the arg-max of the set pooling) and 3e-2 for the median over the tensors (0.6e-2 .. 2.6e-2).
# ---------------------------------------------------------------------------------------------------------------
EMU_TOL = {"out": 1e-2, "scores": 5e-3, "rows": 1e-2, "param_eval": 3e-2, "param_train": 8e-2,
           "param_train_median": 3e-2}


from oracle.chain_emulation import emulated_chain, _bf      # noqa: E402  (the bf16-emulation oracle)


@pytest.mark.parametrize("sizes_fn,N,C,G,train,gating,scaling", [
    (ragged, 3000, 64, 4, True, True, True),
    (ragged_long, 2000, 64, 4, True, True, True),
    (full32, 2048, 64, 4, True, True, True),       # the headline instantiation
    (ragged_long, 2000, 64, 4, False, True, False),
    (ragged_long, 1500, 32, 2, True, True, True),
    (ragged, 1500, 128, 1, True, False, True),
    (ragged_long, 700, 512, 4, True, True, True),
    (ragged_long, 900, 256, 2, False, True, True),
    (edges, 4001, 64, 4, True, True, True),        # every position class of the tile table, hot and cold map rows
    (full32, 4096, 64, 4, True, True, True),
    (ragged, 3000, 128, 2, False, True, True),
])
def test_chain_matches_bf16_emulation(sizes_fn, N, C, G, train, gating, scaling, plan_kind):
    """Whole-tensor gates (EMU_TOL, below) and -- tests/rowwise.py -- the same comparison per point and per map row,
    by stratum, against the float64 twin of the emulation; the row gates are FP32_HEADROOM x the noise of
    bf16(float32 emulation) against that twin, computed here.  Measured: profiles/rowwise_report.txt."""
    from deepviewagg_amd import ops, fused_chain
    case = make_case(13, N, C, sizes_fn)
    gen = case["gen"]
    V, csr = case["V"], case["csr"]
    R = 777
    rows = (torch.randn(R, C, generator=gen)).bfloat16()
    row_idx = torch.randint(0, R, (V,), generator=gen, dtype=torch.int32)
    if sizes_fn is edges:
        # map rows read by >= 512 views (16 hot rows take 40 % of the views), by 32 .. 511, by a few, by one, by none
        R = 20000
        rows = (torch.randn(R, C, generator=gen)).bfloat16()
        u = torch.rand(V, generator=gen)
        row_idx = torch.where(u < 0.4, torch.randint(0, 16, (V,), generator=gen),
                              torch.where(u < 0.7, torch.randint(16, 1000, (V,), generator=gen),
                                          torch.randint(1000, R, (V,), generator=gen))).int()
    ref, m = build(case, G, train, gating=gating, scaling=scaling)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    chain_params = [p for n, p in ref.named_parameters() if not n.startswith("E_mod")]
    names = [n for n, _ in ref.named_parameters() if not n.startswith("E_mod")]
    # sensitivity of the case: how far the exact fp32 maths is from the emulated arithmetic (the 2^-9 operand
    # roundings are amplified by the BatchNorm gains and, for gradients, by sign / arg-max flips)
    rows_fp = rows.float().requires_grad_()
    compat = ref.E_score(ref.E_map(case["x_map"], csr))
    out_fp, _, _ = O.attention_tail(rows_fp[row_idx.long()], compat, csr, ref.G, ref.num_groups, ref.out_mod,
                                    ref.group_scaling)
    g_fp = torch.autograd.grad((out_fp * case["w"]).sum(), [rows_fp] + chain_params, allow_unused=True)
    ref.load_state_dict(sd)
    # device side: the chain on a GatheredFeatures whose rows are the values
    rows_d = rows.to(DEV).requires_grad_()
    gf = ops.GatheredFeatures(rows_d, row_idx.to(DEV), None, True, None)
    fused_chain.FORCE = True
    try:
        out = fused_chain.chain_pool(m, gf, case["x_map"].to(DEV), csr.to(DEV))
    finally:
        fused_chain.FORCE = None
    # the device's BatchNorm constants of the folded layers (fp32 [5, 32] tables saved for the backward: row 1 = invstd):
    # the emulation takes the rounding decisions of the folded operands from them (oracle/chain_emulation.py)
    saved = out.grad_fn.saved_tensors
    dev_invstd = {1: saved[12][1].cpu(), 2: saved[13][1].cpu(), 6: saved[15][1].cpu()}
    dev_scores = saved[17].cpu()[:, :G]          # the scores the fused forward kernel left for the backward
    # oracle side
    rows_ref = rows.float().requires_grad_()
    with torch.no_grad():      # forward parity: the emulation's own output and scores
        out_plain, sc_own = emulated_chain(ref, rows_ref[row_idx.long()], case["x_map"], csr, dev_invstd=dev_invstd,
                                           return_scores=True, set_split=True)
    ref.load_state_dict(sd)
    # gradient parity: the attention tail evaluated at the device's scores (same arg-max views, same gate branches)
    out_ref = emulated_chain(ref, rows_ref[row_idx.long()], case["x_map"], csr, dev_invstd=dev_invstd,
                             dev_scores=dev_scores, set_split=True)
    g_ref = torch.autograd.grad((out_ref * case["w"]).sum(), [rows_ref] + chain_params, allow_unused=True)
    sens_out = rel(out_ref, out_fp.detach())
    dev_params = [p for n, p in m.named_parameters() if not n.startswith("E_mod")]
    g = torch.autograd.grad((out.float() * case["w"].to(DEV)).sum(), [rows_d] + dev_params, allow_unused=True)
    check_plan_kind(plan_kind, C)
    r_out, r_sc = rel(out, out_plain), rel(dev_scores, sc_own)
    report = [("out", round(r_out, 5)), ("scores", round(r_sc, 5))]
    bad, par = [], []
    for n, a, b, f in zip(["rows"] + names, g, g_ref, g_fp):
        if b is None:
            assert a is None or float(a.abs().max()) == 0, n
            continue
        r = rel(a, b)
        sens = rel(b, f)
        report.append((n, round(r, 5), round(sens, 5)))
        # rows: no chaotic element.  Parameters: a rounding-boundary flip of one bf16 activation (1 view in ~30)
        # moves a score by ~1e-3, which flips the arg-max view of a few near-tied points: their gate gradient
        # lands on another view (measured: 3 views of 65536 carry the whole difference, tools/debug_chain.py)
        if n == "E_score.bias" and not gating:
            continue        # exactly zero in exact arithmetic (softmax is shift invariant): nothing to compare
        if n != "rows":
            par.append(r)
        if r > (EMU_TOL["rows"] if n == "rows" else EMU_TOL["param_train" if train else "param_eval"]):
            bad.append((n, r, sens))
    print("chain vs bf16 emulation, rel L2 (kernel vs emulation, emulation vs fp32):", report)
    import os
    if os.path.isdir("gpurun_out"):
        with open("gpurun_out/emu_report_r3.txt", "a") as f:
            f.write(f"{sizes_fn.__name__} N={N} C={C} G={G} train={train} gating={gating} scaling={scaling} "
                    f"sens_out={sens_out:.5f} {report}\n")
    assert r_out < EMU_TOL["out"], (report, sens_out)      # bf16 rounding of the output itself: 2^-9
    assert r_sc < EMU_TOL["scores"], report
    assert rel(out, out_ref) < EMU_TOL["out"]
    assert not bad, (bad, report)
    # What sharing the scores hides, bounded: the gradient leg above evaluates the tail at the DEVICE's scores,
    # so a device score error that moved an arg-max view would be invisible to it.  Independent statement on the scores
    # themselves: the arg-max view of a (point, group) may differ between the device's scores and the emulation's own
    # only where the two best scores of that point are within the score tolerance of each other (a near-tie that either
    # arithmetic may break either way), and only on a small fraction of the points.
    sizes = (csr[1:] - csr[:-1])
    seen = sizes > 0
    pid = torch.repeat_interleave(torch.arange(N), sizes)
    big = 1e30
    flips = near = 0
    for gi in range(G):
        for sc_a, sc_b in ((dev_scores[:, gi], sc_own[:, gi]),):
            def arg_of(sc):
                mx = torch.full((N,), -big).scatter_reduce(0, pid, sc, "amax")
                first = torch.full((N,), V, dtype=torch.long).scatter_reduce(
                    0, pid, torch.where(sc == mx[pid], torch.arange(V), torch.full((V,), V)), "amin")
                second = torch.full((N,), -big).scatter_reduce(
                    0, pid, torch.where(torch.arange(V) == first[pid], torch.full((V,), -big), sc), "amax")
                return first, mx - second
            fa, gap_a = arg_of(sc_a)
            fb, gap_b = arg_of(sc_b)
            moved = seen & (fa != fb)
            flips += int(moved.sum())
            scale = float(sc_b.abs().max())
            near += int((moved & (torch.minimum(gap_a, gap_b) <= 2 * EMU_TOL["scores"] * scale)).sum())
    assert flips == near, f"{flips - near} arg-max views differ although the two best scores are not near-tied"
    assert flips <= max(2, 0.01 * int(seen.sum()) * G), (flips, int(seen.sum()))
    if train:
        med = sorted(par)[len(par) // 2]
        assert med < EMU_TOL["param_train_median"], (med, report)
        for (k, a), b in zip(m.state_dict().items(), ref.state_dict().values()):
            if "running" in k and not k.startswith("E_mod"):
                torch.testing.assert_close(a.cpu(), b, rtol=1e-3, atol=1e-4)
    # ---- row-wise: per point / per map row, by stratum, against the float64 twin of the emulation (tests/rowwise.py) ----
    assert RW.VIEWS_PER_CHUNK == fused_chain.VIEWS_PER_CHUNK
    tiles, n_tiles = fused_chain.build_tiles(csr.to(DEV), V)
    masks = RW.strata(csr, tiles[:int(n_tiles)].cpu(), fused_chain.VIEWS_PER_CHUNK)
    read, read_live = RW.read_strata(row_idx, R)
    if sizes_fn is edges:
        for k, mk in list(masks.items()) + list(read.items()):
            assert int(mk.sum()) >= (1 if k.startswith("cloud_") else 16), (k, int(mk.sum()))
        assert int((~read_live).sum()) >= 16
    ev = RW.emulate_all(ref, sd, rows, row_idx, case["x_map"], csr, case["w"], dev_invstd, dev_scores)
    label = f"{sizes_fn.__name__} N={N} C={C} {'train' if train else 'eval'} {plan_kind['kind'][:5]}"
    rep = Report("bf16 chain against the float64 emulation, row-wise: " + label)
    worst = RW.gate_chain(rep, label, ev, csr, masks, out, dev_scores, g[0], read, read_live)
    print("worst ratio to the float32 emulation's own noise:", {k: round(v, 2) for k, v in worst.items()})
    RW.write_report(rep)
    rep.check()


# ---------------------------------------------------------------------------------------------------------------
# The reference's own output for the headline instantiation (fixtures written by oracle/gen_golden.py pools_headline
# from the reference source: C = 64, G = 4, points with exactly 32 views, with 40 / 70 views, unseen points).  The
# chain runs in bf16 on values that lie on the bf16 grid; yardstick = the oracle under torch.autocast(bfloat16).
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pool_group_c64_train", "pool_group_c64_eval"])
def test_chain_against_reference_fixture(name, plan_kind):
    import ast
    from conftest import load_golden, t, state_dict_from
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    g = load_golden(name)
    kwargs = ast.literal_eval(str(g["kwargs"]))
    train = bool(g["train"])
    csr, x_map, w = t(g["csr"]), t(g["x_map"]), t(g["w"])
    V = x_map.shape[0]
    m = P.GroupBimodalCSRPool(**kwargs)
    m.load_state_dict(state_dict_from(g), strict=True)
    m = m.to(DEV).train(train)
    rows = t(g["x_mod"], DEV).bfloat16().requires_grad_()            # exact: the fixture's values are bf16 numbers
    # every view its own map row: E_mod on the rows == E_mod on the gathered values
    gf = ops.GatheredFeatures(rows, torch.arange(V, dtype=torch.int32, device=DEV),
                              torch.ones(V, dtype=torch.int32, device=DEV), True, None)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(None, gf, x_map.to(DEV), csr.to(DEV))
    assert out.dtype == torch.bfloat16, "the recompute chain must be the path that ran"
    grads = torch.autograd.grad((out.float() * w.to(DEV)).sum(), [rows] + list(m.parameters()), allow_unused=True)
    check_plan_kind(plan_kind, rows.shape[1])
    # yardstick: the oracle under autocast against the same fixture
    ref = O.GroupBimodalCSRPool(**kwargs)
    ref.load_state_dict(state_dict_from(g), strict=True)
    ref.train(train)
    xr = t(g["x_mod"]).requires_grad_()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        out_amp = ref(None, xr, x_map, csr)
    g_amp = torch.autograd.grad((out_amp.float() * w).sum(), [xr] + list(ref.parameters()), allow_unused=True)
    r, r_amp = rel(out, t(g["out"])), rel(out_amp, t(g["out"]))
    print(f"chain vs reference fixture {name}: out {r:.4f} (oracle under autocast {r_amp:.4f})")
    assert r < max(2e-2, 1.5 * r_amp), (r, r_amp)
    unseen = csr[1:] == csr[:-1]
    assert float(out.detach().float().cpu()[unseen].abs().max()) == 0.0
    check_rows_against_autocast(f"fixture {name} {plan_kind['kind'][:5]}", out, out_amp, t(g["out"]), csr)
    names = ["x_mod"] + [n for n, _ in m.named_parameters()]
    refs = [t(g["grad_x_mod"])] + [t(g["gp/" + n]) for n in names[1:]]
    amps = sorted(rel(c, b) for n, b, c in zip(names, refs, g_amp) if c is not None and n.startswith("E_map"))
    med = amps[len(amps) // 2]
    bad, report = [], []
    for n, a, b, c in zip(names, grads, refs, g_amp):
        assert a is not None, f"no gradient for {n}"
        if float(b.abs().max()) == 0:
            assert float(a.abs().max()) == 0, n
            continue
        ours, amp = rel(a, b), (rel(c, b) if c is not None else 0.0)
        report.append((n, round(ours, 4), round(amp, 4)))
        if n.startswith("E_map"):
            amp = max(amp, med)
        loose = n.startswith("G.") or n.startswith("E_score")
        if ours > max((4.0 if loose else 2.0) * amp, 5e-2):
            bad.append(report[-1])
    print("chain vs reference fixture, gradients (ours, oracle under autocast):", report)
    assert not bad, (bad, report)
    if train:
        for k, v in m.state_dict().items():
            if "running" in k:
                torch.testing.assert_close(v.cpu(), t(g["sd_after/" + k]), rtol=2e-2, atol=2e-3)


def test_two_fused_pool_nodes_two_backwards_without_zero_grad():
    """the small zero-filled accumulators of a step are pieces of one pool (ops.zeros_small); pieces
    are saved for backward (BatchNorm moments) and returned as parameter gradients.  As views of the pool tensor they
    shared ONE autograd version counter: AccumulateGrad's in-place `grad += new` after the first fused node (.grad already
    defined: gradient accumulation) invalidated the saved pieces of the next node of the same graph ("modified by an
    inplace operation").  Two fused pooling nodes in one graph, two forward / backward iterations, no zero_grad."""
    from deepviewagg_amd import ops, fused_chain
    from deepviewagg_amd.modules.multimodal import pooling as P
    case = make_case(17, 2500, 64, ragged)
    _, m = build(case, 4, False)              # eval mode: both iterations evaluate the same function
    V = case["V"]
    xd = case["x"].to(DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_()
    packed = ops.pack_gather_index(case["images"].to(DEV), torch.arange(V + 1, device=DEV), case["pixels"].to(DEV))
    x_map2 = torch.rand(V, 8, generator=case["gen"]).to(DEV)
    grads = []
    fused_chain.FORCE = True
    try:
        for _ in range(2):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                lazy = ops.lazy_gather_nearest(xd, packed, exact=True)
                lazy = P.BimodalCSRPool(mode='max')(None, lazy, None, torch.arange(V + 1, device=DEV))
                out1 = m(None, lazy, case["x_map"].to(DEV), case["csr"].to(DEV))
                out2 = m(None, lazy, x_map2, case["csr"].to(DEV))
            loss = ((out1.float() + 0.5 * out2.float()) * case["w"].to(DEV)).sum()
            loss.backward()                   # second iteration: .grad defined, AccumulateGrad adds in place
            grads.append([p.grad.clone() for p in m.parameters() if p.grad is not None] + [xd.grad.clone()])
    finally:
        fused_chain.FORCE = None
    assert len(grads[0]) > 10
    for a, b in zip(*grads):
        assert rel(b, 2 * a.float()) < 2e-3   # the same gradients once more (atomics' order only)


def test_zero_pool_pieces_have_their_own_version_counter():
    from deepviewagg_amd import ops
    a = ops.zeros_small(40, torch.float64, DEV)
    b = ops.zeros_small((3, 5), torch.float32, DEV)
    assert a._base is None and b._base is None and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
    va, vb = a._version, b._version
    a.add_(1.0)
    assert a._version == va + 1 and b._version == vb
    assert float(b.abs().max()) == 0.0 and float(a.sum()) == 40.0 and b.shape == (3, 5) and b.is_contiguous()
