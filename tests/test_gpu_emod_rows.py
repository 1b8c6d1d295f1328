"""-m gpu: the fused E_mod row kernels (csrc/emod_rows.hip, ``ops.emod_rows``) stage by stage against float64.

Every reference is built from the tensors the stage actually read -- its stored bf16 inputs and the bf16-rounded
weights -- so a gate holds one stage, not the accumulated rounding of the stages before it:

* Linear outputs and input gradients (y_a, y_b, g_a, g_x), elementwise:
  ``|got - ref| <= 0.5 ulp_bf16(ref) + 2^-18 sum_k |a_k b_k|`` (K <= 64 exact products accumulated in fp32 give at most
  K 2^-24 of that sum, then one rounding to bf16).  The operands that are formed in registers and never stored
  (a_a, dy_b, dy_a) are taken from the rowbn kernels on the same stored inputs: the two files share the per-element
  arithmetic (csrc/rowbn_math.h), and those operands are themselves held to float64 below.
* BatchNorm stages given the stored y: ``primitives_ref.rowbn_ref`` and the keys of ``tolerances`` exactly as
  test_gpu_primitives_f64.py uses them (bn_mean / bn_var for the statistics and constants, out, grad_in for dy,
  grad_param for d gamma / d beta, out for the running statistics), the kink of the activation handled the same way.
* dW_a, dW_b: the grad_param key.

Shapes: R = 31 (a partial tile), 32 (one tile), 33 (a tile and one row), 1000 (several wavefronts), 4099 (a ragged
tail over several blocks), and R = 4099 on two blocks (a wavefront walks 16 tiles: several flushes of the fp32
statistics and two partial weight gradients to reduce); the four width triples; counts None and 0..4 with zeros;
slopes 0.2 and 0 -- every (widths, counts, slope) combination occurs, spread over the row counts.
"""
import functools

import pytest
import torch

import primitives_ref as P
import tolerances as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
EPS, MOMENTUM = 1e-5, 0.1
ROWS = [31, 32, 33, 1000, 4099]
WIDTHS = [(32, 32, 32), (64, 64, 64), (64, 32, 64), (32, 64, 32)]


def stage_cases():
    cases = []
    for ri, R in enumerate(ROWS):
        for wi, widths in enumerate(WIDTHS):
            k = (ri + wi) % 4          # over four of the five row counts a width meets all four (counts, slope) pairs
            cases.append((R, widths, bool(k & 1), 0.2 if k < 2 else 0.0, 0))
    cases.append((4099, (64, 64, 64), True, 0.2, 2))
    return cases


def case_id(c):
    R, w, counts, slope, mb = c
    return f"R{R}-{'x'.join(map(str, w))}-{'counts' if counts else 'ones'}-slope{slope:g}" + (f"-blocks{mb}" if mb else "")


@functools.lru_cache(maxsize=None)
def make_case(R, widths, with_counts, seed=0):
    """Inputs of a case on the CPU (left unchanged by every user)."""
    gen = torch.Generator().manual_seed(1000 * R + 10 * widths[0] + widths[1] // 32 + seed)
    c_i, c_m, c_o = widths
    counts = None
    if with_counts:
        counts = torch.randint(0, 5, (R,), generator=gen, dtype=torch.int32)
        counts[:3] = torch.tensor([2, 1, 3], dtype=torch.int32)
        assert int((counts == 0).sum()) > 0
    x = (torch.randn(R, c_i, generator=gen) * 1.5 + 0.5).to(BF16)
    w_a = torch.randn(c_m, c_i, generator=gen) / c_i ** 0.5
    w_b = torch.randn(c_o, c_m, generator=gen) / c_m ** 0.5
    affine = [(torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.5) for c in (c_m, c_o)]
    running = [(torch.randn(c, generator=gen) * 0.3, torch.rand(c, generator=gen) * 2 + 0.5) for c in (c_m, c_o)]
    gview = torch.randint(-32, 33, (R, c_o), generator=gen).float() / 8      # x counts <= 4: exact in bf16
    return dict(x=x, w_a=w_a, w_b=w_b, affine=affine, running=running, counts=counts, gview=gview)


def modules(case):
    """(lin_a, lin_b, bn_a, bn_b) on the device, train mode, with the case's parameters and buffers."""
    (c_m, c_i), c_o = case["w_a"].shape, case["w_b"].shape[0]
    lins = [torch.nn.Linear(c_i, c_m, bias=False), torch.nn.Linear(c_m, c_o, bias=False)]
    bns = [torch.nn.BatchNorm1d(c_m, eps=EPS, momentum=MOMENTUM), torch.nn.BatchNorm1d(c_o, eps=EPS, momentum=MOMENTUM)]
    with torch.no_grad():
        lins[0].weight.copy_(case["w_a"])
        lins[1].weight.copy_(case["w_b"])
        for bn, (g, b), (rm, rv) in zip(bns, case["affine"], case["running"]):
            bn.weight.copy_(g)
            bn.bias.copy_(b)
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
    return [m.to(DEV).train() for m in lins + bns]


def row_counts(case):
    R = case["x"].shape[0]
    cnt = torch.ones(R) if case["counts"] is None else case["counts"].float()
    return cnt, float(cnt.sum())


def run_fused(case, slope, max_blocks):
    """The six passes through ``ops.emod_rows_forward`` / ``ops.emod_rows_backward``: every stored tensor, on the CPU."""
    from deepviewagg_amd import ops
    lin_a, lin_b, bn_a, bn_b = modules(case)
    cnt, n = row_counts(case)
    x = case["x"].to(DEV)
    counts = case["counts"].to(DEV) if case["counts"] is not None else None
    gout = (case["gview"] * cnt.view(-1, 1)).to(BF16).to(DEV)
    fwd = ops.emod_rows_forward(x, counts, lin_a.weight.detach(), lin_b.weight.detach(), bn_a, bn_b, n, slope, slope,
                                max_blocks)
    bwd = ops.emod_rows_backward(gout, x, counts, lin_a.weight.detach(), lin_b.weight.detach(), fwd, n, slope, slope,
                                 True, max_blocks)
    got = {k: v.detach().clone() for k, v in {**fwd, **bwd}.items()}
    got.update(gout=gout, n=n, running=[(bn.running_mean.clone(), bn.running_var.clone()) for bn in (bn_a, bn_b)],
               tracked=[int(bn.num_batches_tracked) for bn in (bn_a, bn_b)])
    torch.cuda.synchronize()
    return got


def rowbn_operand(kind, got, case, layer, slope):
    """The operand a fused pass forms in registers, from the rowbn kernel on the same stored inputs (module docstring):
    ``act`` = bf16(leaky(BN(y))), ``dy`` = bf16 of the BatchNorm backward."""
    from deepviewagg_amd import _lib
    from deepviewagg_amd._lib import check, ptr, stream_of
    lib = _lib.load()
    y, tab = got["y_" + layer], got["tab_" + layer]
    R, C = y.shape
    out = torch.empty_like(y)
    if kind == "act":
        check(lib.dva_rowbn_apply(ptr(y), ptr(tab), ptr(out), R, C, slope, _lib.DVA_BF16, stream_of(y)), "apply")
    else:
        g = got["gout"] if layer == "b" else got["g_a"]
        counts = case["counts"].to(DEV) if case["counts"] is not None else None
        check(lib.dva_rowbn_bwd_apply(ptr(g), ptr(y), ptr(counts), ptr(tab), ptr(got["sm_" + layer]), ptr(out), R, C,
                                      slope, _lib.DVA_BF16, stream_of(y)), "bwd_apply")
    return out


def hold_linear(failures, case, name, got, a, b):
    """``got`` [R, N] bf16 against a [R, K] (stored bf16) times bf16(b [N, K])^T in float64: the rule of the module
    docstring, every element."""
    a64, b64 = a.detach().cpu().double(), b.detach().cpu().to(BF16).double()
    ref, mag = a64 @ b64.T, a64.abs() @ b64.abs().T
    bound = 0.5 * P.ulp(ref, BF16) + 2.0 ** -18 * mag
    ratio = float(((got.detach().cpu().double() - ref).abs() / bound).max())
    print(f"{case:44s} {name:6s} linear   err / bound {ratio:9.3e}")
    if not ratio <= 1.0:
        failures.append((case, name, ratio))


def hold_bn_layer(rep, case, tag, got, data, layer, slope, y, counts, gamma, beta, grow, act, dy, running0):
    """One BatchNorm + LeakyReLU stage given its stored input ``y`` against ``rowbn_ref`` (float64 over the repeated
    rows), as test_gpu_primitives_f64.check_rowbn holds the rowbn kernels.  ``grow`` = the gradient rows the backward
    read (zero where a row has no view): per view, grow / counts."""
    cnt, n = row_counts(data)
    gview = grow.detach().cpu().double() / cnt.clamp(min=1).double().view(-1, 1)
    assert bool((grow.detach().cpu()[cnt == 0] == 0).all())
    y = y.detach().cpu()
    r32f = P.rowbn_ref(y, counts, gamma, beta, slope, None, None, EPS, dtype=torch.float32)
    r64 = P.rowbn_ref(y, counts, gamma, beta, slope, gview, None, EPS, out_got=act, z32=r32f["z"])
    r32 = P.rowbn_ref(y, counts, gamma, beta, slope, gview, None, EPS, side=r64["side"], dtype=torch.float32)
    rep.n_kink = getattr(rep, "n_kink", 0) + r64["n_kink"]
    C = y.shape[1]
    # statistics: the fp64 sums of the fused pass, and the constants the next pass reads
    sums, tab = got["sums_" + layer].cpu(), got["tab_" + layer].cpu().double()
    mean = sums[:C] / n
    em, ev = T.bn_errors(mean, sums[C:] / n - mean * mean, r64["mean"], r64["var"])
    em32, ev32 = T.bn_errors(r32["mean"], r32["var"], r64["mean"], r64["var"])
    rep.add(case, f"{tag} batch mean", "bn_mean", em, em32)
    rep.add(case, f"{tag} batch var", "bn_var", ev, ev32)
    em, ev = T.bn_errors(tab[0], 1.0 / tab[1] ** 2 - EPS, r64["mean"], r64["var"])
    rep.add(case, f"{tag} table mean", "bn_mean", em, em32)
    rep.add(case, f"{tag} table var", "bn_var", ev, ev32)
    assert torch.equal(tab[2].float(), gamma) and torch.equal(tab[3].float(), beta)
    rep.hold(case, f"{tag} act", "out", act, r64["out"], r32["out"])
    rep.hold(case, f"{tag} dy", "grad_in", dy, r64["dy"], r32["dy"])
    rep.hold(case, f"{tag} dgamma", "grad_param", got["dgamma_" + layer], r64["dgamma"], r32["dgamma"])
    rep.hold(case, f"{tag} dbeta", "grad_param", got["dbeta_" + layer], r64["dbeta"], r32["dbeta"])
    # running statistics: nn.BatchNorm1d's update from the batch statistics of the views (unbiased variance)
    rm0, rv0 = running0
    unb = n / max(n - 1.0, 1.0)
    want = lambda r, dt: ((1 - MOMENTUM) * rm0.to(dt) + MOMENTUM * r["mean"].to(dt),
                          (1 - MOMENTUM) * rv0.to(dt) + MOMENTUM * r["var"].to(dt) * unb)
    (m64, v64), (m32, v32) = want(r64, torch.float64), want(r32, torch.float32)
    rm, rv = got["running"][0 if layer == "a" else 1]
    rep.hold(case, f"{tag} running_mean", "out", rm, m64, m32)
    rep.hold(case, f"{tag} running_var", "out", rv, v64, v32)


@pytest.mark.parametrize("case", stage_cases(), ids=case_id)
def test_emod_rows_stages(case):
    R, widths, with_counts, slope, max_blocks = case
    data = make_case(R, widths, with_counts)
    got = run_fused(data, slope, max_blocks)
    name = case_id(case)
    rep = P.Report(f"emod_rows {name}")
    assert got["tracked"] == [1, 1]
    a_a = rowbn_operand("act", got, data, "a", slope)
    dy_b = rowbn_operand("dy", got, data, "b", slope)
    dy_a = rowbn_operand("dy", got, data, "a", slope)
    failures = []
    hold_linear(failures, name, "y_a", got["y_a"], data["x"], data["w_a"])
    hold_linear(failures, name, "y_b", got["y_b"], a_a, data["w_b"])
    hold_linear(failures, name, "g_a", got["g_a"], dy_b, data["w_b"].T)
    hold_linear(failures, name, "g_x", got["g_x"], dy_a, data["w_a"].T)
    (g_a, b_a), (g_b, b_b) = data["affine"]
    hold_bn_layer(rep, name, "a", got, data, "a", slope, got["y_a"], data["counts"], g_a, b_a, got["g_a"], a_a, dy_a,
                  data["running"][0])
    hold_bn_layer(rep, name, "b", got, data, "b", slope, got["y_b"], data["counts"], g_b, b_b, got["gout"], got["out"],
                  dy_b, data["running"][1])
    for tag, dy, act in (("dW_a", dy_a, data["x"]), ("dW_b", dy_b, a_a)):
        d64, a64 = dy.cpu().double(), act.detach().cpu().double()
        rep.hold(name, tag, "grad_param", got[tag.lower()], d64.T @ a64, d64.float().T @ a64.float())
    rep.notes.append(f"{getattr(rep, 'n_kink', 0)} elements inside the LeakyReLU kink window (side taken from the run)")
    rep.check()
    assert not failures, failures


def test_emod_rows_deterministic():
    """Two calls on the same inputs: every stored tensor and every gradient has the same bits (the weight gradients are
    summed without float atomics; the fp64 statistics are rounded to fp32 before anything reads them)."""
    data = make_case(4099, (64, 64, 64), True)
    for max_blocks in (0, 3):
        one, two = run_fused(data, 0.2, max_blocks), run_fused(data, 0.2, max_blocks)
        for k in ("out", "y_a", "y_b", "tab_a", "tab_b", "g_x", "g_a", "dw_a", "dw_b", "dgamma_a", "dbeta_a", "dgamma_b",
                  "dbeta_b"):
            a, b = one[k].contiguous(), two[k].contiguous()
            view = torch.int16 if a.element_size() == 2 else torch.int32
            assert torch.equal(a.view(view), b.view(view)), (max_blocks, k)


def mlp_of(widths, seed=3, **kwargs):
    from deepviewagg_amd.core.common_modules import MLP
    torch.manual_seed(seed)
    mlp = MLP(list(widths), **kwargs).to(DEV).train()
    with torch.no_grad():
        for block in mlp:
            block[1].batch_norm.weight.uniform_(0.5, 1.5)
            block[1].batch_norm.bias.normal_(0.0, 0.5)
    return mlp


def test_emod_rows_dispatch(monkeypatch):
    """What the fused path serves and what keeps the composition of library GEMMs and rowbn passes."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as PL
    calls = []
    real = ops.emod_rows
    monkeypatch.setattr(ops, "emod_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    gen = torch.Generator().manual_seed(5)
    rows = lambda R, C, dt: torch.randn(R, C, generator=gen).to(dt).to(DEV)
    counts = torch.randint(0, 4, (200,), generator=gen, dtype=torch.int32).to(DEV)

    def run(mlp, x, cnt=None, **kw):
        calls.clear()
        out = PL.mlp_on_gathered_rows(mlp, x, cnt, float(cnt.sum()) if cnt is not None else x.shape[0], **kw)
        assert out.shape == (x.shape[0], mlp[-1][0].out_features) and bool(torch.isfinite(out.float()).all())
        return len(calls)

    mlp = mlp_of((64, 64, 64), bias=False)
    assert run(mlp, rows(200, 64, BF16)) == 1
    assert run(mlp, rows(200, 64, BF16), counts) == 1
    assert run(mlp_of((32, 64, 32), bias=False, activation=torch.nn.ReLU()), rows(200, 32, BF16)) == 1
    with torch.autocast("cuda", dtype=BF16):
        assert run(mlp, rows(200, 64, BF16)) == 1
    # the composition keeps: other storage types, eval mode, a hoisted first Linear, wider layers, V-sized rows, another
    # depth, a bias, a misaligned or strided row tensor, the switch
    assert run(mlp, rows(200, 64, torch.float16)) == 0
    assert run(mlp, rows(200, 64, torch.float32)) == 0
    assert run(mlp, rows(200, 64, BF16), first_linear_done=True) == 0
    assert run(mlp, rows(200, 64, BF16), map_rows=False) == 0
    assert run(mlp_of((64, 128, 64), bias=False), rows(200, 64, BF16)) == 0
    assert run(mlp_of((128, 64, 64), bias=False), rows(200, 128, BF16)) == 0
    assert run(mlp_of((64, 64, 64, 64), bias=False), rows(200, 64, BF16)) == 0
    assert run(mlp_of((64, 64, 64), bias=True), rows(200, 64, BF16)) == 0
    assert run(mlp, rows(200, 128, BF16)[:, :64]) == 0
    assert run(mlp, rows(201, 64, BF16).view(-1)[8:8 + 200 * 64].view(200, 64)) == 1            # 16 bytes in: aligned
    assert run(mlp, rows(201, 64, BF16).view(-1)[4:4 + 200 * 64].view(200, 64)) == 0            # 8 bytes in
    assert run(mlp.eval(), rows(200, 64, BF16)) == 0
    mlp.train()
    monkeypatch.setattr(ops, "EMOD_FUSED", False)
    assert run(mlp, rows(200, 64, BF16)) == 0


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def mlp_ref64(data, slope):
    """The two blocks in float64 on the rows with count-weighted batch statistics (= nn.BatchNorm1d over the repeated
    rows), unrounded parameters: out, g_x and the six parameter gradients of sum_v out_v gview_v."""
    cnt, n = row_counts(data)
    w = cnt.double().view(-1, 1)
    x = data["x"].double().requires_grad_()
    params = [data["w_a"].double().requires_grad_(), data["w_b"].double().requires_grad_()]
    aff = [(g.double().requires_grad_(), b.double().requires_grad_()) for g, b in data["affine"]]
    h = x
    for W, (g, b) in zip(params, aff):
        y = h @ W.T
        mean = (w * y).sum(0) / n
        var = (w * (y - mean) ** 2).sum(0) / n
        h = torch.nn.functional.leaky_relu((y - mean) / (var + EPS).sqrt() * g + b, slope)
    leaves = [x, params[0], aff[0][0], aff[0][1], params[1], aff[1][0], aff[1][1]]
    grads = torch.autograd.grad((h * (data["gview"].double() * w)).sum(), leaves)
    return [h.detach()] + list(grads)


AGREE_CASES = [(1000, (64, 64, 64), True, 0.2), (4099, (32, 64, 32), False, 0.0), (1000, (64, 32, 64), True, 0.0),
               (4099, (32, 32, 32), False, 0.2)]


@pytest.mark.parametrize("R,widths,with_counts,slope", AGREE_CASES,
                         ids=[case_id((R, w, c, s, 0)) for R, w, c, s in AGREE_CASES])
def test_emod_rows_agrees_with_composition(R, widths, with_counts, slope, monkeypatch):
    """``pooling.mlp_on_gathered_rows`` with EMOD_FUSED on and off: out, g_x and the six parameter gradients agree in
    relative L2 to 1.5 x the relative L2 error of the composition against float64 on the same case (both round at the
    same points and differ in summation order: the factor covers the elements that round the other way).  All elements."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.core.common_modules.base_modules import FastBatchNorm1d
    from deepviewagg_amd.modules.multimodal import pooling as PL
    data = make_case(R, widths, with_counts, seed=1)
    cnt, n = row_counts(data)
    names = ["out", "g_x", "dW_a", "dgamma_a", "dbeta_a", "dW_b", "dgamma_b", "dbeta_b"]

    def run(fused):
        monkeypatch.setattr(ops, "EMOD_FUSED", fused)
        lin_a, lin_b, bn_a, bn_b = modules(data)
        act = torch.nn.LeakyReLU(slope) if slope else torch.nn.ReLU()
        blocks = []
        for lin, bn in ((lin_a, bn_a), (lin_b, bn_b)):
            holder = FastBatchNorm1d(bn.num_features)
            holder.batch_norm = bn
            blocks.append(torch.nn.Sequential(lin, holder, act))
        mlp = torch.nn.Sequential(*blocks)
        x = data["x"].to(DEV).requires_grad_()
        counts = data["counts"].to(DEV) if with_counts else None
        out = PL.mlp_on_gathered_rows(mlp, x, counts, n)
        leaves = [x, lin_a.weight, bn_a.weight, bn_a.bias, lin_b.weight, bn_b.weight, bn_b.bias]
        grads = torch.autograd.grad(out, leaves, grad_outputs=(data["gview"] * cnt.view(-1, 1)).to(BF16).to(DEV))
        return [out.detach()] + list(grads)

    old, new, ref = run(False), run(True), mlp_ref64(data, slope)
    bad = []
    for name, o, f, r in zip(names, old, new, ref):
        e_old, d = rel_l2(o, r), rel_l2(f, o)
        print(f"{name:9s} composition vs float64 {e_old:9.3e}   fused vs composition {d:9.3e}   ratio {d / e_old:6.3f}"
              f"   fused vs float64 {rel_l2(f, r):9.3e}")
        if not d <= 1.5 * e_old:
            bad.append((name, d, e_old))
    assert not bad, bad
