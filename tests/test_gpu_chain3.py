"""-m gpu: the fp32 recompute chain (csrc/chain_f32.hip, fused_chain_f32.chain_scores) -- DeepSetFeat + E_score for fp32
features outside autocast -- against the reference's golden vectors, an fp64 evaluation of the oracle module and the
stored-activation fp32 kernels it replaces (fused_deepset.deepset_linear).

Tolerances of this path (products on the fp32 matrix cores = exact fp32 fma chains, fp32 BatchNorm, fp64 statistics):
  scores                 rtol 1e-5 + atol 1e-5 against fp64      (golden fixtures: the fixture tolerances, unchanged)
  parameter gradients    2e-5 of the tensor's largest entry against fp64 (measured 2e-7 .. 2e-6)
"""
import ast
import copy

import pytest
import torch

from conftest import load_golden, t, state_dict_from
from oracle import pooling_oracle as O
import tolerances as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(a, b, rtol, atol):
    torch.testing.assert_close(a.detach().double().cpu(), b.detach().double().cpu(), rtol=rtol, atol=atol)


def _ragged(gen, N, max_views, long_points=0, long_len=150, empty_head=0):
    sizes = torch.randint(0, max_views + 1, (N,), generator=gen)
    if long_points:
        sizes[N // 3:N // 3 + long_points] = long_len       # segments spanning several 32-view tiles
    if empty_head:
        sizes[:empty_head] = 0
    return torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])


def _modules(gen, G, use_num, train, scale=0.4):
    from deepviewagg_amd.modules.multimodal import pooling as P
    ref = O.DeepSetFeat(8, 32, use_num=use_num)
    lin = torch.nn.Linear(32, G)
    with torch.no_grad():
        for p in list(ref.parameters()) + list(lin.parameters()):
            p.copy_(torch.randn(p.shape, generator=gen) * scale)
    ref.train(train)
    dev = P.DeepSetFeat(8, 32, use_num=use_num)
    dev.load_state_dict(ref.state_dict(), strict=True)
    return ref, lin, dev.to(DEV).train(train), copy.deepcopy(lin).to(DEV)


@pytest.mark.parametrize("name", ["pool_group_default_train", "pool_group_default_eval"])
def test_chain3_matches_reference_fixtures(name, monkeypatch):
    """The reference's golden GroupBimodalCSRPool cases through the fp32-class chain (the default fp32 path)."""
    from deepviewagg_amd.modules.multimodal import pooling as P
    from deepviewagg_amd import fused_chain_f32
    calls = []
    real = fused_chain_f32.chain_scores
    monkeypatch.setattr(fused_chain_f32, "chain_scores", lambda *a: (calls.append(1), real(*a))[1])
    g = load_golden(name)
    kwargs = ast.literal_eval(str(g["kwargs"]))
    m = P.GroupBimodalCSRPool(**kwargs)
    m.load_state_dict(state_dict_from(g), strict=True)
    m = m.to(DEV).train(bool(g["train"]))
    csr = t(g["csr"], DEV)
    x_mod, x_map = t(g["x_mod"], DEV).requires_grad_(), t(g["x_map"], DEV)
    assert fused_chain_f32.applicable(m.E_map, m.E_score, x_map, csr)
    out = m(None, x_mod, x_map, csr)
    assert calls, "the module did not take the fp32-class chain"
    close(out, t(g["out"]), **T.FIXTURE_OUT)
    names = [n for n, _ in m.named_parameters()]
    grads = torch.autograd.grad((out * t(g["w"], DEV)).sum(), [x_mod] + list(m.parameters()), allow_unused=True)
    close(grads[0], t(g["grad_x_mod"]), **T.FIXTURE_GRAD_IN)
    for n, gr in zip(names, grads[1:]):
        ref = t(g["gp/" + n])
        gr = gr if gr is not None else torch.zeros_like(ref)
        close(gr, ref, **T.FIXTURE_GRAD_PARAM)
    for k, v in m.state_dict().items():
        if "running" in k:
            close(v, t(g["sd_after/" + k]), **T.FIXTURE_RUNNING)
        if "num_batches_tracked" in k:
            assert int(v) == int(g["sd_after/" + k])


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("G,use_num", [(4, True), (3, False), (2, False), (1, True)])
def test_chain3_scores_vs_fp64(G, use_num, train):
    """Scores and every parameter gradient against the oracle module evaluated in fp64; the stored-activation fp32
    kernels run beside it on the same inputs (their error is printed with -s: 1e-4 .. 2e-3 on the gradients)."""
    from deepviewagg_amd import fused_chain_f32, fused_deepset
    gen = torch.Generator().manual_seed(11 + G)
    N = 6000
    csr = _ragged(gen, N, 9, long_points=20, empty_head=3)
    V = int(csr[-1])
    ref, lin, e_map, e_lin = _modules(gen, G, use_num, train)
    x_map = torch.rand(V, 8, generator=gen)
    w = torch.randn(V, G, generator=gen)
    ref64, lin64 = copy.deepcopy(ref).double(), copy.deepcopy(lin).double()
    s64 = lin64(ref64(x_map.double(), csr))
    g64 = torch.autograd.grad((s64 * w.double()).sum(), list(ref64.parameters()) + list(lin64.parameters()))

    def run(fn, em, el):
        s = fn(em, el, x_map.to(DEV), csr.to(DEV))
        gr = torch.autograd.grad((s * w.to(DEV)).sum(), list(em.parameters()) + list(el.parameters()))
        return s, gr
    assert fused_chain_f32.applicable(e_map, e_lin, x_map.to(DEV), csr.to(DEV))
    e_map2, e_lin2 = copy.deepcopy(e_map), copy.deepcopy(e_lin)
    s3, g3 = run(fused_chain_f32.chain_scores, e_map, e_lin)
    s1, g1 = run(fused_deepset.deepset_linear, e_map2, e_lin2)
    assert s3.shape == (V, G)
    close(s3, s64, **T.CHAIN3_SCORES)
    names = [n for n, _ in ref.named_parameters()] + ["Ws", "bs"]
    for n, a, a1, b in zip(names, g3, g1, g64):
        scale = float(b.abs().max()) + 1e-9
        e3 = float((a.double().cpu() - b).abs().max()) / scale
        e1 = float((a1.double().cpu() - b).abs().max()) / scale
        print(f"{n:34s} chain {e3:.2e}  stored-activation kernels {e1:.2e}")
        assert e3 < T.CHAIN3_PARAM_GRAD, (n, e3, e1)
    if train:       # running statistics follow nn.BatchNorm1d
        ref(x_map, csr)
        for (k, a), b in zip(e_map.state_dict().items(), ref.state_dict().values()):
            if "running" in k:
                close(a, b, **T.ORACLE_RUNNING)


def test_chain3_large_ragged_vs_fp64():
    """V ~ 1.3M views, points of 0 .. 40 views and a few of 500 (fragments of one point across tiles and wavefronts):
    scores against the oracle in fp64; parameter gradients against fp64 with the oracle's own fp32 evaluation (CPU) as
    the yardstick -- at this size every fp32 evaluation flips leaky' on a handful of the 1.7e8 pre-activations that lie
    within rounding of zero, each flip worth ~1e-3 of a gradient entry (the 6000-point cases above have none and hold
    2e-5); bit-identical scores on a second evaluation."""
    from deepviewagg_amd import fused_chain_f32
    gen = torch.Generator().manual_seed(21)
    N = 60000
    csr = _ragged(gen, N, 40, long_points=7, long_len=500, empty_head=50)
    V = int(csr[-1])
    ref, lin, e_map, e_lin = _modules(gen, 4, True, True)
    x_map = torch.rand(V, 8, generator=gen)
    w = torch.randn(V, 4, generator=gen)
    ref64, lin64 = copy.deepcopy(ref).double(), copy.deepcopy(lin).double()
    s64 = lin64(ref64(x_map.double(), csr))
    g64 = torch.autograd.grad((s64 * w.double()).sum(), list(ref64.parameters()) + list(lin64.parameters()))
    xd, cd = x_map.to(DEV), csr.to(DEV)
    s3 = fused_chain_f32.chain_scores(e_map, e_lin, xd, cd)
    close(s3, s64, **T.CHAIN3_SCORES)
    g3 = torch.autograd.grad((s3 * w.to(DEV)).sum(), list(e_map.parameters()) + list(e_lin.parameters()))
    s32 = lin(ref(x_map, csr))
    g32 = torch.autograd.grad((s32 * w).sum(), list(ref.parameters()) + list(lin.parameters()))
    errs, errs32 = {}, {}
    for (n, _), a, a32, b in zip(list(e_map.named_parameters()) + list(e_lin.named_parameters()), g3, g32, g64):
        scale = float(b.abs().max()) + 1e-9
        errs[n] = float((a.double().cpu() - b).abs().max()) / scale
        errs32[n] = float((a32.double() - b).abs().max()) / scale
    print("chain", max(errs.values()), "oracle fp32", max(errs32.values()))
    assert max(errs.values()) < T.CLASS_GATES["grad_param"] + 3 * max(errs32.values()), (errs, errs32)
    # same inputs, second evaluation: bit-identical scores (deterministic statistics)
    s3b = fused_chain_f32.chain_scores(e_map, e_lin, xd, cd)
    assert torch.equal(s3.detach(), s3b.detach())


def test_chain3_edge_cases():
    from deepviewagg_amd import fused_chain_f32
    gen = torch.Generator().manual_seed(5)
    _, _, e_map, e_lin = _modules(gen, 4, True, False)
    # no views at all: left to the stored-activation kernels
    csr = torch.zeros(6, dtype=torch.long, device=DEV)
    assert not fused_chain_f32.applicable(e_map, e_lin, torch.zeros(0, 8, device=DEV), csr)
    # one point with one view; a second backward is refused
    e_map.train()
    csr = torch.tensor([0, 0, 3, 3, 4], dtype=torch.long, device=DEV)
    x = torch.rand(4, 8, generator=gen).to(DEV)
    s = fused_chain_f32.chain_scores(e_map, e_lin, x, csr)
    assert s.shape == (4, 4) and bool(torch.isfinite(s).all())
    s.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="ran twice"):
        s.sum().backward()
    # x_map that needs a gradient is not taken (the generic composition produces it)
    assert not fused_chain_f32.applicable(e_map, e_lin, x.clone().requires_grad_(), csr)
    # more than 4 scores per view stay on the stored-activation kernels
    assert not fused_chain_f32.applicable(e_map, torch.nn.Linear(32, 8).to(DEV), x, csr)
