"""-m gpu: the fp32 pooling path held to float64 at the gates of tests/tolerances.py.

1. The ten reference fixtures with a float64 twin (<name>_f64.npz) through the product modules in fp32: the default
   dispatch (the fp32 chain for <= 4 scores), the stored-activation passes (fused_chain_f32.ENABLED = False) and the
   save_last composition (C / A / G and the x_map gradient exist only there).
2. Large random module cases on the fp32 headline dataflow (lazy nearest gather -> E_mod on the map rows -> fp32
   scores -> view_gather_attention -> rows gradient into the feature map) against the oracle module in .double() on
   the device, over the permutation and the split row plan, with a bf16-autocast negative control.
3. Train-mode BatchNorm statistics at the headline size (N = 2^20 x 32 views) against the chunked float64
   restatement of oracle/deepset_f64.py, and gradients at V = 2^23 against float64 autograd of the oracle module.

-s prints one table of measured error against gate per test.
"""
import ast
import copy

import pytest
import torch

from conftest import load_golden, t, state_dict_from
from oracle import pooling_oracle as O
from oracle.deepset_f64 import LAYERS, deepset_scores_f64
import tolerances as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

F64_CASES = ["pool_group_default_train", "pool_group_default_eval", "pool_group_docstring",
             "pool_group_usemod_nogate", "pool_group_mlpset_g1", "pool_group_minmaxpool",
             "pool_qkv_default", "pool_qkv_modqk", "pool_group_c64_train", "pool_group_c64_eval"]


@pytest.fixture
def spies(monkeypatch):
    """Counts the calls of the fp32 chain and of the stored-activation passes."""
    from deepviewagg_amd import fused_chain_f32, fused_deepset
    calls = {"chain": 0, "stored": 0}
    real_c, real_s = fused_chain_f32.chain_scores, fused_deepset.deepset_linear

    def chain(*a, **k):
        calls["chain"] += 1
        return real_c(*a, **k)

    def stored(*a, **k):
        calls["stored"] += 1
        return real_s(*a, **k)
    monkeypatch.setattr(fused_chain_f32, "chain_scores", chain)
    monkeypatch.setattr(fused_deepset, "deepset_linear", stored)
    monkeypatch.setattr(fused_chain_f32, "ENABLED", fused_chain_f32.ENABLED)      # restored on teardown
    return calls


def _fixture_run(name, path, spies):
    from deepviewagg_amd.modules.multimodal import pooling as P
    from deepviewagg_amd import fused_chain_f32
    g, r = load_golden(name), load_golden(name + "_f64")
    kwargs = ast.literal_eval(str(g["kwargs"]))
    qkv = "qkv" in name
    cls = P.QKVBimodalCSRPool if qkv else P.GroupBimodalCSRPool
    save_last = path == "save_last"
    m = cls(save_last=save_last, **kwargs)
    m.load_state_dict(state_dict_from(g), strict=True)
    m = m.to(DEV).train(bool(g["train"]))
    fused_chain_f32.ENABLED = path != "stored"
    csr = t(g["csr"], DEV)
    x_mod = t(g["x_mod"], DEV).requires_grad_()
    x_map = t(g["x_map"], DEV).requires_grad_(save_last)
    x_main = t(g["x_main"], DEV).requires_grad_() if "x_main" in g else None
    out = m(x_main, x_mod, x_map, csr)
    deepset = (kwargs.get("map_encoder", "DeepSetFeat") == "DeepSetFeat" and kwargs["in_map"] == 8
               and kwargs.get("pool", "max") == "max" and kwargs.get("fusion", "concatenation") == "concatenation")
    fused = deepset and not save_last and not kwargs.get("use_mod" if not qkv else "use_mod_k", False)
    chain = fused and not qkv and kwargs.get("num_groups", 1) <= 4 and path == "default"
    assert spies["chain"] == int(chain), (path, spies)
    assert spies["stored"] == int(fused and not chain), (path, spies)
    ins = {"grad_x_mod": x_mod}
    if save_last:
        ins["grad_x_map"] = x_map
    if x_main is not None:
        ins["grad_x_main"] = x_main
    names = [n for n, _ in m.named_parameters()]
    grads = torch.autograd.grad((out * t(g["w"], DEV)).sum(), list(ins.values()) + list(m.parameters()),
                                allow_unused=True)
    rep = T.Report(f"{name} [{path}]")

    def e32(key, scale=None):
        if key not in g or key not in r:
            return None
        return T.rel_err(t(g[key]), t(r[key]), None if scale is None else t(scale))

    rep.add(name, "out", "out", T.rel_err(out, t(r["out"])), e32("out"))
    if save_last:
        for k in ("C", "A", "G"):
            if "last_" + k in r:
                rep.add(name, "last_" + k, "out", T.rel_err(getattr(m, "_last_" + k), t(r["last_" + k])),
                        e32("last_" + k))
    for (key, _), gr in zip(ins.items(), grads):
        rep.add(name, key, "grad_in", T.rel_err(gr, t(r[key])), e32(key))
    g64 = {n: t(r["gp/" + n]) for n in names}
    for n, gr in zip(names, grads[len(ins):]):
        ref = g64[n]
        gr = gr if gr is not None else torch.zeros_like(ref)
        scale = T.param_scale(n, g64)
        rep.add(name, n, "grad_param", T.rel_err(gr, ref, scale),
                None if "gp/" + n not in g else T.rel_err(t(g["gp/" + n]), ref, scale))
    for k, v in m.state_dict().items():
        if "running" in k:
            rep.add(name, k, "out", T.rel_err(v, t(r["sd_after/" + k])), e32("sd_after/" + k))
    rep.check()


@pytest.mark.parametrize("path", ["default", "stored", "save_last"])
@pytest.mark.parametrize("name", F64_CASES)
def test_fixture_vs_f64(name, path, spies):
    _fixture_run(name, path, spies)


# ---------------------------------------------------------------------------------------------------------------
# 2. large random module cases on the fp32 headline dataflow
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["permutation_plan", "split_plan"])
def row_plan_kind(request, monkeypatch):
    """fp32 value rows at C = 64: the split plan's rows gradient is ``SplitPlan.rows_grad_f32`` (pass A on the 32-byte
    records of the lean attention backward + the fp32 bucket kernel); the permutation plan's is
    ``dva_view_gather_rows_grad``.  Counts the calls of ``rows_grad_f32`` that returned a tensor and those that did not."""
    from deepviewagg_amd import ops
    calls = {"kind": request.param, "f32_bucket": 0, "f32_declined": 0}
    orig = ops.SplitPlan.rows_grad_f32

    def rows_grad_f32(self, *a, **k):
        res = orig(self, *a, **k)
        calls["f32_bucket" if res is not None else "f32_declined"] += 1
        return res
    monkeypatch.setattr(ops.SplitPlan, "rows_grad_f32", rows_grad_f32)
    if request.param == "split_plan":
        monkeypatch.setattr(ops, "SPLIT_PLAN", True)
        monkeypatch.setattr(ops, "SPLIT_PLAN_MIN_VIEWS", 0)
        monkeypatch.setattr(ops, "SPLIT_FUSED", True)
    else:                                           # these scenes are above the threshold: keep the permutation plan
        monkeypatch.setattr(ops, "SPLIT_PLAN_MIN_VIEWS", 1 << 62)
    return calls


def check_rows_grad_kernel(calls):
    if calls["kind"] == "split_plan":
        assert calls["f32_bucket"] == 1 and calls["f32_declined"] == 0, calls
    else:
        assert calls["f32_bucket"] == 0 and calls["f32_declined"] == 0, calls


LB, LC, LH, LW = 4, 64, 32, 32           # feature map [4, 64, 32, 32]: 4096 map rows


@pytest.fixture(scope="module")
def large_scene():
    gen = torch.Generator().manual_seed(123)
    N = 1 << 17
    sizes = torch.randint(0, 49, (N,), generator=gen)
    sizes[torch.randint(0, N, (6,), generator=gen)] = 500                 # a few points of ~500 views
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    V = int(csr[-1])
    images = torch.randint(0, LB, (V,), generator=gen)
    pixels = torch.stack([torch.randint(0, LW, (V,), generator=gen), torch.randint(0, LH, (V,), generator=gen)], 1)
    hot = torch.rand(V, generator=gen) < 0.03                              # 16 map rows read by ~6000 views each
    k = int(hot.sum())
    images[hot] = torch.randint(0, 2, (k,), generator=gen)
    pixels[hot] = torch.stack([torch.randint(0, 4, (k,), generator=gen), torch.randint(0, 2, (k,), generator=gen)], 1)
    pixels = pixels.short()
    x = torch.randn(LB, LC, LH, LW, generator=gen)
    x_map = torch.rand(V, 8, generator=gen)
    x_main = torch.randn(N, 6, generator=gen)
    w = torch.randn(N, LC, generator=gen)
    return dict(gen=gen, N=N, V=V, csr=csr.to(DEV), images=images.to(DEV), pixels=pixels.to(DEV), x=x.to(DEV),
                x_map=x_map.to(DEV), x_main=x_main.to(DEV), w=w.to(DEV))


def _large_modules(cls_name, train, seed):
    from deepviewagg_amd.modules.multimodal import pooling as P
    gen = torch.Generator().manual_seed(seed)
    kwargs = dict(in_map=8, in_mod=LC, num_groups=4, use_num=True)
    if cls_name.startswith("QKV"):
        kwargs.update(in_main=6, nc_qk=4)
    ref = getattr(O, cls_name)(**kwargs)
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.4)
        for mod in ref.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):      # running statistics that differ from the batch's
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=gen) * 0.3)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=gen) + 0.5)
    ref.train(train)
    m = getattr(P, cls_name)(**kwargs)
    m.load_state_dict(ref.state_dict(), strict=True)
    return ref, m.to(DEV).train(train)


def _oracle_eval(ref, s, dtype):
    r = copy.deepcopy(ref).to(DEV).to(dtype)
    x = s["x"].to(dtype).requires_grad_()
    x_mod = O.gather_nearest(x, s["images"], s["pixels"])
    x_main = s["x_main"].to(dtype) if hasattr(r, "E_main") else None
    out = r(x_main, x_mod, s["x_map"].to(dtype), s["csr"])
    grads = torch.autograd.grad((out * s["w"].to(dtype)).sum(), [x] + list(r.parameters()), allow_unused=True)
    names = [n for n, _ in r.named_parameters()]
    running = {k: v for k, v in r.state_dict().items() if "running" in k}
    return out.detach(), grads[0], dict(zip(names, grads[1:])), running


def _device_eval(m, s, autocast=False):
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    V = s["V"]
    x = s["x"].clone().requires_grad_()
    packed = ops.pack_gather_index(s["images"], torch.arange(V + 1, device=DEV), s["pixels"])
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        lazy = ops.lazy_gather_nearest(x, packed, exact=True)
        lazy = P.BimodalCSRPool(mode='max')(None, lazy, None, torch.arange(V + 1, device=DEV))
        assert isinstance(lazy, ops.GatheredFeatures)
        x_main = s["x_main"] if isinstance(m, P.QKVBimodalCSRPool) else None
        out = m(x_main, lazy, s["x_map"], s["csr"])
    grads = torch.autograd.grad((out.float() * s["w"]).sum(), [x] + list(m.parameters()), allow_unused=True)
    names = [n for n, _ in m.named_parameters()]
    return out.detach().float(), grads[0].float(), dict(zip(names, grads[1:]))


# Open findings of the eval-mode cases, one tensor each; every other tensor of these cases is held to its gate.
# What was measured: the eval-mode scores of both kernels are as close to float64 as the oracle's own fp32 evaluation
# (chain 8.4e-7, stored 1.1e-6 / 3.6e-7, oracle fp32 1.3e-6 / 4.8e-7); over all E_map gradients the kernels' worst
# tensor is within 2x of the oracle fp32's worst (Group 4.5e-4 vs 2.8e-4, QKV 2.3e-3 vs 1.2e-3), in a different tensor;
# one QKV gating pre-activation lies 1.7e-7 (of the largest) from zero, inside the fp32 rounding of the compatibilities,
# where a relu' flip moves G.weight's gradient by a whole point's term.  The likely cause is such derivative flips at
# pre-activations within fp32 rounding of zero rather than a kernel defect; it is not proven, so the rows stay open.
OPEN_EVAL = {
    ("GroupBimodalCSRPool", "E_map.mlp_elt_1.1.1.batch_norm.weight"): 2.55e-4,    # oracle fp32: 6.0e-5
    ("QKVBimodalCSRPool", "G.weight"): 7.7e-5,                                      # oracle fp32: 2e-7 .. 6e-7
}
OPEN_WHY = "eval mode: likely a relu' / leaky' flip at a pre-activation within fp32 rounding of zero"


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("cls_name", ["GroupBimodalCSRPool", "QKVBimodalCSRPool"])
def test_large_module_vs_f64(cls_name, train, large_scene, row_plan_kind, spies):
    s = large_scene
    ref, m = _large_modules(cls_name, train, seed=7 + train)
    out, gx, gp = _device_eval(m, s)
    group = cls_name.startswith("Group")
    assert spies["chain"] == int(group) and spies["stored"] == int(not group), spies
    check_rows_grad_kernel(row_plan_kind)
    o64, gx64, gp64, run64 = _oracle_eval(ref, s, torch.float64)
    o32, gx32, gp32, run32 = _oracle_eval(ref, s, torch.float32)
    case = f"{cls_name[:5]} {'train' if train else 'eval'} {row_plan_kind['kind']}"
    rep = T.Report(f"large random V={s['V']}: {case}")
    rep.add(case, "out", "out", T.rel_err(out, o64), T.rel_err(o32, o64))
    rep.add(case, "grad_x (feature map)", "grad_in", T.rel_err(gx, gx64), T.rel_err(gx32, gx64))
    for n, ref_g in gp64.items():
        if ref_g is None:
            assert gp[n] is None or float(gp[n].abs().max()) == 0, n
            continue
        got = gp[n] if gp[n] is not None else torch.zeros_like(ref_g)
        scale = T.param_scale(n, {k: v for k, v in gp64.items() if v is not None})
        err, err32 = T.rel_err(got, ref_g, scale), T.rel_err(gp32[n], ref_g, scale)
        if not train and (cls_name, n) in OPEN_EVAL:
            rep.add_open(case, n, "grad_param", err, err32, OPEN_EVAL[(cls_name, n)], OPEN_WHY)
        else:
            rep.add(case, n, "grad_param", err, err32)
    for k, v in m.state_dict().items():
        if "running" in k:
            rep.add(case, k, "out", T.rel_err(v, run64[k]), T.rel_err(run32[k], run64[k]))
    rep.check()


def test_large_module_bf16_autocast_misses_the_fp32_gates(large_scene):
    """Negative control: the same Group case under autocast(bfloat16) misses the fp32 gates of `out` and of the
    feature-map gradient by at least 10x -- the gates tell the two precisions apart."""
    s = large_scene
    ref, m = _large_modules("GroupBimodalCSRPool", True, seed=8)
    o64, gx64, _, _ = _oracle_eval(ref, s, torch.float64)
    out, gx, _ = _device_eval(m, s, autocast=True)
    e_out, e_gx = T.rel_err(out, o64), T.rel_err(gx, gx64)
    print(f"\nbf16 autocast: out {e_out:.2e} (fp32 gate {T.gate('out'):.0e}), feature-map gradient {e_gx:.2e} "
          f"(fp32 gate {T.gate('grad_in'):.0e})")
    assert e_out >= 10 * T.gate("out") and e_gx >= 10 * T.gate("grad_in"), (e_out, e_gx)


# ---------------------------------------------------------------------------------------------------------------
# 3. train-mode BatchNorm statistics at the headline size
# ---------------------------------------------------------------------------------------------------------------
FN, FVIEWS = 1 << 20, 32


def _bn_layers(e_map):
    return {name: getattr(e_map, name.split(".")[0])[int(name.split(".")[1])][1].batch_norm for name in LAYERS}


def _headline_module():
    from deepviewagg_amd.modules.multimodal import pooling as P
    torch.manual_seed(5)
    m = P.GroupBimodalCSRPool(in_map=8, in_mod=64, num_groups=4, use_num=True)
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if "batch_norm" in n_:
                p.add_(0.2 * torch.randn_like(p))
    for bn in m.modules():
        if isinstance(bn, torch.nn.BatchNorm1d):
            bn.momentum = 1.0           # after one train forward: running = batch mean / unbiased batch variance
    return m.to(DEV).train()


def _x_map(V, dist, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.rand(V, 8, generator=g, device=DEV)
    return x if dist == "rand" else 1.0 + 0.03 * x


_F64_CACHE = {}


def _full_reference(dist):
    if dist not in _F64_CACHE:
        _F64_CACHE.clear()
        V = FN * FVIEWS
        m = _headline_module()
        x_map = _x_map(V, dist, 17)
        csr = torch.arange(0, V + 1, FVIEWS, device=DEV)
        stats, scores = deepset_scores_f64(m.E_map, m.E_score, x_map, csr)
        stats32, scores32 = deepset_scores_f64(m.E_map, m.E_score, x_map, csr, dtype=torch.float32)
        yard = {k: T.bn_errors(stats32[k][0], stats32[k][1], stats[k][0], stats[k][1]) for k in LAYERS}
        yard["scores"] = T.rel_err(scores32, scores)
        # yardstick: torch.var_mean in fp32 on the first layer's z
        z1 = x_map @ m.E_map.mlp_elt_1[0][0].weight.detach().T
        var32, mean32 = torch.var_mean(z1, 0, unbiased=False)
        mean64, var64, _ = stats["mlp_elt_1.0"]
        ratio = (mean64.abs() / var64.sqrt()).cpu()
        del z1
        _F64_CACHE[dist] = dict(stats=stats, scores=scores, yard=T.bn_errors(mean32, var32, mean64, var64),
                                ratio=ratio, fp32=yard)
    return _F64_CACHE[dist]


@pytest.mark.parametrize("path", ["chain", "stored"])
@pytest.mark.parametrize("dist", ["rand", "shifted"])
def test_full_size_train_statistics_vs_f64(dist, path):
    from deepviewagg_amd import fused_chain_f32, fused_deepset
    ref = _full_reference(dist)
    V = FN * FVIEWS
    m = _headline_module()
    x_map = _x_map(V, dist, 17)
    csr = torch.arange(0, V + 1, FVIEWS, device=DEV)
    with torch.no_grad():
        if path == "chain":
            assert fused_chain_f32.applicable(m.E_map, m.E_score, x_map, csr)
            s = fused_chain_f32.chain_scores(m.E_map, m.E_score, x_map, csr)
        else:
            assert fused_deepset.applicable(m.E_map, m.E_score, x_map)
            s = fused_deepset.deepset_linear(m.E_map, m.E_score, x_map, csr)
    case = f"V=2^25 x_map={dist} {path}"
    r = ref["ratio"]
    print(f"\n{case}: |mean|/sd of layer-1 channels: min {float(r.min()):.1f} median {float(r.median()):.1f} "
          f"max {float(r.max()):.1f}; torch.var_mean fp32 on z1: mean {ref['yard'][0]:.2e} sd, var {ref['yard'][1]:.2e}")
    rep = T.Report(case)
    for name, bn in _bn_layers(m.E_map).items():
        mean64, var64, n = ref["stats"][name]
        var = bn.running_var.double() * (n - 1) / n
        em, ev = T.bn_errors(bn.running_mean, var, mean64, var64)
        rep.add(case, name + " mean", "bn_mean", em, ref["fp32"][name][0])
        rep.add(case, name + " var", "bn_var", ev, ref["fp32"][name][1])
    n_s = ref["scores"].shape[0]
    rep.add(case, "scores[:2^16 points]", "out", T.rel_err(s[:n_s], ref["scores"]), ref["fp32"]["scores"])
    rep.check()


@pytest.mark.parametrize("dist", ["rand", "shifted"])
def test_v2p23_gradients_vs_f64(dist):
    """N = 2^18 points x 32 views: output, x_mod gradient and every parameter gradient (the BatchNorm-backward sums
    are the gamma / beta gradients) of GroupBimodalCSRPool with its scores on the fp32 chain, against float64 autograd
    of the oracle module on the device; gates raised at most to 4x the oracle's own fp32 error."""
    from deepviewagg_amd import fused_chain_f32
    n = 1 << 18
    V = n * FVIEWS
    m = _headline_module()
    ref = O.GroupBimodalCSRPool(in_map=8, in_mod=64, num_groups=4, use_num=True)
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    for mod in ref.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.momentum = 1.0
    ref.train()
    g = torch.Generator(device=DEV).manual_seed(29)
    x_map = _x_map(V, dist, 31)
    x_mod = torch.randn(V, 64, generator=g, device=DEV)
    w = torch.randn(n, 64, generator=g, device=DEV)
    csr = torch.arange(0, V + 1, FVIEWS, device=DEV)
    calls = []
    real = fused_chain_f32.chain_scores
    fused_chain_f32.chain_scores = lambda *a: (calls.append(1), real(*a))[1]
    try:
        xm = x_mod.clone().requires_grad_()
        out = m(None, xm, x_map, csr)
    finally:
        fused_chain_f32.chain_scores = real
    assert calls, "the fp32 chain did not run"
    names = [k for k, _ in m.named_parameters()]
    grads = torch.autograd.grad((out * w).sum(), [xm] + list(m.parameters()))
    res = {}
    torch.cuda.reset_peak_memory_stats()
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(ref).to(DEV).to(dt)
        xr = x_mod.to(dt).requires_grad_()
        o = r(None, xr, x_map.to(dt), csr)
        gr = torch.autograd.grad((o * w.to(dt)).sum(), [xr] + list(r.parameters()))
        res[dt] = (o.detach(), gr, {k: v for k, v in r.state_dict().items() if "running" in k})
        del r, xr, o, gr
    print(f"\nfloat64 + float32 oracle autograd at V = 2^23: max_memory_allocated "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    (o64, g64, run64), (o32, g32, run32) = res[torch.float64], res[torch.float32]
    case = f"V=2^23 x_map={dist}"
    rep = T.Report(case)
    rep.add(case, "out", "out", T.rel_err(out, o64), T.rel_err(o32, o64))
    rep.add(case, "grad_x_mod", "grad_in", T.rel_err(grads[0], g64[0]), T.rel_err(g32[0], g64[0]))
    gp64 = dict(zip(names, g64[1:]))
    for k, a, b, b32 in zip(names, grads[1:], g64[1:], g32[1:]):
        scale = T.param_scale(k, gp64)
        rep.add(case, k, "grad_param", T.rel_err(a, b, scale), T.rel_err(b32, b, scale))
    for k, v in m.state_dict().items():
        if "running_mean" in k:
            var_k = k.replace("running_mean", "running_var")
            nn_ = V if "mlp_set" not in k else n
            vv = m.state_dict()[var_k]
            em, ev = T.bn_errors(v, vv * (nn_ - 1) / nn_, run64[k], run64[var_k] * (nn_ - 1) / nn_)
            em32, ev32 = T.bn_errors(run32[k], run32[var_k] * (nn_ - 1) / nn_, run64[k], run64[var_k] * (nn_ - 1) / nn_)
            rep.add(case, k.replace(".running_mean", "") + " mean", "bn_mean", em, em32)
            rep.add(case, k.replace(".running_mean", "") + " var", "bn_var", ev, ev32)
    rep.check()
