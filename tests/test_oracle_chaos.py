"""CPU (-m "not gpu"): how reproducible is the bf16 arithmetic of the recompute chain ITSELF?

The tolerances of tests/test_gpu_chain.py::test_chain_matches_bf16_emulation for train-mode parameter gradients rest on
this measurement: the emulation oracle (oracle/chain_emulation.py) evaluated twice, the second time with x_map
perturbed by a relative 1e-6 (a few fp32 ulps: what a different summation order or a different exp / rsqrt does),
disagrees with itself by percents on the parameter gradients, while the output and the rows gradient move by ~1e-3.
bf16 roundings that flip (2^-8 per flipped activation / weight-operand entry), train-mode BatchNorm (batch statistics
and the folded operand bf16(0.6 G W) couple all views) and the BatchNorm backward (which removes most of dy) make the
parameter gradients of ANY bf16 evaluation -- these kernels, the reference under autocast -- a chaotic function of
the last bits of its inputs.  In eval mode (running statistics) the same perturbation stays below 1 %."""
import torch

from oracle import pooling_oracle as O
from oracle.chain_emulation import emulated_chain


def _case(seed, N, C, G, train):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(0, 9, (N,), generator=gen)
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    V = int(csr[-1])
    x_map = torch.rand(V, 8, generator=gen)
    w = torch.randn(N, C, generator=gen)
    rows = torch.randn(777, C, generator=gen).bfloat16()
    row_idx = torch.randint(0, 777, (V,), generator=gen)
    ref = O.GroupBimodalCSRPool(in_map=8, in_mod=C, num_groups=G, use_num=True)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
            if "batch_norm.weight" in n or n == "G.weight":
                p.add_(1.0)
        for n, b in ref.named_buffers():
            if "running_mean" in n:
                b.copy_(torch.randn(b.shape, generator=gen) * 0.1)
            if "running_var" in n:
                b.copy_(torch.rand(b.shape, generator=gen) + 0.5)
    ref.train(train)
    return ref, csr, x_map, w, rows, row_idx


def _grads(ref, sd, csr, x_map, w, rows, row_idx):
    ref.load_state_dict(sd)
    params = [p for n, p in ref.named_parameters() if not n.startswith("E_mod")]
    rr = rows.float().requires_grad_()
    out = emulated_chain(ref, rr[row_idx], x_map, csr)
    return out.detach(), torch.autograd.grad((out * w).sum(), [rr] + params, allow_unused=True)


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _self_deviation(train, eps):
    ref, csr, x_map, w, rows, row_idx = _case(13, 3000, 64, 4, train)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    noise = torch.randn(x_map.shape, generator=torch.Generator().manual_seed(1))
    o0, g0 = _grads(ref, sd, csr, x_map, w, rows, row_idx)
    o1, g1 = _grads(ref, sd, csr, x_map * (1 + eps * noise), w, rows, row_idx)
    par = sorted(_rel(a, b) for a, b in zip(g1[1:], g0[1:]) if a is not None)
    return _rel(o1, o0), _rel(g1[0], g0[0]), par[len(par) // 2], par[-1]


def test_train_mode_parameter_gradients_are_chaotic_in_the_last_bits_of_the_input():
    out, rows, med, worst = _self_deviation(train=True, eps=1e-6)
    print(f"train, 1e-6: out {out:.2e} rows {rows:.2e} parameters median {med:.2e} max {worst:.2e}")
    assert out < 5e-3 and rows < 5e-3                # the output and the rows gradient are well conditioned ...
    assert med > 5e-3 and worst > 2e-2               # ... the parameter gradients are not: percents from 1e-6
    out, rows, med, worst = _self_deviation(train=True, eps=1.5e-5)          # 2^-16: the kernels' first-layer input
    print(f"train, 1.5e-5: out {out:.2e} rows {rows:.2e} parameters median {med:.2e} max {worst:.2e}")
    assert med > 2e-2 and worst < 3e-1


def test_eval_mode_parameter_gradients_are_well_conditioned():
    out, rows, med, worst = _self_deviation(train=False, eps=1e-6)
    print(f"eval, 1e-6: out {out:.2e} rows {rows:.2e} parameters median {med:.2e} max {worst:.2e}")
    assert out < 5e-3 and rows < 5e-3 and worst < 3e-2


def test_float32_emulation_is_unchanged_by_the_dtype_preserving_form(monkeypatch):
    """oracle/chain_emulation.py keeps the dtype of its input (``.to(t.dtype)`` where it said ``.float()``) so that a
    float64 twin can be evaluated (tests/rowwise.py).  What is checked here: with the rounding helper ``_bf`` -- the edit
    that every layer passes -- put back to its ``.float()`` form the float32 output is bit-equal and float32 throughout.
    (The x16 lines, set_num and the dev_invstd branch are identities on float32 by reading; they are not put back here.)
    Bit-equal output (the gradients are compared
    to 1e-5: the CPU's index_add of the backward is not run-to-run deterministic, ~5e-7 of the same code twice)."""
    import oracle.chain_emulation as CE
    ref, csr, x_map, w, rows, row_idx = _case(13, 1500, 64, 4, True)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    o_new, g_new = _grads(ref, sd, csr, x_map, w, rows, row_idx)
    monkeypatch.setattr(CE, "_bf", lambda t: t + (t.bfloat16().float() - t).detach())
    o_old, g_old = _grads(ref, sd, csr, x_map, w, rows, row_idx)
    assert o_new.dtype == torch.float32 and torch.equal(o_new, o_old)
    for a, b in zip(g_new, g_old):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.dtype == torch.float32 and _rel(a, b) < 1e-5
