"""CPU: the chunked float64 restatement of DeepSetFeat + score layer (oracle/deepset_f64.py) against the oracle module
evaluated in float64 train mode in one piece, on a small ragged scene (empty points, chunks that split nowhere
special): BatchNorm batch statistics of all six layers and the scores of a slice, to 1e-12."""
import pytest
import torch

from oracle import pooling_oracle as O
from oracle.deepset_f64 import LAYERS, deepset_scores_f64


@pytest.mark.parametrize("use_num", [True, False])
@pytest.mark.parametrize("shift", [0.0, 1.0])
def test_chunked_restatement_equals_oracle_module(use_num, shift):
    gen = torch.Generator().manual_seed(3 + use_num)
    N = 700
    sizes = torch.randint(0, 9, (N,), generator=gen)
    sizes[:5] = 0
    sizes[100] = 70
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    V = int(csr[-1])
    x_map = shift + (0.03 if shift else 1.0) * torch.rand(V, 8, generator=gen, dtype=torch.float64)
    e_map = O.DeepSetFeat(8, 32, use_num=use_num)
    lin = torch.nn.Linear(32, 4)
    with torch.no_grad():
        for p in list(e_map.parameters()) + list(lin.parameters()):
            p.copy_(torch.randn(p.shape, generator=gen) * 0.4)
    e_map, lin = e_map.double().train(), lin.double()
    for mod in e_map.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.momentum = 1.0               # running statistics := this batch's (mean, unbiased variance)
    stats, scores = deepset_scores_f64(e_map, lin, x_map, csr, chunk_points=97, slice_points=250)
    with torch.no_grad():
        ref = lin(e_map(x_map, csr))
    n_s = int(csr[250])
    assert scores.shape == (n_s, 4)
    torch.testing.assert_close(scores, ref[:n_s], rtol=1e-12, atol=1e-12 * float(ref.abs().max()))
    for name in LAYERS:
        mlp, i = name.split(".")
        bn = getattr(e_map, mlp)[int(i)][1].batch_norm
        mean, var, n = stats[name]
        assert n == (N if mlp == "mlp_set" else V)
        torch.testing.assert_close(mean, bn.running_mean, rtol=1e-12, atol=1e-12 * float(var.max()) ** 0.5)
        torch.testing.assert_close(var * n / (n - 1), bn.running_var, rtol=1e-12, atol=0)
