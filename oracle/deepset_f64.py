"""ORACLE (test infrastructure, NOT product code): train-mode DeepSetFeat + score layer in float64, restated in
plain torch over point-aligned chunks of the views, for scenes too large for one autograd evaluation.

Restates pooling.py:604-673 (DeepSetFeat with pool='max', fusion='concatenation', optional use_num) followed by the
score Linear (pooling.py:258,282), with the MLP blocks of core/common_modules/base_modules.py:38-48 (Linear without
bias -> FastBatchNorm1d -> LeakyReLU(0.2)) in train mode: every BatchNorm normalises with the batch mean and the
biased batch variance of its whole input.  One BatchNorm layer is resolved per pass over the chunks, each pass
re-deriving the layer inputs from x_map with the float64 statistics of the layers before it:

  pass 1  elt_1.0   z1 = x W1^T                             -> mean / var of z1
  pass 2  elt_1.1   z2 = a1 W2^T                            -> mean / var of z2
  pass 3            a2 = act(BN2(z2)), max over each point  -> x_set [N, 32 (+1)]
          set.0, set.1 over the N points (one dense evaluation)
  pass 4  elt_2.0   z5 = [a2 | set[point]] W5^T             -> mean / var of z5
  pass 5  elt_2.1   z6 = a5 W6^T                            -> mean / var of z6
  then    scores of the first ``slice_points`` points: act(BN6(z6)) Ws^T + bs

The per-chunk statistics are combined as (count, mean, M2) (Chan et al.), so the variance does not lose digits to
E[z^2] - E[z]^2 when the mean is large against the spread.  Works on any device; the module is only read.
"""
import torch

SLOPE = 0.2
LAYERS = ("mlp_elt_1.0", "mlp_elt_1.1", "mlp_set.0", "mlp_set.1", "mlp_elt_2.0", "mlp_elt_2.1")


class _Moments:
    """Running (n, mean, M2) per channel, float64, Chan's parallel combination."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0, None, None

    def add(self, z):
        nb = z.shape[0]
        if nb == 0:
            return
        mb = z.mean(0)
        m2b = ((z - mb) ** 2).sum(0)
        if self.n == 0:
            self.n, self.mean, self.m2 = nb, mb, m2b
            return
        n = self.n + nb
        d = mb - self.mean
        self.mean = self.mean + d * (nb / n)
        self.m2 = self.m2 + m2b + d * d * (self.n * nb / n)
        self.n = n

    def result(self):
        return self.mean, self.m2 / self.n            # biased variance: what BatchNorm normalises with


def _block(mlp, i, dt):
    lin, bn = mlp[i][0], mlp[i][1].batch_norm
    return lin.weight.detach().to(dt), bn.weight.detach().to(dt), bn.bias.detach().to(dt), bn.eps


def _act(z, stats, block):
    mean, var = stats
    _, gamma, beta, eps = block
    y = (z - mean) * torch.rsqrt(var + eps) * gamma + beta
    return torch.where(y > 0, y, SLOPE * y)


def _set_num(csr):
    # pooling.py:664-666 (the reference evaluates 1 / (n + 1e-3) in the default float32, then casts)
    return torch.sqrt(1 / (csr[1:] - csr[:-1] + 1e-3)).view(-1, 1)


def deepset_scores_f64(e_map, e_score, x_map, csr, chunk_points=1 << 17, slice_points=1 << 16, dtype=torch.float64):
    """Train-mode ``e_score(e_map(x_map, csr))`` in float64.  Returns ``(stats, scores)``: ``stats[layer] = (mean,
    biased var, count)`` for the six BatchNorm layers of ``LAYERS``, ``scores`` [V_slice, G] for the first
    ``slice_points`` points.  ``dtype=torch.float32``: the same evaluation in plain fp32 (a yardstick)."""
    dev = x_map.device
    N = csr.shape[0] - 1
    csr = csr.to(dev)
    bounds = list(range(0, N, chunk_points)) + [N]
    chunks = list(zip(bounds[:-1], bounds[1:]))
    B1, B2 = _block(e_map.mlp_elt_1, 0, dtype), _block(e_map.mlp_elt_1, 1, dtype)
    S1, S2 = _block(e_map.mlp_set, 0, dtype), _block(e_map.mlp_set, 1, dtype)
    B5, B6 = _block(e_map.mlp_elt_2, 0, dtype), _block(e_map.mlp_elt_2, 1, dtype)
    stats = {}

    def views(p0, p1):
        v0, v1 = int(csr[p0]), int(csr[p1])
        sizes = csr[p0 + 1:p1 + 1] - csr[p0:p1]
        local = torch.arange(p1 - p0, device=dev).repeat_interleave(sizes)
        return x_map[v0:v1].to(dtype), local, sizes

    def a1_of(x):
        return _act(x @ B1[0].T, stats["mlp_elt_1.0"][:2], B1)

    def a2_of(x):
        return _act(a1_of(x) @ B2[0].T, stats["mlp_elt_1.1"][:2], B2)

    def one_pass(name, fn):
        mom = _Moments()
        for p0, p1 in chunks:
            mom.add(fn(p0, p1))
        stats[name] = mom.result() + (mom.n,)

    one_pass("mlp_elt_1.0", lambda p0, p1: views(p0, p1)[0] @ B1[0].T)
    one_pass("mlp_elt_1.1", lambda p0, p1: a1_of(views(p0, p1)[0]) @ B2[0].T)
    # per-point max of a2 (empty points: 0, pooling.py:870 / torch_scatter)
    pooled = torch.zeros((N, B2[0].shape[0]), dtype=dtype, device=dev)
    for p0, p1 in chunks:
        x, local, _ = views(p0, p1)
        a2 = a2_of(x)
        part = torch.full((p1 - p0, a2.shape[1]), float("-inf"), dtype=dtype, device=dev)
        part.scatter_reduce_(0, local.view(-1, 1).expand_as(a2), a2, "amax", include_self=True)
        pooled[p0:p1] = torch.where(torch.isinf(part), torch.zeros_like(part), part)
    x_set = torch.cat([pooled, _set_num(csr).to(dtype)], 1) if e_map.use_num else pooled
    z = x_set @ S1[0].T
    stats["mlp_set.0"] = (z.mean(0), z.var(0, unbiased=False), N)
    a = _act(z, stats["mlp_set.0"][:2], S1)
    z = a @ S2[0].T
    stats["mlp_set.1"] = (z.mean(0), z.var(0, unbiased=False), N)
    y_set = _act(z, stats["mlp_set.1"][:2], S2)
    del pooled, x_set, z, a

    def z5_of(p0, p1):
        x, local, _ = views(p0, p1)
        return torch.cat([a2_of(x), y_set[p0:p1][local]], 1) @ B5[0].T

    def z6_of(p0, p1):
        return _act(z5_of(p0, p1), stats["mlp_elt_2.0"][:2], B5) @ B6[0].T

    one_pass("mlp_elt_2.0", z5_of)
    one_pass("mlp_elt_2.1", z6_of)
    n_s = min(slice_points, N)
    a6 = _act(z6_of(0, n_s), stats["mlp_elt_2.1"][:2], B6)
    scores = a6 @ e_score.weight.detach().to(dtype).T + e_score.bias.detach().to(dtype)
    return stats, scores
