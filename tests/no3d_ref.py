"""Plain-torch CPU restatements for the tail of the image-only models (reference
models/segmentation/multimodal/no3d.py:102-154): the brute-force nearest seen point, the materialised view-level loss
and the tail itself.  Test infrastructure: nothing here is imported by the package."""
import torch

IGNORE_LABEL = -1       # torch_points3d.datasets.segmentation.IGNORE_LABEL


def sq_dist(q, s):
    """[Q, S] squared distances ((dx*dx + dy*dy) + dz*dz) in the dtype of the inputs; torch rounds every elementwise
    operation on its own, so in float32 this is the expression of include/dva.h."""
    dx = q[:, None, 0] - s[None, :, 0]
    dy = q[:, None, 1] - s[None, :, 1]
    dz = q[:, None, 2] - s[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest_seen_ref(pos, seen, dtype=torch.float32, chunk=512, with_margin=False):
    """``src`` int64 [N]: i for a seen point, else the original index of the seen point at the smallest squared distance
    evaluated in ``dtype``, ties to the lowest index; i everywhere when no point is seen (no3d.py:106, :119-125).
    ``with_margin``: also (d2 of the nearest, d2 of the second nearest seen point) per point, inf where there is none."""
    pos = pos.detach().cpu().to(dtype)
    seen = seen.detach().cpu().bool()
    n = pos.shape[0]
    src = torch.arange(n)
    d1 = torch.full((n,), float("inf"), dtype=dtype)
    d2 = torch.full((n,), float("inf"), dtype=dtype)
    s_idx = torch.nonzero(seen).flatten()
    q_idx = torch.nonzero(~seen).flatten()
    if s_idx.numel() and q_idx.numel():
        s = pos[s_idx]
        for a in range(0, q_idx.numel(), chunk):
            qi = q_idx[a:a + chunk]
            d = sq_dist(pos[qi], s)
            best = d.min(1).values
            big = torch.iinfo(torch.int64).max
            first = torch.where(d == best[:, None], s_idx[None, :], torch.full((1, 1), big)).min(1).values
            src[qi] = first
            if with_margin:
                d1[qi] = best
                if s_idx.numel() > 1:
                    d2[qi] = d.topk(2, dim=1, largest=False).values[:, 1]
    return (src, d1, d2) if with_margin else src


def in_margin(d1, d2, rel=1e-4):
    """Queries whose nearest and second-nearest float64 squared distances differ by at most ``rel`` relative: there the
    float32 and the float64 argmin may name different points.  A query with a single candidate (d2 = inf) is not."""
    return torch.isfinite(d2) & ((d2 - d1) <= rel * d2)


def view_nll_ref(x_view, labels, csr_idx, weight=None, ignore_index=IGNORE_LABEL, dtype=torch.float64):
    """The materialised view loss (no3d.py:150-154) written out: per view the log-softmax of its row, scored against the
    label of the point that owns the view; ``sum w[y] (-logp[y]) / sum w[y]`` over the views whose label is neither
    ``ignore_index`` nor outside [0, K)."""
    x = x_view.detach().cpu().to(dtype)
    labels, csr_idx = labels.detach().cpu().long(), csr_idx.detach().cpu().long()
    K = x.shape[1]
    target = torch.repeat_interleave(labels, csr_idx[1:] - csr_idx[:-1])            # :151-152
    m = x.max(1, keepdim=True).values if x.shape[0] else x[:, :1]
    logp = (x - m) - (x - m).exp().sum(1, keepdim=True).log()                        # :150
    counted = (target != ignore_index) & (target >= 0) & (target < K)
    t = target.clamp(0, K - 1)
    w = torch.ones(K, dtype=dtype) if weight is None else weight.detach().cpu().to(dtype)
    wv = torch.where(counted, w[t], torch.zeros((), dtype=dtype))
    picked = logp.gather(1, t[:, None])[:, 0]
    return (wv * -torch.where(counted, picked, torch.zeros((), dtype=dtype))).sum() / wv.sum()      # :154


def no3d_tail_ref(features, seen, pos, labels=None, head=None, training=False, view=None, weight=None,
                  ignore_label=IGNORE_LABEL, log_softmax=None, dtype=torch.float32):
    """The tail of ``No3D.forward`` on CPU tensors: ``(output, loss, labels after masking)``.  ``view`` is the
    materialised ``(last_view_x_mod [V, C], csr_idx)``; ``log_softmax`` replaces ``torch.log_softmax(., -1)`` (the GPU
    test passes the device's, to hold the row copies bit for bit); the losses are evaluated in ``dtype``."""
    log_softmax = log_softmax or (lambda z: torch.log_softmax(z, -1))
    logits = head(features) if head is not None else features                        # no3d.py:102
    output = log_softmax(logits).clone()                                             # :103
    n = output.shape[0]
    if seen is None:                                                                 # :83-84
        seen = torch.zeros(n, dtype=torch.bool)
    seen = seen.bool()
    if labels is not None:
        labels = labels.clone()               # the reference writes into self.labels; the caller's tensor stays here
    if not training:                                                                 # :105
        if bool(seen.any()):                                                         # :106
            src = nearest_seen_ref(pos, seen)                                        # :119-122, brute force for KeOps
            output[~seen] = output[src[~seen]]                                       # :125
        elif labels is not None:
            labels[~seen] = ignore_label                                             # :129
    elif labels is not None:
        labels[~seen] = ignore_label                                                 # :134
    if labels is None:                                                               # :137
        return output, None, None
    if view is None:                                                                 # :140-142
        t = labels.long()
        K = output.shape[1]
        counted = (t != ignore_label) & (t >= 0) & (t < K)
        w = torch.ones(K, dtype=dtype) if weight is None else weight.to(dtype)
        wv = torch.where(counted, w[t.clamp(0, K - 1)], torch.zeros((), dtype=dtype))
        picked = output.to(dtype).gather(1, t.clamp(0, K - 1)[:, None])[:, 0]
        loss = (wv * -torch.where(counted, picked, torch.zeros((), dtype=dtype))).sum() / wv.sum()   # :154
    else:                                                                            # :145-152
        view_features, csr_idx = view
        view_logits = head(view_features) if head is not None else view_features     # :148-149
        loss = view_nll_ref(view_logits, labels, csr_idx, weight, ignore_label, dtype)
    return output, loss, labels


# ---------------------------------------------------------------------------------------------
# the clouds and masks of the nearest-seen tests (tests/test_no3d_host.py, tests/test_gpu_no3d.py)
# ---------------------------------------------------------------------------------------------
BOX = (4.0, 4.0, 2.5)
UNIFORM_SIZES = (1, 63, 64, 65, 3000, 4097)
UNIFORM_LAYOUTS = ("f0.5", "f0.3", "f0.02", "one", "all", "none", "corner")


def uniform_cloud(n, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    return torch.rand(n, 3, generator=gen) * torch.tensor(BOX)


def seen_layout(kind, pos, seed=0):
    n = pos.shape[0]
    gen = torch.Generator().manual_seed(2000 + seed)
    if kind.startswith("f"):
        return torch.rand(n, generator=gen) < float(kind[1:])
    if kind == "one":
        seen = torch.zeros(n, dtype=torch.bool)
        seen[n // 3] = True
        return seen
    if kind == "all":
        return torch.ones(n, dtype=torch.bool)
    if kind == "none":
        return torch.zeros(n, dtype=torch.bool)
    if kind == "corner":                      # seen points confined to x < 0.5: most queries need the coarse levels
        return pos[:, 0] < 0.5
    raise ValueError(kind)


def uniform_cases():
    """(name, pos, seen) over the sizes and layouts above."""
    for n in UNIFORM_SIZES:
        pos = uniform_cloud(n, seed=n)
        for kind in UNIFORM_LAYOUTS:
            yield f"uniform{n}-{kind}", pos, seen_layout(kind, pos, seed=n)


def special_cases():
    """(name, pos, seen): tied, duplicated, planar and far-apart clouds."""
    c = torch.arange(14, dtype=torch.float32)
    grid = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    voxel = (grid + 0.5) * 0.05                                    # voxel centres: most queries are tied in float64
    yield "voxel14-f0.3", voxel, seen_layout("f0.3", voxel, seed=1)
    yield "voxel14-f0.02", voxel, seen_layout("f0.02", voxel, seed=2)
    base = uniform_cloud(500, seed=3)
    gen = torch.Generator().manual_seed(4)
    dup = base[torch.randint(0, 500, (1700,), generator=gen)]      # distance 0 to several seen points
    yield "duplicates-f0.5", dup, seen_layout("f0.5", dup, seed=5)
    planar = uniform_cloud(2100, seed=6)
    planar[:, 2] = 1.25
    yield "planar-f0.3", planar, seen_layout("f0.3", planar, seed=7)
    far = uniform_cloud(2500, seed=8)
    far[1250:, 0] += 1000.0                                        # two clusters 1000 units apart
    yield "clusters-f0.3", far, seen_layout("f0.3", far, seed=9)
    only_a = seen_layout("f0.3", far, seed=10)
    only_a[1250:] = False                                          # every query of the second cluster crosses the gap
    yield "clusters-one-side", far, only_a


def view_case(K, seed=0, n=257, rows=4 * 16 * 32):
    """The small view-loss case: ``n`` points with 0 to 5 views each, one with 70, several with none; ``rows`` map rows
    of which most have no view; labels in [0, K) with some ignored and one out of range.  Returns a dict of CPU
    tensors: rows fp32 [R, K], row_idx int32 [V], csr_idx int64 [n + 1], labels int64 [n], weight fp32 [K]."""
    gen = torch.Generator().manual_seed(3000 + seed)
    sizes = torch.randint(0, 6, (n,), generator=gen)
    sizes[7] = 70
    sizes[[0, 11, 12, n - 1]] = 0
    csr_idx = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    V = int(csr_idx[-1])
    labels = torch.randint(0, K, (n,), generator=gen)
    labels[torch.rand(n, generator=gen) < 0.2] = IGNORE_LABEL
    labels[5] = K + 3                                              # out of range: takes no part
    labels[7] = K - 1
    return dict(rows=torch.randn(rows, K, generator=gen) * 3.0,
                row_idx=torch.randint(0, rows, (V,), generator=gen).int(), csr_idx=csr_idx, labels=labels,
                weight=torch.rand(K, generator=gen) + 0.5)
