"""CPU ORACLE (test infrastructure, NOT product code) for the gather + view-pooling half of the
DeepViewAgg hot path.

Plain-PyTorch (CPU, fp32/fp64) restatement of the reference's algorithm, each function citing the
reference file:line it follows (paths relative to /root/reference).  Only ``tests/``,
``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import this module; the
package ``deepviewagg_amd`` never does.

Pinned against the reference itself: ``oracle/gen_golden.py`` imports the reference's Python source
in the build container and stores its inputs/outputs/gradients under ``tests/golden/``;
``tests/test_oracle_golden.py`` checks this restatement against those vectors (and against the
docstring known answers of pooling.py:913-921).

Third-party arithmetic the reference leans on and that is absent from /root/reference:
``torch_scatter`` (version unpinned by install.sh:125).  Restated semantics: deterministic CSR
reductions, empty groups -> 0 (pooling.py:870), max/min gradient routed to the first extremal row.
"""
import math

import torch
import torch.nn as nn


# ----------------------------------------------------------------------------------------------
# torch_scatter.segment_csr / gather_csr / softmax
# ----------------------------------------------------------------------------------------------

def dense_index(csr_idx):
    """pooling.py:779-782: group id of every element."""
    sizes = csr_idx[1:] - csr_idx[:-1]
    return torch.arange(csr_idx.shape[0] - 1, device=csr_idx.device).repeat_interleave(sizes)


def segment_arg(src, csr_idx, reduce):
    """Row index of the per-group max/min (first row on ties, -1 for empty groups)."""
    src2 = src.detach().reshape(src.shape[0], -1)
    n, C = csr_idx.shape[0] - 1, src2.shape[1]
    arg = torch.full((n, C), -1, dtype=torch.long)
    for g in range(n):  # small sizes only: this is the readable definition
        b, e = int(csr_idx[g]), int(csr_idx[g + 1])
        if e > b:
            seg = src2[b:e]
            # torch's argmax/argmin return the FIRST extremal index on CPU
            arg[g] = (seg.argmax(0) if reduce == 'max' else seg.argmin(0)) + b
    return arg.reshape((n,) + tuple(src.shape[1:]))


def segment_arg_fast(src, csr_idx, reduce):
    """Vectorised equivalent of segment_arg (used at sizes where the loop is too slow)."""
    src2 = src.detach().reshape(src.shape[0], -1)
    n, C = csr_idx.shape[0] - 1, src2.shape[1]
    M = src2.shape[0]
    idx = dense_index(csr_idx).view(-1, 1).expand(M, C)
    init = float('-inf') if reduce == 'max' else float('inf')
    ext = torch.full((n, C), init, dtype=src2.dtype, device=src2.device).scatter_reduce(
        0, idx, src2, 'amax' if reduce == 'max' else 'amin', include_self=True)
    rows = torch.arange(M, device=src2.device).view(-1, 1).expand(M, C)
    cand = torch.where(src2 == ext.gather(0, idx), rows, torch.full_like(rows, M))
    arg = torch.full((n, C), M, dtype=torch.long, device=src2.device).scatter_reduce(0, idx, cand, 'amin',
                                                                                     include_self=True)
    arg = torch.where(arg == M, torch.full_like(arg, -1), arg)
    return arg.reshape((n,) + tuple(src.shape[1:]))


def segment_csr(src, csr_idx, reduce='sum'):
    """torch_scatter.segment_csr along dim 0 (call sites pooling.py:63,289,295,628,787,807)."""
    n = csr_idx.shape[0] - 1
    sizes = csr_idx[1:] - csr_idx[:-1]
    tail = tuple(src.shape[1:])
    if reduce in ('sum', 'add', 'mean'):
        out = torch.zeros((n,) + tail, dtype=src.dtype, device=src.device).index_add(0, dense_index(csr_idx), src)
        if reduce == 'mean':
            out = out / sizes.clamp(min=1).to(src.dtype).view((-1,) + (1,) * len(tail))
        return out
    if reduce in ('max', 'min'):
        arg = segment_arg_fast(src, csr_idx, reduce)
        src0 = torch.cat([src, torch.zeros((1,) + tail, dtype=src.dtype, device=src.device)])  # row M == zeros
        arg0 = torch.where(arg < 0, torch.full_like(arg, src.shape[0]), arg)
        return src0.gather(0, arg0) if src.dim() > 1 else src0[arg0]
    raise ValueError(reduce)


def gather_csr(src, csr_idx):
    """pooling.py:813-841."""
    return src[dense_index(csr_idx)]


def segment_gather_csr(src, csr_idx, reduce='sum'):
    """pooling.py:844-856."""
    return gather_csr(segment_csr(src, csr_idx, reduce), csr_idx)


def segment_softmax_csr(src, csr_idx, eps=1e-12, scaling=False):
    """pooling.py:758-810: centre on the group max, optionally divide by sqrt(group size) AFTER
    centring (:792-801), exp, divide by (group sum + eps)."""
    idx = dense_index(csr_idx)
    centered = src - segment_csr(src, csr_idx, 'max')[idx]
    if scaling:
        num = (csr_idx[1:] - csr_idx[:-1]).float().sqrt()[idx]
        centered = centered / (num.view(-1, 1) if src.dim() > 1 else num)
    e = centered.exp()
    return e / (segment_csr(e, csr_idx, 'sum') + eps)[idx]


def group_sizes(num_elements, num_groups):
    """pooling.py:737-745."""
    sizes = torch.full((num_groups,), math.floor(num_elements / num_groups), dtype=torch.long)
    sizes += torch.arange(num_groups) < num_elements - sizes.sum()
    return sizes


def expand_group_feat(A, num_groups, num_channels):
    """pooling.py:748-755."""
    if num_groups == 1:
        return A.view(-1, 1)
    if num_groups < num_channels:
        return A.repeat_interleave(group_sizes(num_channels, num_groups).to(A.device), dim=1)
    return A


def nearest_power_of_2(x, min_power=16):
    """pooling.py:718-734."""
    x = int(x)
    if x < min_power:
        return min_power
    previous_power = 2 ** ((x - 1).bit_length() - 1)
    next_power = 2 ** (x - 1).bit_length()
    return previous_power if x - previous_power < next_power - x else next_power


# ----------------------------------------------------------------------------------------------
# modules (parameter names identical to the reference so state dicts are interchangeable)
# ----------------------------------------------------------------------------------------------

class FastBatchNorm1d(nn.Module):
    """core/common_modules/base_modules.py:131-156 (2D input: BN over rows)."""

    def __init__(self, num_features, momentum=0.1):
        super().__init__()
        self.batch_norm = nn.BatchNorm1d(num_features, momentum=momentum)

    def forward(self, x):
        return self.batch_norm(x.unsqueeze(2).transpose(0, 2)).transpose(0, 2).squeeze(2)


def MLP(channels, bias=True):
    """core/common_modules/base_modules.py:38-48."""
    return nn.Sequential(*[
        nn.Sequential(nn.Linear(channels[i - 1], channels[i], bias=bias),
                      FastBatchNorm1d(channels[i]), nn.LeakyReLU(0.2))
        for i in range(1, len(channels))])


class Gating(nn.Module):
    """pooling.py:690-715 (out-of-place)."""

    def __init__(self, num_groups):
        super().__init__()
        self.num_groups = num_groups
        self.weight = nn.Parameter(torch.ones(1, num_groups))
        self.bias = nn.Parameter(torch.zeros(1, num_groups))

    def forward(self, x):
        return torch.tanh(torch.relu(x * self.weight + self.bias)).view(-1, self.num_groups).squeeze(1)


class DeepSetFeat(nn.Module):
    """pooling.py:604-673."""

    def __init__(self, d_in, d_out, pool='max', fusion='concatenation', use_num=False, **kw):
        super().__init__()
        self.pool = pool.split('_')
        self.fusion = fusion
        self.use_num = use_num
        self.mlp_elt_1 = MLP([d_in, d_out, d_out], bias=False)
        self.mlp_set = MLP([d_out * len(self.pool) + use_num, d_out, d_out], bias=False)
        self.mlp_elt_2 = MLP([d_out if fusion == 'residual' else 2 * d_out, d_out, d_out], bias=False)

    def forward(self, x, csr_idx):
        x = self.mlp_elt_1(x)
        x_set = torch.cat([segment_csr(x, csr_idx, p) for p in self.pool], dim=-1)
        if self.use_num:
            set_num = torch.sqrt(1 / (csr_idx[1:] - csr_idx[:-1] + 1e-3))
            x_set = torch.cat((x_set, set_num.view(-1, 1).to(x_set.dtype)), dim=1)
        x_set = gather_csr(self.mlp_set(x_set), csr_idx)
        if self.fusion == 'residual':
            x_out = x + x_set
        elif self.fusion == 'concatenation':
            x_out = torch.cat((x, x_set), dim=-1)
        else:
            x_out = torch.cat((x, x + x_set), dim=-1)
        return self.mlp_elt_2(x_out)


class MinMaxDiffSetFeat(nn.Module):
    """pooling.py:554-601."""

    def __init__(self, d_in, d_out, use_min=True, use_max=True, use_num=False, **kw):
        super().__init__()
        self.use_min, self.use_max, self.use_num = use_min, use_max, use_num
        self.mlp = MLP([d_in * (1 + use_min + use_max) + use_num, d_out, d_out], bias=False)

    def forward(self, x, csr_idx):
        feats = [x]
        if self.use_min:
            feats.append(x - segment_gather_csr(x, csr_idx, 'min'))
        if self.use_max:
            feats.append(x - segment_gather_csr(x, csr_idx, 'max'))
        if self.use_num:
            sizes = csr_idx[1:] - csr_idx[:-1]
            feats.append(torch.sqrt(1 / (sizes + 1e-3)).repeat_interleave(sizes).view(-1, 1).to(x.dtype))
        return self.mlp(torch.cat(feats, dim=1))


class MLPSetFeat(nn.Module):
    """pooling.py:676-687."""

    def __init__(self, d_in, d_out, **kw):
        super().__init__()
        self.mlp = MLP([d_in, d_out, d_out], bias=False)

    def forward(self, x, csr_idx):
        return self.mlp(x)


_ENCODERS = {'DeepSetFeat': DeepSetFeat, 'MinMaxDiffSetFeat': MinMaxDiffSetFeat, 'MLPSetFeat': MLPSetFeat}


def attention_tail(x_mod, compat, csr_idx, G_module, num_groups, out_mod, group_scaling):
    """pooling.py:284-300 (== :514-530)."""
    att = segment_softmax_csr(compat, csr_idx, scaling=group_scaling)
    x_pool = segment_csr(x_mod * expand_group_feat(att, num_groups, out_mod), csr_idx, 'sum')
    gating = None
    if G_module is not None:
        gating = G_module(segment_csr(compat, csr_idx, 'max'))
        x_pool = x_pool * expand_group_feat(gating, num_groups, out_mod)
    return x_pool, att, gating


class GroupBimodalCSRPool(nn.Module):
    """pooling.py:159-319."""

    def __init__(self, in_map=None, in_mod=None, out_mod=None, num_groups=1, use_mod=False,
                 gating=True, group_scaling=True, nc_inner=32, map_encoder='DeepSetFeat', **kw):
        super().__init__()
        out_mod = in_mod if out_mod is None else out_mod
        self.out_mod, self.use_mod, self.num_groups = out_mod, use_mod, num_groups
        self.group_scaling = group_scaling
        self.E_map = _ENCODERS[map_encoder](in_map, nc_inner, **kw)
        self.E_mod = MLP([in_mod, out_mod, out_mod], bias=False)
        if use_mod:
            in_mix = nc_inner + out_mod
            mid = nearest_power_of_2((in_mix + nc_inner) / 2, nc_inner * 2)
            self.E_mix = MLP([in_mix, mid, nc_inner], bias=False)
        self.E_score = nn.Linear(nc_inner, num_groups, bias=True)
        self.G = Gating(num_groups) if gating else None

    def forward(self, x_main, x_mod, x_map, csr_idx):
        x_map = self.E_map(x_map, csr_idx)
        x_mod = self.E_mod(x_mod)
        compat = self.E_score(self.E_mix(torch.cat([x_map, x_mod], dim=1)) if self.use_mod else x_map)
        x_pool, self.last_A, self.last_G = attention_tail(
            x_mod, compat, csr_idx, self.G, self.num_groups, self.out_mod, self.group_scaling)
        self.last_C = compat
        return x_pool


class QKVBimodalCSRPool(nn.Module):
    """pooling.py:322-551 (debug mode omitted: it draws random numbers)."""

    def __init__(self, in_main=None, in_map=None, in_mod=None, out_mod=None, num_groups=1,
                 use_mod_q=False, use_mod_k=False, nc_qk=8, gating=True, dim_scaling=True,
                 group_scaling=False, nc_inner=32, map_encoder='DeepSetFeat', **kw):
        super().__init__()
        out_mod = in_mod if out_mod is None else out_mod
        self.out_mod, self.nc_qk, self.num_groups = out_mod, nc_qk, num_groups
        self.use_mod_q, self.use_mod_k = use_mod_q, use_mod_k
        self.dim_scaling, self.group_scaling = dim_scaling, group_scaling
        self.E_main = MLP([in_main, nc_inner, nc_inner], bias=False)
        self.E_map = _ENCODERS[map_encoder](in_map, nc_inner, **kw)
        self.E_mod = MLP([in_mod, out_mod, out_mod], bias=False)
        if use_mod_q:
            in_mix = nc_inner + out_mod
            self.E_mix_Q = MLP([in_mix, nearest_power_of_2((in_mix + nc_inner) / 2, nc_inner * 2),
                                nc_inner], bias=False)
        self.Q = nn.Linear(nc_inner, nc_qk * num_groups, bias=True)
        if use_mod_k:
            in_mix = nc_inner + in_mod
            self.E_mix_K = MLP([in_mix, nearest_power_of_2((in_mix + nc_inner) / 2, nc_inner * 2),
                                nc_inner], bias=False)
        self.K = nn.Linear(nc_inner, nc_qk * num_groups, bias=True)
        self.G = Gating(num_groups) if gating else None

    def forward(self, x_main, x_mod, x_map, csr_idx):
        sizes = csr_idx[1:] - csr_idx[:-1]
        x_main = self.E_main(x_main)
        x_map = self.E_map(x_map, csr_idx)
        x_mod = self.E_mod(x_mod)
        keys = self.K(self.E_mix_K(torch.cat([x_map, x_mod], dim=1)) if self.use_mod_k else x_map)
        if self.use_mod_q:
            x_main_q = torch.repeat_interleave(x_main, sizes, dim=0)
            queries = self.Q(self.E_mix_Q(torch.cat([x_main_q, x_mod], dim=1)))
        else:
            queries = torch.repeat_interleave(self.Q(x_main), sizes, dim=0)
        compat = (keys.reshape(keys.shape[0], self.num_groups, self.nc_qk)
                  * queries.reshape(queries.shape[0], self.num_groups, self.nc_qk)).sum(dim=2)
        if self.dim_scaling:
            compat = compat / math.sqrt(self.nc_qk)
        x_pool, self.last_A, self.last_G = attention_tail(
            x_mod, compat, csr_idx, self.G, self.num_groups, self.out_mod, self.group_scaling)
        self.last_C = compat
        return x_pool


def bimodal_csr_pool(x_mod, csr_idx, mode='max'):
    """pooling.py:53-71."""
    return segment_csr(x_mod, csr_idx, mode)


def heuristic_csr_pool(x_mod, x_map, csr_idx, mode='max', feat=0):
    """pooling.py:129-152: pick the row with extremal mapping feature; unseen -> zeros."""
    arg = segment_arg_fast(x_map[:, feat], csr_idx, mode)
    arg = torch.where(arg < 0, torch.full_like(arg, x_mod.shape[0]), arg)
    return torch.cat((x_mod, torch.zeros_like(x_mod[[0]])))[arg]


def bimodal_fusion(x_main, x_mod, mode='residual'):
    """fusion.py:38-50."""
    if x_main is None:
        return x_mod
    if x_mod is None:
        return x_main
    return {'residual': lambda a, b: a + b, 'concatenation': lambda a, b: torch.cat((a, b), -1),
            'both': lambda a, b: torch.cat((a, a + b), -1), 'modality': lambda a, b: b}[mode](x_main, x_mod)


# ----------------------------------------------------------------------------------------------
# gather (core/multimodal/image.py)
# ----------------------------------------------------------------------------------------------

def floor_div_pixels(pixels, ratio):
    """image.py:1953-1954: (pix // ratio).long() with a float ratio."""
    if ratio == 1:
        return pixels.long()
    return (pixels // float(ratio)).long()


def gather_nearest(x, images_per_atom, pixels, ratio=1.0):
    """image.py:1262-1287 nearest branch: x[(batch, ..., h, w)] on [B,C,H,W] after the mapping was
    downscaled by ``ratio`` (:1916-1980; the lexargunique there is an identity because ids are unique)."""
    pix = floor_div_pixels(pixels, ratio)
    return x[images_per_atom.long(), :, pix[:, 1], pix[:, 0]]


def sparse_interpolation(features, coords, batch):
    """image.py:105-170 with padding_mode='border'."""
    images_pad = torch.nn.ReplicationPad2d(1)(features)
    h, w = features.shape[2:]
    pixels = coords * torch.Tensor([[h, w]]) + 0.5
    top, bottom = torch.floor(pixels[:, 0]), torch.floor(pixels[:, 0] + 1)
    left, right = torch.floor(pixels[:, 1]), torch.floor(pixels[:, 1] + 1)
    tl, tr = torch.stack((top, left)).T.long(), torch.stack((top, right)).T.long()
    bl, br = torch.stack((bottom, left)).T.long(), torch.stack((bottom, right)).T.long()
    w_tl = torch.prod(pixels - br, dim=1).abs().unsqueeze(1)
    w_tr = torch.prod(pixels - bl, dim=1).abs().unsqueeze(1)
    w_bl = torch.prod(pixels - tr, dim=1).abs().unsqueeze(1)
    w_br = torch.prod(pixels - tl, dim=1).abs().unsqueeze(1)
    return (w_tl * images_pad[batch, :, tl[:, 0], tl[:, 1]] + w_tr * images_pad[batch, :, tr[:, 0], tr[:, 1]]
            + w_bl * images_pad[batch, :, bl[:, 0], bl[:, 1]] + w_br * images_pad[batch, :, br[:, 0], br[:, 1]])


def gather_bilinear(x, images_per_atom, pixels, mapping_size):
    """image.py:1278-1283: coords = pixels / (mapping_size - 1), swapped to (H, W) order."""
    resolution = torch.Tensor([mapping_size])
    coords = (pixels / (resolution - 1))[:, [1, 0]]
    return sparse_interpolation(x, coords, images_per_atom.long())
