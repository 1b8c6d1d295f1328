"""Row-wise comparison of the sparse convolution with its split emulation (statistics: rowwise.py, gates:
tolerances.py).

``max|got - ref64| <= 2e-5 max|ref64|`` over a whole tensor has to be that wide because the 3-term bf16 split of
sparseconv.hip is 5e-6 .. 7e-6 away from exact float64 BY DESIGN; a float64 evaluation of the split itself
(oracle.sparseconv_oracle.sparse_conv_split) is what a correct kernel sits ~1.5e-7 from.  This module gives

* ``strata_cloud``: a voxel cloud whose first part is SORTED ascending (b, z, y, x) as real tensors are
  (``downsample_coords``) and made of a solid block (27 neighbours inside), the same block at the same coordinates in a
  second batch item (a map that crossed the batch column would pair them), a line (3 neighbours: 64 consecutive rows
  share 24 missing offsets, the skip branch of ``sconv_apply_kernel``), a plane (9) and isolated voxels (centre only),
  followed by a shuffled surface cloud far away (no wavefront skips anything there);
* ``conv_strata`` / ``wgrad_strata``: boolean masks over the destination rows / over the rows of ``grad W`` seen as
  [K Cin, Cout], from the ORACLE's kernel map;
* ``gate``: one tensor of one case through ``rowwise.row_err`` / ``rowwise.gate_rows``: the device against the float64
  yardstick per stratum, held to FP32_HEADROOM x the same statistic of a plain evaluation (float32, rounded to the
  device's storage type) against that yardstick over all live rows.  No row tolerance is typed in.

Plain Python (not a conftest): tests import it by name, like rowwise.py."""
import numpy as np
import torch

import rowwise as RW

WAVE_ROWS = 64          # destination rows of one wavefront of sconv_apply_kernel
FAR = 1000              # where the shuffled surface part starts


def surface_part(n, extent, seed, batches=1, lo=FAR):
    """Voxels near the faces of a box, unique rows (x, y, z, b), SHUFFLED."""
    rng = np.random.default_rng(seed)
    p = rng.integers(lo, lo + extent, size=(n, 3))
    face = rng.integers(0, 3, n)
    p[np.arange(n), face] = lo + rng.integers(0, 2, n) * (extent - 1)
    b = rng.integers(0, batches, size=(n, 1))
    c = np.unique(np.concatenate([p, b], 1), axis=0)
    rng.shuffle(c)
    return c.astype(np.int64)


def structured_part():
    """Block, line, plane, isolated voxels in batch 0 (each in a z range of its own, so that each is a run of
    consecutive rows once sorted) and the block again in batch 1; sorted ascending (b, z, y, x)."""
    r6 = np.arange(6)
    block = np.stack(np.meshgrid(r6, r6, r6, indexing="ij"), -1).reshape(-1, 3)
    line = np.stack([np.arange(200), np.full(200, 3), np.full(200, 10)], 1)
    r12 = np.arange(12)
    plane = np.stack(np.meshgrid(r12, r12, indexing="ij"), -1).reshape(-1, 2)
    plane = np.concatenate([plane, np.full((144, 1), 20)], 1)
    lat = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3)[:70]
    lone = lat * 3 + np.array([0, 0, 30])

    def rows(xyz, b):
        return np.concatenate([xyz, np.full((xyz.shape[0], 1), b)], 1)
    c = np.concatenate([rows(block, 0), rows(line, 0), rows(plane, 0), rows(lone, 0), rows(block, 1)]).astype(np.int64)
    return c[np.lexsort((c[:, 0], c[:, 1], c[:, 2], c[:, 3]))]


def strata_cloud(seed, n_surface, stride=1):
    """int32 [n, 4] (x, y, z, b): the sorted structured part (846 voxels) followed by a shuffled surface cloud drawn from
    ``n_surface`` points (fewer voxels: duplicates go).  ``stride``: every coordinate times it (a tensor at that
    stride)."""
    parts = [structured_part()]
    if n_surface > 0:
        parts.append(surface_part(n_surface, 14 if n_surface <= 2000 else 40, seed))
    c = np.concatenate(parts)
    c[:, :3] *= stride
    assert np.unique(c, axis=0).shape[0] == c.shape[0]
    return torch.from_numpy(c.astype(np.int32))


def conv_strata(nbr, require=()):
    """{name: bool [n_dst]} from the oracle's map ``nbr`` int [K, n_dst]; every stratum named in ``require`` must hold
    at least one row."""
    nbr = torch.as_tensor(nbr).cpu()
    K, n = nbr.shape
    has = nbr >= 0
    cnt = has.sum(0)
    j = torch.arange(n)
    s = {"nbr_0": cnt == 0, "nbr_1": cnt == 1, "nbr_2_8": (cnt >= 2) & (cnt <= 8), "nbr_9_26": (cnt >= 9) & (cnt <= 26),
         "nbr_27": cnt == 27,
         "tile_edge": ((j % WAVE_ROWS == 0) | (j % WAVE_ROWS == 31) | (j % WAVE_ROWS == 32) | (j % WAVE_ROWS == 63)),
         "last_tile": j >= WAVE_ROWS * (n // WAVE_ROWS)}
    skips = torch.zeros(n, dtype=torch.bool)
    for b0 in range(0, n, WAVE_ROWS):
        if bool((~has[:, b0:b0 + WAVE_ROWS].any(1)).any()):       # an offset without any neighbour in this 64-row block
            skips[b0:b0 + WAVE_ROWS] = True
    s["wave_skips"], s["wave_no_skip"] = skips, ~skips
    for name in require:
        assert bool(s[name].any()), f"stratum {name} is empty"
    return s


def skipped_offsets(nbr):
    """Per 64-row block, the number of offsets the wavefront skips."""
    has = torch.as_tensor(nbr).cpu() >= 0
    return [int((~has[:, b0:b0 + WAVE_ROWS].any(1)).sum()) for b0 in range(0, has.shape[1], WAVE_ROWS)]


def wgrad_strata(nbr, cin, require=()):
    """({name: bool [K cin]}, live [K cin]) over the rows of ``grad W`` seen as [K cin, Cout], by the number of pairs
    under the row's offset.  Rows outside ``live`` (an offset without any pair) must be exactly 0."""
    pairs = (torch.as_tensor(nbr).cpu() >= 0).sum(1).repeat_interleave(cin)
    s = {"pairs_1_31": (pairs >= 1) & (pairs <= 31), "pairs_32_2047": (pairs >= 32) & (pairs <= 2047),
         "pairs_ge2048": pairs >= 2048}
    for name in require:
        assert bool(s[name].any()), f"stratum {name} is empty"
    return s, pairs > 0


def gate(rep, case, tensor, dev, ref64, plain, masks=None, live=None, require=(), open_findings=None):
    """``dev`` against the float64 yardstick ``ref64`` per stratum, gated by FP32_HEADROOM x the statistic of ``plain``
    (one plain evaluation in the arithmetic of the device, float32) rounded to the dtype ``dev`` is stored in.  Rows
    outside ``live`` must be exactly zero on the device and in the yardstick.  Returns the worst err / noise ratio."""
    n = ref64.shape[0]
    live = torch.ones(n, dtype=torch.bool) if live is None else live
    masks = {} if masks is None else masks
    for name in require:
        assert bool((masks[name] & live).any()), f"{case} {tensor}: stratum {name} is empty"
    d = dev.detach().cpu()
    if bool((~live).any()):
        assert float(d.reshape(n, -1)[~live].double().abs().max()) == 0.0, f"{case} {tensor}: a dead row is not 0"
        assert float(ref64.reshape(n, -1)[~live].abs().max()) == 0.0
    err = RW.row_err(d, ref64, live)
    # no float32 evaluation is expected closer to the yardstick than one float32 unit roundoff: a plain evaluation that
    # happens to be exact (a bias gradient of 7 sums of bf16 values is, on the CPU) does not make the gate 0
    noise = RW.row_err(RW.as_device_rounds(plain, dev), ref64, live).clamp_min(torch.finfo(torch.float32).eps / 2)
    return RW.gate_rows(rep, case, tensor, err, noise, masks, live, open_findings=open_findings)


def map_cloud(n_src, seed, stride=1, duplicates=False):
    """(src, dst) int32 [n, 4] for a kernel-map test: ``n_src`` source rows with negative coordinates, two batch items
    that hold EQUAL coordinates (the second half repeats xyz of the first in batch 1), shuffled; ``dst`` = another
    shuffle of three quarters of the source voxels plus as many voxels far away (no neighbour at all).  Coordinates are
    multiples of ``stride``.  ``duplicates``: a fifth of the source rows is overwritten with copies of other rows (the
    smallest row id must win)."""
    rng = np.random.default_rng(seed)
    half = (n_src + 1) // 2
    ext = max(2, int(round((half * 1.5) ** (1 / 3))) + 1)
    cells = np.stack(np.meshgrid(*[np.arange(-(ext // 2), ext - ext // 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    xyz = cells[rng.permutation(cells.shape[0])[:half]]
    src = np.concatenate([np.concatenate([xyz, np.zeros((half, 1), dtype=np.int64)], 1),
                          np.concatenate([xyz, np.ones((half, 1), dtype=np.int64)], 1)[:n_src - half]])
    src = src[rng.permutation(n_src)]
    if duplicates and n_src >= 5:
        to = rng.permutation(n_src)[:n_src // 5]
        src[to] = src[rng.integers(0, n_src, to.shape[0])]
    near = src[rng.permutation(n_src)[:max(1, 3 * n_src // 4)]]
    far = near + np.array([10 * ext + 7, 0, 0, 0])
    dst = np.concatenate([near, far])
    dst = dst[rng.permutation(dst.shape[0])]
    src[:, :3] *= stride
    dst[:, :3] *= stride
    return torch.from_numpy(src.astype(np.int32)), torch.from_numpy(dst.astype(np.int32))


MAP_SIZES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4096, 4097)     # the table capacity steps at 32 -> 33, 64 -> 65


# ---- cases: inputs, oracle maps and every CPU evaluation, computed once per session and left unchanged ----------------
_cases = {}


def maps(coords, k=3, stride=1, tensor_stride=1, dilation=1):
    """(dst coords, offsets, nbr [K, n_dst], nbr_t [K, n_src]) of a convolution on ``coords``, all from the oracle:
    ``nbr`` = map(src, dst, offsets), ``nbr_t`` = map(dst, src, -offsets)."""
    from oracle import sparseconv_oracle as O
    dst = coords if stride == 1 else O.downsample_coords(coords, tensor_stride * stride)
    offs = O.kernel_offsets(k, tensor_stride, dilation)
    return dst, offs, O.kernel_map_sorted(coords, dst, offs), O.kernel_map_sorted(dst, coords, -offs)


def conv_case(name, coords, cin, cout, k=3, stride=1, bias=False, transpose=False, dtype=torch.float32, seed=0):
    """One convolution case with its float64 yardsticks and plain float32 evaluations.

    fp32 features: yardstick = the 3-term split in float64, plain = the split in float32, and ``exact`` = the exact
    float64 oracle with its autograd gradients (the kept 2e-5 statement).  bf16 features: yardstick = the float64
    oracle on the bf16 operands (W rounded to bf16), plain = the same in float32.  ``transpose``: the maps of the
    strided convolution with the roles swapped, as Conv3d._maps does."""
    from oracle import sparseconv_oracle as O
    if name in _cases:
        return _cases[name]
    fine_dst, offs, nbr, nbr_t = maps(coords, k, stride)
    if transpose:
        src_coords, dst_coords, nbr, nbr_t, offs = fine_dst, coords, nbr_t, nbr, -offs
    else:
        src_coords, dst_coords = coords, fine_dst
    gen = torch.Generator().manual_seed(seed)
    K, n_src, n_dst = nbr.shape[0], src_coords.shape[0], dst_coords.shape[0]
    x = torch.randn(n_src, cin, generator=gen).to(dtype)
    W = torch.randn(K, cin, cout, generator=gen) / np.sqrt(cin * K / 4)
    b = torch.randn(cout, generator=gen) if bias else None
    g = torch.randn(n_dst, cout, generator=gen).to(dtype)
    c = dict(name=name, src=src_coords, dst=dst_coords, offs=offs, nbr=nbr, nbr_t=nbr_t, x=x, W=W, b=b, g=g, dtype=dtype,
             cin=cin, cout=cout, K=K)
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        xe, ge = x.to(dt), g.to(dt)
        be = None if b is None else b.to(dt)
        if dtype == torch.float32:
            We = W.to(dt)
            c["out" + tag] = O.sparse_conv_split(xe, We, be, nbr)
            c["gx" + tag] = O.sparse_conv_split_grad_x(ge, We, nbr_t)
            c["gW" + tag] = O.sparse_conv_split_grad_w(xe, ge, nbr)
            if dt == torch.float32:     # the same float32 evaluation in the kernel's accumulation order
                c["out32o"] = O.sparse_conv_split_mfma_order(xe, We, be, nbr)
                c["gx32o"] = O.sparse_conv_split_mfma_order(ge, We.transpose(1, 2), None, nbr_t)
        else:
            We = W.bfloat16().to(dt)
            c["out" + tag] = O.sparse_conv(xe, We, be, nbr)
            c["gx" + tag] = O.sparse_conv(ge, We.transpose(1, 2), None, nbr_t)
            c["gW" + tag] = O.sparse_conv_grad_w(xe, ge, nbr)
        c["gb" + tag] = ge.sum(0, keepdim=True)
    if dtype == torch.float32:
        xr, Wr = x.double().requires_grad_(True), W.double().requires_grad_(True)
        br = None if b is None else b.double().requires_grad_(True)
        ref = O.sparse_conv(xr, Wr, br, nbr)
        ref.backward(g.double())
        c["exact"] = dict(out=ref.detach(), gx=xr.grad, gW=Wr.grad, gb=None if br is None else br.grad.reshape(1, -1))
    _cases[name] = c
    return c


def gate_case(rep, c, out=None, gx=None, gW=None, gb=None, require=(), require_t=(), require_w=(), open_findings=None):
    """Every tensor given, of the device or of a stand-in for it, through ``gate``; returns {tensor: worst ratio}."""
    worst = {}
    if out is not None:
        worst["out"] = gate(rep, c["name"], "out", out, c["out64"], c["out32"], conv_strata(c["nbr"]), require=require,
                            open_findings=open_findings)
    if gx is not None:
        worst["grad_x"] = gate(rep, c["name"], "grad_x", gx, c["gx64"], c["gx32"], conv_strata(c["nbr_t"]),
                               require=require_t, open_findings=open_findings)
    if gW is not None:
        masks, live = wgrad_strata(c["nbr"], c["cin"])
        worst["grad_W"] = gate(rep, c["name"], "grad_W", gW.reshape(-1, c["cout"]), c["gW64"].reshape(-1, c["cout"]),
                               c["gW32"].reshape(-1, c["cout"]), masks, live, require=require_w,
                               open_findings=open_findings)
    if gb is not None:
        worst["grad_b"] = gate(rep, c["name"], "grad_b", gb.reshape(1, -1), c["gb64"], c["gb32"],
                               open_findings=open_findings)
    return worst


def gate_kernel_order(rep, c, out, gx):
    """The proof behind an open finding of an fp32 case: the same strata of ``out`` and ``grad_x`` against the same
    float64 yardstick, with the noise taken from the float32 evaluation in the KERNEL'S accumulation order
    (oracle.sparse_conv_split_mfma_order).  A stratum that misses the plain gate and meets this one differs from the
    plain evaluation by the order of its fp32 additions and nothing else; every stratum must meet this one."""
    tag = "[noise in kernel order] "
    return {"out": gate(rep, c["name"], tag + "out", out, c["out64"], c["out32o"], conv_strata(c["nbr"])),
            "grad_x": gate(rep, c["name"], tag + "grad_x", gx, c["gx64"], c["gx32o"], conv_strata(c["nbr_t"]))}


def old_metric(got, ref):
    """The whole-tensor statement the GPU tests keep: max|got - ref| / max|ref| (held to 2e-5 against exact float64)."""
    r = ref.detach().double()
    return float((got.detach().cpu().double() - r).abs().max()) / (float(r.abs().max()) + 1e-12)
