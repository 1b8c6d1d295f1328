"""The fused first pass of the split plan for exact mappings (``dva_mapping_row_index_split``: row keys + the first
histogram from one kernel) against the two entries it replaces, byte for byte; and the 16-byte-store form of
``dva_csr_expand`` against ``torch.repeat_interleave``.  The sizes are tiny -- the properties are those of the tile
(4096 views) and of the 512-row bucket, not of the workload -- but for one case: the kernel form in which a workgroup
walks K tiles is only launched from K * 512 tiles on, so one mapping of that size is built on the device."""
import pytest
import torch

from deepviewagg_amd import _lib

DEV = "cuda:0"
TILE = 4096
FUSED_K = 16         # csrc/plan_split.hip DVA_PLAN_FUSED_K: tiles per workgroup of the fused kernel from K * 512 tiles on
V_CASES = (1, 4095, 4096, 4097, 3 * 4096 + 17, FUSED_K * 4096 - 1, FUSED_K * 4096 + 1)
MAPS = {"515_rows": (1, 5, 103), "2^18_rows": (32, 64, 128), "2880_rows": (3, 24, 40)}


def p(t):
    return _lib.ptr(t)


def build_old(images, pixels, ratio, B, H, W):
    """dva_mapping_row_index with atom_ptr = 0 .. V, then dva_plan_split_build; tables and scratch zeroed first."""
    lib = _lib.load()
    V, R = images.shape[0], B * H * W
    nbytes = int(lib.dva_plan_split_table_bytes(V, R))
    assert nbytes > 0, nbytes
    atom_ptr = torch.arange(V + 1, dtype=torch.int64, device=DEV)
    row_idx = torch.empty(V, dtype=torch.int32, device=DEV)
    row_ptr = torch.empty(R + 1, dtype=torch.int32, device=DEV)
    counts = torch.empty(R, dtype=torch.int32, device=DEV)
    tables = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    lows = torch.zeros(V, dtype=torch.int16, device=DEV)
    st = _lib.stream_of(images)
    _lib.check(lib.dva_mapping_row_index(p(images), p(atom_ptr), p(pixels), pixels.element_size(), float(ratio), V, V,
                                         B, H, W, p(row_idx), st), "dva_mapping_row_index")
    _lib.check(lib.dva_plan_split_build(p(row_idx), V, R, p(row_ptr), p(counts), p(tables), nbytes, p(lows), V * 2, st),
               "dva_plan_split_build")
    return row_idx, row_ptr, counts, tables


def build_new(images, pixels, ratio, B, H, W):
    lib = _lib.load()
    V, R = images.shape[0], B * H * W
    nbytes = int(lib.dva_plan_split_table_bytes(V, R))
    assert nbytes > 0, nbytes
    row_idx = torch.empty(V, dtype=torch.int32, device=DEV)
    row_ptr = torch.empty(R + 1, dtype=torch.int32, device=DEV)
    counts = torch.empty(R, dtype=torch.int32, device=DEV)
    tables = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    lows = torch.zeros(V, dtype=torch.int16, device=DEV)
    _lib.check(lib.dva_mapping_row_index_split(p(images), p(pixels), pixels.element_size(), float(ratio), V, B, H, W,
                                               p(row_idx), p(row_ptr), p(counts), p(tables), nbytes, p(lows), V * 2,
                                               _lib.stream_of(images)), "dva_mapping_row_index_split")
    return row_idx, row_ptr, counts, tables


def assert_same_build(images, pixels, ratio, B, H, W, what):
    old = build_old(images, pixels, ratio, B, H, W)
    new = build_new(images, pixels, ratio, B, H, W)
    for name, a, b in zip(("row_idx", "row_ptr", "counts", "tables"), old, new):
        assert torch.equal(a, b), (what, name, int((a != b).sum()))
    return new


def random_mapping(V, B, H, W, ratio, pix_dtype, gen):
    images = torch.randint(0, B, (V,), generator=gen)
    pixels = torch.stack([torch.randint(0, int(W * ratio), (V,), generator=gen),
                          torch.randint(0, int(H * ratio), (V,), generator=gen)], 1).to(pix_dtype)
    return images.to(DEV), pixels.to(DEV).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [1.0, 4.0])
@pytest.mark.parametrize("pix_dtype", [torch.int16, torch.int32, torch.int64])
@pytest.mark.parametrize("map_name", list(MAPS))
def test_fused_build_is_the_two_entry_build_byte_for_byte(map_name, pix_dtype, ratio):
    """row_idx, row_ptr, counts and the whole tables buffer of the fused build equal those of dva_mapping_row_index +
    dva_plan_split_build at every tile edge (one tile, K tiles, one view more or less), on maps just above one bucket,
    at the largest row count and at a row count that is no multiple of the bucket."""
    B, H, W = MAPS[map_name]
    gen = torch.Generator().manual_seed(len(map_name) * 7 + int(ratio))
    for V in V_CASES:
        images, pixels = random_mapping(V, B, H, W, ratio, pix_dtype, gen)
        row_idx, row_ptr, counts, _ = assert_same_build(images, pixels, ratio, B, H, W, (map_name, V))
        r = int(ratio)
        expect = (images.cpu() * H + pixels[:, 1].cpu().long() // r) * W + pixels[:, 0].cpu().long() // r
        assert torch.equal(row_idx.cpu().long(), expect), (map_name, V)
        assert torch.equal(counts.cpu().long(), torch.bincount(expect, minlength=B * H * W)), (map_name, V)
        assert int(row_ptr[-1]) == V


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["one_row", "last_bucket"])
def test_fused_build_on_crowded_keys(which):
    """Every view on the same row (one LDS counter takes a whole tile), and every view in the last bucket of a map whose
    row count is no multiple of 512 (the clamp of the high digit)."""
    B, H, W = 3, 24, 40                                   # 2880 rows: buckets 0 .. 5, the last one of 320 rows
    V = 3 * TILE + 17
    gen = torch.Generator().manual_seed(11)
    if which == "one_row":
        images = torch.full((V,), 1, dtype=torch.int64)
        pixels = torch.tensor([[7, 5]], dtype=torch.int16).repeat(V, 1)
    else:
        rows = torch.randint(5 * 512, B * H * W, (V,), generator=gen)
        images = rows // (H * W)
        pixels = torch.stack([rows % W, (rows // W) % H], 1).to(torch.int16)
    row_idx, _, counts, _ = assert_same_build(images.to(DEV), pixels.to(DEV).contiguous(), 1.0, B, H, W, which)
    if which == "one_row":
        assert int(counts[(1 * H + 5) * W + 7]) == V
    else:
        assert int(row_idx.min()) >= 5 * 512 and int(counts[5 * 512:].sum()) == V


@pytest.mark.gpu
def test_fused_build_where_a_workgroup_walks_k_tiles():
    """The threshold between the two forms of the fused kernel: K * 512 tiles and three and a bit more, so that the K-tile
    form runs, its last workgroup has fewer than K tiles and its last tile is not full (the mapping is drawn on the
    device; the comparison is the same byte identity)."""
    B, H, W = 32, 64, 128
    V = FUSED_K * 512 * TILE + 3 * TILE + 17
    gen = torch.Generator(device=DEV).manual_seed(9)
    images = torch.randint(0, B, (V,), generator=gen, device=DEV)
    pixels = torch.stack([torch.randint(0, W, (V,), generator=gen, device=DEV, dtype=torch.int16),
                          torch.randint(0, H, (V,), generator=gen, device=DEV, dtype=torch.int16)], 1).contiguous()
    row_idx, _, counts, _ = assert_same_build(images, pixels, 1.0, B, H, W, "k_tiles")
    expect = (images * H + pixels[:, 1]) * W + pixels[:, 0]
    assert torch.equal(row_idx.long(), expect)
    assert torch.equal(counts.long(), torch.bincount(expect, minlength=B * H * W))


def test_fused_entry_refuses_what_the_split_plan_refuses():
    """Argument checks return before any device call: the row counts ps::eligible refuses, null pointers, sizes."""
    lib = _lib.load()
    one = ctypes_one()
    args = lambda V, B, H, W, tb=1 << 20, sb=1 << 20, pix=2, ratio=1.0, ptrs=one: (
        ptrs, ptrs, pix, ratio, V, B, H, W, ptrs, ptrs, None, ptrs, tb, ptrs, sb, None)
    assert lib.dva_mapping_row_index_split(*args(100, 1, 16, 32)) == -2           # 512 rows: not more than one bucket
    assert lib.dva_mapping_row_index_split(*args(100, 33, 64, 128)) == -2         # more than 2^18 rows
    assert lib.dva_mapping_row_index_split(*args(0, 1, 5, 103)) == -2             # no views
    assert lib.dva_mapping_row_index_split(*args(-1, 1, 5, 103)) == -1
    assert lib.dva_mapping_row_index_split(*args(100, 1, 5, 103, ratio=0.5)) == -1
    assert lib.dva_mapping_row_index_split(*args(100, 1, 5, 103, pix=3)) == -1
    assert lib.dva_mapping_row_index_split(*args(100, 1, 5, 103, ptrs=None)) == -1
    assert lib.dva_mapping_row_index_split(*args(100, 1, 5, 103, tb=16)) == -1    # tables too small
    assert lib.dva_mapping_row_index_split(*args(100, 1, 5, 103, sb=199)) == -1   # scratch too small
    for V, R in ((100, 512), (100, (1 << 18) + 1), (0, 515)):
        assert lib.dva_plan_split_build(one, V, R, one, None, one, 1 << 20, one, 1 << 20, None) == -2


def ctypes_one():
    """A non-null, 16-byte aligned address that is never dereferenced (the calls above return at the argument checks)."""
    import ctypes
    return ctypes.c_void_p(4096)


@pytest.mark.gpu
def test_rows_gradient_over_the_fused_plan():
    """The plan works: the rows gradient through SplitPlan.sort_records (pass A) + dva_plan_split_rows_grad over the plan
    of the fused build equals the one over the two-entry build bit for bit (ragged points, a few thousand views)."""
    from deepviewagg_amd import ops
    B, H, W, C, G = 3, 24, 40, 64, 4
    gen = torch.Generator().manual_seed(5)
    sizes = torch.randint(0, 9, (1500,), generator=gen)
    sizes[7] = 90
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).to(DEV)
    V, N = int(csr[-1]), sizes.shape[0]
    images, pixels = random_mapping(V, B, H, W, 1.0, torch.int16, gen)
    gout = torch.randn(N, C, generator=gen).to(DEV).bfloat16()
    weights = torch.rand(V, 4, generator=gen).to(DEV).bfloat16().view(torch.int32)          # [V, 2]
    grads = []
    for build in (build_old, build_new):
        row_idx, row_ptr, _, tables = build(images, pixels, 1.0, B, H, W)
        rec = torch.cat([ops.csr_expand(csr, V)[:, None], weights, row_idx[:, None]], 1).contiguous()
        plan = ops.SplitPlan(row_idx, B * H * W, row_ptr, tables)
        g = plan.rows_grad_fused(gout, rec, C, G, _lib.stream_of(gout))
        assert g is not None
        grads.append(g)
    assert torch.equal(grads[0], grads[1])
    assert float(grads[0].float().abs().sum()) > 0


@pytest.mark.gpu
def test_ops_take_the_fused_build_for_exact_mappings(monkeypatch):
    """ops.mapping_row_index(exact=True) above the split plan's threshold: one timed region, the same row index, counts,
    row pointers and tables as the two-call path (exact=False)."""
    from deepviewagg_amd import ops
    monkeypatch.setattr(ops, "SPLIT_PLAN_MIN_VIEWS", 2048)
    B, H, W, V = 3, 24, 40, 2 * TILE + 5
    images, pixels = random_mapping(V, B, H, W, 4.0, torch.int16, torch.Generator().manual_seed(3))
    atom_ptr = torch.arange(V + 1, device=DEV)
    seen = []
    monkeypatch.setattr(ops, "_timed", lambda name, nbytes: seen.append(name) or ops._NO_TIMER)
    new = ops.mapping_row_index(images, atom_ptr, pixels, 4.0, B, H, W, exact=True)
    assert seen == ["mapping_row_plan"], seen
    del seen[:]
    old = ops.mapping_row_index(images, atom_ptr, pixels, 4.0, B, H, W)
    assert seen == ["gather_row_index", "row_plan"], seen
    assert isinstance(new[2], ops.SplitPlan) and isinstance(old[2], ops.SplitPlan)
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
    assert torch.equal(new[2].row_ptr, old[2].row_ptr)
    # below the threshold an exact mapping keeps the permutation plan
    monkeypatch.setattr(ops, "SPLIT_PLAN_MIN_VIEWS", 1 << 20)
    small = ops.mapping_row_index(images, atom_ptr, pixels, 4.0, B, H, W, exact=True)
    assert not isinstance(small[2], ops.SplitPlan) and torch.equal(small[0], old[0])


def csr_cases():
    gen = torch.Generator().manual_seed(21)
    short = torch.randint(1, 4, (300,), generator=gen)
    one_long = short.clone()
    one_long[130] = 400
    empties = torch.randint(0, 24, (333,), generator=gen)
    empties[:3] = 0
    empties[100:170] = 0                                   # a whole wavefront of empty points and more
    empties[-2:] = 0
    return {
        "empty_start_middle_end": empties,
        "only_one_view_points": torch.ones(700, dtype=torch.long),
        "uniform_32_N_64k": torch.full((64 * 9,), 32, dtype=torch.long),
        "uniform_32_N_64k_plus_5": torch.full((64 * 9 + 5,), 32, dtype=torch.long),
        "one_400_view_point_among_short": one_long,
        "ragged_0_to_23": torch.randint(0, 24, (1000,), generator=gen),
        "odd_long_segments": torch.randint(30, 300, (130,), generator=gen) * 2 + 1,
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(csr_cases()))
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_csr_expand_equals_repeat_interleave(name, misalign):
    """dva_csr_expand (16-byte stores on long segments, per-lane loops on short ones) == torch.repeat_interleave, which
    is what the one-point-after-the-other kernel before it was held to; also into an output that starts 4 or 12 bytes
    past a 16-byte boundary, with guard words on both sides."""
    lib = _lib.load()
    sizes = csr_cases()[name]
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).to(DEV)
    V, N = int(csr[-1]), sizes.shape[0]
    buf = torch.full((V + 8,), -7, dtype=torch.int32, device=DEV)
    out = buf[4 + misalign: 4 + misalign + V]
    _lib.check(lib.dva_csr_expand(p(csr), N, p(out), _lib.stream_of(csr)), "dva_csr_expand")
    expect = torch.repeat_interleave(torch.arange(N, dtype=torch.int32), sizes)
    assert torch.equal(out.cpu(), expect)
    assert bool((buf[:4 + misalign] == -7).all()) and bool((buf[4 + misalign + V:] == -7).all())
