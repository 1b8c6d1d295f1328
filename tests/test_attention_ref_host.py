"""CPU tests of tests/attention_ref.py: its fp32 evaluation is the oracle's attention tail (plus autograd), its softmax
reproduces the reference project's known answers, the geometry query of the library answers a pinned table, and every
case of tests/test_gpu_attention_f64.py meets its input conditions (generated here on the CPU from the same seeds)."""
import pytest
import torch

import attention_ref as A
from conftest import load_golden, t
from oracle import pooling_oracle as O

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def _oracle_tail(rows, row_idx, compat, ptr, gw, gb, scaling, w):
    C, G = rows.shape[1], compat.shape[1]
    x, c = rows.clone().requires_grad_(), compat.clone().requires_grad_()
    val = x if row_idx is None else x[row_idx.long()]
    gate_mod, params = None, []
    if gw is not None:
        gate_mod = O.Gating(G)
        with torch.no_grad():
            gate_mod.weight.copy_(gw)
            gate_mod.bias.copy_(gb)
        params = [gate_mod.weight, gate_mod.bias]
    out, att, gate = O.attention_tail(val, c, ptr, gate_mod, G, C, scaling)
    grads = torch.autograd.grad((out * w).sum(), [x, c] + params)
    return out, att, (gate.view(-1, G) if gate is not None else None), grads


@pytest.mark.parametrize("ints", [False, True], ids=["random", "tied"])
@pytest.mark.parametrize("C,G,gating,scaling,gather", [(8, 2, True, True, True), (7, 2, True, False, False),
                                                       (12, 1, False, True, True), (6, 6, True, True, False)])
def test_fp32_evaluation_is_the_oracle(C, G, gating, scaling, gather, ints):
    """Same expressions, same dtype: the two agree to the rounding of a differently ordered fp32 sum (a few ulp of
    the largest term; 1e-6 of the tensor's scale), and exactly in the argmax."""
    gen = torch.Generator().manual_seed(C * 10 + G + ints)
    sizes = torch.tensor([0, 1, 5, 0, 2, 9, 3, 1, 0])
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    N, V = sizes.shape[0], int(ptr[-1])
    R = 7 if gather else V
    rows = torch.randn(R, C, generator=gen)
    row_idx = torch.randint(0, R, (V,), generator=gen).int() if gather else None
    compat = torch.randint(-2, 3, (V, G), generator=gen).float() if ints else torch.randn(V, G, generator=gen)
    gw = torch.randn(1, G, generator=gen) if gating else None
    gb = torch.randn(1, G, generator=gen) * 0.5 if gating else None
    w = torch.randn(N, C, generator=gen)
    got = A.tail_ref(rows, row_idx, compat, ptr, gw, gb, scaling, w, dtype=F32)
    out, att, gate, grads = _oracle_tail(rows, row_idx, compat, ptr, gw, gb, scaling, w)

    def same(a, b):
        b = b.detach()
        torch.testing.assert_close(a, b, rtol=0, atol=1e-6 * max(1.0, float(b.abs().max())))
    same(got["out"], out)
    same(got["att"], att)
    same(got["grad_rows"], grads[0])
    same(got["grad_compat"], grads[1])
    if gating:
        same(got["gate"], gate)
        same(got["grad_gate_w"], grads[2].reshape(-1))
        same(got["grad_gate_b"], grads[3].reshape(-1))
    assert torch.equal(got["arg"], O.segment_arg(compat, ptr, "max"))
    assert bool((got["out"][sizes == 0] == 0).all())
    # the float64 evaluation of the same case is within fp32 rounding of it
    r64 = A.tail_ref(rows, row_idx, compat, ptr, gw, gb, scaling, w)
    for k in ("out", "att", "grad_rows", "grad_compat"):
        assert float((got[k].double() - r64[k]).abs().max()) <= 2e-5 * max(1.0, float(r64[k].abs().max())), k


def test_group_index_is_the_reference_split():
    assert A.group_index(7, 2).tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert A.group_index(20, 5).tolist() == [g for g in range(5) for _ in range(4)]
    assert A.group_index(5, 1).tolist() == [0] * 5 and A.group_index(3, 3).tolist() == [0, 1, 2]
    a = torch.arange(6.0).view(3, 2)
    assert torch.equal(O.expand_group_feat(a, 2, 7), a[:, A.group_index(7, 2)])


def test_softmax_known_answers():
    g = load_golden("softmax_known")
    src, ptr = t(g["src"]), t(g["csr"])
    src2 = src.view(src.shape[0], -1)
    ones = torch.ones(src2.shape[0], src2.shape[1])
    for scaling, key in ((False, "out"), (True, "out_scaled")):
        for dtype, tol in ((F32, 1e-6), (torch.float64, 1e-6)):
            att = A.tail_ref(ones, None, src2, ptr, None, None, scaling, None, dtype=dtype)["att"]
            assert float((att.double() - t(g[key]).view_as(att).double()).abs().max()) <= tol


def test_segmented_sum_references_agree_between_forms():
    gen = torch.Generator().manual_seed(3)
    N, V, R, C, G = 9, 40, 6, 8, 2
    att, gate = torch.rand(V, G, generator=gen), torch.rand(N, G, generator=gen)
    vp = torch.randint(0, N, (V,), generator=gen).int()
    row_idx = torch.randint(0, R, (V,), generator=gen).int()
    gout = torch.randn(N, C, generator=gen)
    a = A.rows_grad_ref(gout, row_idx, R, C, G, att=att, gate=gate, view_point=vp)
    rec = A.make_records(att, gate, vp, 8)
    b = A.rows_grad_ref(gout, row_idx, R, C, G, rec=rec)
    assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())        # the records hold the fp32 product
    loop = torch.zeros(R, C, dtype=torch.float64)
    for v in range(V):
        p = int(vp[v])
        for c in range(C):
            loop[int(row_idx[v]), c] += float(gout[p, c]) * float(att[v, c // 4]) * float(gate[p, c // 4])
    assert float((a - loop).abs().max()) <= 1e-12
    wts = torch.rand(4 * N, generator=gen)
    ridx = torch.randint(0, R, (4 * N,), generator=gen).int()
    s = A.rows_sum_ref(gout, ridx, R, wts, 2)
    loop = torch.zeros(R, C, dtype=torch.float64)
    for e in range(4 * N):
        loop[int(ridx[e])] += float(wts[e]) * gout[e >> 2].double()
    assert float((s - loop).abs().max()) <= 1e-12
    w4 = torch.rand(N, 4, generator=gen)
    anchors = torch.randint(0, 5, (N,), generator=gen).int()
    S = A.anchor_rows_sum_ref(gout, anchors, 5, w4)
    loop = torch.zeros(5, 4, C, dtype=torch.float64)
    for v in range(N):
        for k in range(4):
            loop[int(anchors[v]), k] += float(w4[v, k]) * gout[v].double()
    assert float((S - loop).abs().max()) <= 1e-12


# (dtype, C, G, N, V) -> (lpr, rows); (0, 0) = the generic kernels.  The four averages around the switch points
# rows / 2 >= 0.75 avg (2.67 and 5.33 for lpr = 8, 1.33 and 2.67 for lpr = 16) are the first eight lines.
GEOMETRY_TABLE = [
    (F32, 32, 4, 1000, 2666, (8, 2)), (F32, 32, 4, 1000, 2667, (8, 4)),
    (F32, 32, 4, 1000, 5333, (8, 4)), (F32, 32, 4, 1000, 5334, (8, 8)),
    (F32, 64, 4, 1000, 1333, (16, 1)), (F32, 64, 4, 1000, 1334, (16, 2)),
    (F32, 64, 4, 1000, 2666, (16, 2)), (F32, 64, 4, 1000, 2667, (16, 4)),
    (BF16, 64, 4, 1000, 2666, (8, 2)), (BF16, 64, 4, 1000, 2667, (8, 4)),
    (BF16, 64, 4, 1000, 5333, (8, 4)), (BF16, 64, 4, 1000, 5334, (8, 8)),
    (F16, 64, 8, 1000, 5334, (8, 8)), (F16, 64, 8, 1000, 1000, (8, 1)),
    (BF16, 128, 2, 1000, 2666, (16, 2)), (BF16, 128, 2, 1000, 2667, (16, 4)),
    (F32, 16, 1, 100, 1100, (4, 16)), (F32, 16, 1, 100, 1000, (4, 8)),
    (BF16, 512, 4, 100, 3200, (64, 1)), (F32, 128, 32, 100, 1000, (32, 2)), (F32, 128, 32, 100, 100, (32, 1)),
    (F32, 256, 4, 10, 320, (64, 1)), (F32, 512, 4, 10, 320, (0, 0)),                       # lpr = 128 > 64
    (F32, 7, 2, 10, 50, (0, 0)), (F32, 20, 5, 10, 50, (0, 0)), (BF16, 12, 4, 10, 50, (0, 0)),
    (F32, 24, 3, 10, 50, (0, 0)), (F32, 64, 32, 10, 50, (0, 0)), (BF16, 64, 16, 10, 50, (0, 0)),   # (C / G) % VEC
    (F32, 64, 4, 0, 0, (16, 1)),
]


def test_geometry_table():
    from deepviewagg_amd import _lib, ops
    lib = _lib.load()
    assert lib.dva_version() >= 320
    for dtype, C, G, N, V, want in GEOMETRY_TABLE:
        team, lpr, rows = A.geometry_of(lib, dtype, C, G, N, V)
        assert (lpr, rows) == want and team == int(want != (0, 0)), (dtype, C, G, N, V, (team, lpr, rows), want)
        # the Python mirror that sizes the view records agrees with the library's answer
        assert ops._team_records_ok(C, G, dtype) == bool(team), (dtype, C, G)
    import ctypes
    lpr, rows = ctypes.c_int32(), ctypes.c_int32()
    assert lib.dva_view_attention_geometry(64, 4, 10, 50, 7, ctypes.byref(lpr), ctypes.byref(rows)) == -1    # dtype
    assert lib.dva_view_attention_geometry(0, 4, 10, 50, 0, ctypes.byref(lpr), ctypes.byref(rows)) == -1
    assert lib.dva_view_attention_geometry(64, 4, 10, 50, 0, None, None) == -1


def test_case_list_reaches_every_form():
    geoms = {}
    for name in A.CASES:
        c = A.CASES[name]
        geoms.setdefault((c["geom"], c["dtype"]), []).append(c)
    for g in A.SPECIALISED:
        for dtype in (F32, BF16):
            assert (g, dtype) in geoms, (g, dtype)
        both = [c for (gg, _), cs in geoms.items() if gg == g for c in cs]
        assert {c["scaling"] for c in both} == {True, False} and {c["gating"] for c in both} == {True, False}, g
    assert ((8, 8), F16) in geoms and ((8, 4), F16) in geoms
    spec = [c for c in A.CASES.values() if c["geom"] in A.SPECIALISED]
    assert {1, 2, 4, 8} <= {c["G"] for c in spec}
    runtime = [c for c in A.CASES.values() if c["geom"] is not None and c["geom"] not in A.SPECIALISED]
    assert {(c["dtype"], c["C"], c["G"]) for c in runtime} >= {(F32, 16, 1), (BF16, 512, 4), (BF16, 64, 4)}
    assert any(c["G"] in (16, 32) for c in runtime)
    generic = {(c["dtype"], c["C"], c["G"], c["algo"]) for c in A.CASES.values() if c["geom"] is None}
    assert generic >= {(F32, 7, 2, 0), (F32, 20, 5, 0), (F32, 64, 4, 1), (BF16, 12, 4, 0)}
    assert any(c["ints"] and c["geom"] for c in A.CASES.values()) and any(c["ints"] and not c["geom"] for c in A.CASES.values())


@pytest.mark.parametrize("name", list(A.CASES))
def test_case_input_conditions(name):
    from deepviewagg_amd import _lib
    d = A.make_case(name)
    sizes, N, V, G = d["sizes"], d["N"], d["V"], d["G"]
    assert V < 10 ** 5 and sizes[0] == 0 and sizes[-1] == 0
    team, lpr, rows = A.geometry_of(_lib.load(), d["dtype"], d["C"], G, N, V)
    if d["geom"] is None:
        assert team == 0 or d["algo"] == 1, (team, lpr, rows)
    else:
        assert team == 1 and (lpr, rows) == d["geom"] and d["algo"] == 0, (team, lpr, rows)
    if d["n_grid"]:
        ts = lpr * rows
        assert N == 4096 * (256 // ts) + 3 and int(sizes.max()) <= (700 if d["geom"] == (8, 8) else 4)
        assert int((sizes <= 4).sum()) >= N - 64
    else:
        have = set(sizes.tolist())
        assert set(A.special_sizes(d)) <= have and max(have) >= 300, sorted(have)
        if d["geom"] is not None:
            U, cap = A.team_consts(d["dtype"], lpr, rows)
            assert {0, 1, U * rows, U * rows + 1, cap // G, cap // G + 1} <= have
            assert cap // G > U * rows          # the LDS-parked path exists between the other two
    if d["ints"]:
        assert torch.equal(d["compat"], d["compat"].round()) and float(d["compat"].abs().max()) == 2
        arg = A.reference(name, "val")[0]["arg"]
        mx = torch.cat([d["compat"], torch.zeros(1, G)]).gather(0, torch.where(arg < 0, torch.full_like(arg, V), arg))
        tied = (d["compat"] == mx[O.dense_index(d["ptr"])]).long()
        n_at_max = torch.zeros(N, G, dtype=torch.long).index_add(0, O.dense_index(d["ptr"]), tied)
        assert float((n_at_max > 1).float().mean()) > 0.15          # the max is tied in dozens of (point, group) entries
    if d["gating"]:
        r64, r32, window = A.reference(name, "val")
        pre = r64["pre"]
        pos = float((pre > 0).float().mean())
        assert 0.2 <= pos <= 0.8, pos
        assert float((pre.abs() <= window).float().mean()) <= 0.02
        assert window < 1e-4


def test_offset_pointers_are_refused_by_the_team_kernels():
    """``algo = 2`` asks for the team kernels or DVA_ERR_UNSUPPORTED: a team shape whose value, output or gradient
    pointer is no multiple of 16 bytes is refused before anything is launched (the pointers are never dereferenced, so
    made-up addresses do), which is the term that sends such a call to the generic kernels under ``algo = 0``.  An
    aligned call of the same shape would launch, so it is left to the GPU tests."""
    import ctypes
    from deepviewagg_amd import _lib
    lib = _lib.load()
    ok, off = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8)
    N, V, C, G = 10, 50, 64, 4
    for dtype in (0, 1, 2):
        for val, out in ((off, ok), (ok, off)):
            assert lib.dva_view_attention_fwd(val, ok, ok, None, None, out, ok, ok, ok, N, V, C, G, 1, 1e-12, dtype, 2,
                                              None) == -2
            assert lib.dva_view_gather_attention_fwd(val, ok, ok, ok, None, None, out, ok, ok, ok, N, V, C, G, 1, 1e-12,
                                                     dtype, 2, None) == -2
        for gout, val, gval in ((off, ok, ok), (ok, off, ok), (ok, ok, off)):
            assert lib.dva_view_attention_bwd(gout, val, ok, ok, ok, ok, ok, None, None, gval, ok, None, N, V, C, G, 1,
                                              dtype, 2, None) == -2
        for gout, rows in ((off, ok), (ok, off)):
            assert lib.dva_view_gather_attention_bwd(gout, rows, ok, ok, ok, ok, ok, ok, None, None, ok, ok, None, None,
                                                     0, N, V, C, G, 1, dtype, 2, None) == -2
    # a shape the teams do not cover is refused the same way, aligned or not
    assert lib.dva_view_attention_fwd(ok, ok, ok, None, None, ok, ok, ok, ok, N, V, 20, 5, 1, 1e-12, 0, 2, None) == -2
