"""-m gpu: the view-attention kernels of csrc/attention.hip against the float64 references of tests/attention_ref.py,
on every branch their dispatchers can take.

Every case of ``attention_ref.CASES`` runs through ``ops.view_attention`` (materialised values) and
``ops.view_gather_attention`` (``rows[row_idx]``) with ``ops.LEAN_ATTENTION_BWD = False``, so that the backward is
attention.hip's own (the lean kernels of chain_bwd.hip are held equal to it by test_gpu_ops.py).  Which kernels a case
runs is asserted through ``dva_view_attention_geometry`` -- the rule the dispatchers themselves call -- and the input
conditions of every case (segment lengths at the boundaries of the three backward paths, both ReLU sides of the gate
populated, few entries near the kink) are asserted on the CPU by tests/test_attention_ref_host.py.

Gates, none typed in: ``tolerances.gate(cls, fp32_err)`` for fp32 storage, the half-ulp rule of ``Report.hold`` for
bf16 / fp16 storage, ``torch.equal`` for the argmax.  ``-s`` prints one table per case.

Dispatch (``team_geometry``: lpr = C / VEC lanes per row, ``rows`` shrinks with the average segment):
  compiled <8, 8>, <16, 4>, <8, 4>, <16, 2>; the run-time instance for every other team pair; the generic kernels for
  C / G the teams do not cover, for ``ATTENTION_ALGO = 1`` and for base pointers that are no multiple of 16 bytes.
Backward team kernel, by segment length n: registers (n <= U rows), parked in LDS (gather form, n G <= 1024 ts / 64),
  round trip through grad_compat.  Every team case has n on both sides of both boundaries.
Rows gradients (C ABI, over ``ops.row_plan``): team kernels (64 / lpr row slots x U views per step) and the generic ones.
"""
import pytest
import torch

import attention_ref as A
import primitives_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ROWS_SWEEP = 4096 * 4            # rows one sweep of the capped grid covers: 4096 blocks x 4 wavefronts, a row each
GENERIC_SWEEP = 4096 * 256       # (row, channel) elements one sweep of the generic kernels covers


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def offset8(t):
    """A contiguous copy of ``t`` that starts 8 bytes into a 16-byte aligned buffer."""
    k = 8 // t.element_size()
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 8
    return v


def assert_geometry(d):
    from deepviewagg_amd import _lib
    team, lpr, rows = A.geometry_of(_lib.load(), d["dtype"], d["C"], d["G"], d["N"], d["V"])
    if d["geom"] is None:
        assert team == 0 or d["algo"] == 1, (d["name"], team, lpr, rows)
    else:
        assert team == 1 and (lpr, rows) == d["geom"] and d["algo"] == 0, (d["name"], team, lpr, rows)


def run_form(monkeypatch, name, form, misalign=False):
    """One forward + backward of a case on the device -> dict of detached device tensors."""
    from deepviewagg_amd import ops
    d = A.make_case(name)
    monkeypatch.setattr(ops, "LEAN_ATTENTION_BWD", False)
    monkeypatch.setattr(ops, "ATTENTION_ALGO", d["algo"])
    place = offset8 if misalign else (lambda t: t)
    x = place((d["rows"] if form == "gather" else d["val"]).to(DEV)).requires_grad_()
    c = d["compat"].to(DEV).requires_grad_()
    gw = d["gate_w"].to(DEV).requires_grad_() if d["gating"] else None
    gb = d["gate_b"].to(DEV).requires_grad_() if d["gating"] else None
    ptr = d["ptr"].to(DEV)
    if form == "gather":
        out, att, gate = ops.view_gather_attention(x, d["row_idx"].to(DEV), c, ptr, gw, gb, scaling=d["scaling"])
    else:
        out, att, gate = ops.view_attention(x, c, ptr, gw, gb, scaling=d["scaling"])
    gout = place(d["w"].to(d["dtype"]).to(DEV))
    grads = torch.autograd.grad(out, [x, c] + ([gw, gb] if d["gating"] else []), grad_outputs=gout)
    torch.cuda.synchronize()
    res = dict(out=out.detach(), att=att.detach(), gate=gate.detach(), grad_x=grads[0], grad_compat=grads[1])
    if d["gating"]:
        res["grad_gate_w"], res["grad_gate_b"] = grads[2].reshape(-1), grads[3].reshape(-1)
    return res


def hold_form(rep, name, form, got):
    d = A.make_case(name)
    r64, r32, n_kink = A.reference_for(name, form, got["gate"])
    case = f"{name}/{form}"
    assert got["out"].dtype == d["dtype"] and got["grad_x"].dtype == d["dtype"]
    for key, cls in (("out", "out"), ("att", "out")) + ((("gate", "out"),) if d["gating"] else ()):
        rep.hold(case, key, cls, got[key], r64[key], r32[key])
    gx = "grad_rows" if form == "gather" else "grad_val"
    rep.hold(case, gx, "grad_in", got["grad_x"], r64[gx], r32[gx])
    rep.hold(case, "grad_compat", "grad_in", got["grad_compat"], r64["grad_compat"], r32["grad_compat"])
    if d["gating"]:
        for key in ("grad_gate_w", "grad_gate_b"):
            rep.hold(case, key, "grad_param", got[key], r64[key], r32[key])
        rep.notes.append(f"{case}: {n_kink} of {d['N'] * d['G']} gate entries inside the kink window "
                         f"(side taken from the run)")
    else:
        assert bool((got["gate"] == 1).all())
    assert bool((got["out"][(d["sizes"] == 0).to(DEV)] == 0).all()), "empty segments give 0"


@pytest.mark.parametrize("name", list(A.CASES))
def test_attention_f64(name, monkeypatch):
    d = A.make_case(name)
    assert_geometry(d)
    rep = P.Report(f"view attention against float64: {name} (N = {d['N']}, V = {d['V']}, C = {d['C']}, G = {d['G']}, "
                   f"geometry {d['geom'] or 'generic'}, gating {d['gating']}, scaling {d['scaling']})")
    for form in ("val", "gather"):
        hold_form(rep, name, form, run_form(monkeypatch, name, form))
    rep.check()


def test_case_list_names_every_form():
    geoms = {(c["geom"], c["dtype"]) for c in A.CASES.values()}
    for g in A.SPECIALISED:
        assert (g, F32) in geoms and (g, BF16) in geoms
    assert ((8, 8), F16) in geoms and ((8, 4), F16) in geoms
    assert {(4, 16), (32, 2), (64, 1), (8, 2)} <= {g for g, _ in geoms}           # the run-time instance
    assert len(A.GENERIC_CASES) >= 5 and any(A.CASES[k]["algo"] == 1 for k in A.GENERIC_CASES)


@pytest.mark.parametrize("name", ["f32-16x4-ties", "f32-gen-C20-ties"])
def test_argmax_of_tied_scores(name):
    """Raw ABI: ``amax`` is the FIRST row of the group max (-1 for an empty segment), in both forward entries."""
    from deepviewagg_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    d = A.make_case(name)
    assert_geometry(d)
    N, V, C, G = d["N"], d["V"], d["C"], d["G"]
    ref = A.reference(name, "val")[0]["arg"]
    val, rows, ridx = d["val"].to(DEV), d["rows"].to(DEV), d["row_idx"].to(DEV)
    compat, ptr, gw, gb = d["compat"].to(DEV), d["ptr"].to(DEV), d["gate_w"].reshape(-1).to(DEV), d["gate_b"].reshape(-1).to(DEV)
    algo = 2 if d["geom"] is not None else 1
    for form in ("val", "gather"):
        out = torch.empty(N, C, device=DEV)
        att = torch.zeros(V, G, device=DEV)
        gate = torch.empty(N, G, device=DEV)
        amax = torch.full((N, G), -7, dtype=torch.int32, device=DEV)
        tail = (p(compat), p(ptr), p(gw), p(gb), p(out), p(att), p(gate), p(amax), N, V, C, G, int(d["scaling"]), 1e-12,
                A.DTYPE_CODE[d["dtype"]], algo, None)
        if form == "val":
            rc = lib.dva_view_attention_fwd(p(val), *tail)
        else:
            rc = lib.dva_view_gather_attention_fwd(p(rows), p(ridx), *tail)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(amax.cpu().long(), ref), form


@pytest.mark.parametrize("name", ["f32-16x4", "bf16-8x8"])
def test_attention_offset_by_8_bytes(name, monkeypatch):
    """Values / rows and the output gradient start 8 bytes into their buffers: contiguous, but no base for the 16-byte
    accesses of the team kernels -- the dispatchers take the generic kernels, and the same gates hold."""
    rep = P.Report(f"view attention, base pointers offset by 8 bytes: {name}")
    for form in ("val", "gather"):
        hold_form(rep, name, form, run_form(monkeypatch, name, form, misalign=True))
    rep.check()


def test_team_case_is_deterministic(monkeypatch):
    """Two runs, equal bits.  The gradients of the gate's two parameters are sums of fp32 atomics (LDS partials per
    block, one global atomic per block: csrc/attention.hip), the only outputs whose order of summation is not fixed:
    the case without gating has none and is compared in every output, the gated one in every other output."""
    for name in ("bf16-16x4", "f32-16x4"):
        for form in ("val", "gather"):
            a = run_form(monkeypatch, name, form)
            b = run_form(monkeypatch, name, form)
            assert set(a) - {"grad_gate_w", "grad_gate_b"} == {"out", "att", "gate", "grad_x", "grad_compat"}
            for k in ("out", "att", "gate", "grad_x", "grad_compat"):
                assert torch.equal(bits(a[k]), bits(b[k])), (name, form, k)


# ----------------------------------------------------------------------------------------------
# rows gradients over a row plan (C ABI)
# ----------------------------------------------------------------------------------------------
def populations(lpr, U):
    slots = 64 // lpr
    return [0, 1, slots * U, slots * U + 1, 300]


def plan_on_device(row_idx, n_rows):
    from deepviewagg_amd import ops
    (perm, row_ptr), _ = ops.row_plan(row_idx, n_rows, with_counts=False, split=False)
    return perm, row_ptr


def rows_grad_inputs(dtype, C, G, R, seed):
    team = C % A.vec_of(dtype) == 0 and G in (1, 2, 4, 8)
    lpr = C // A.vec_of(dtype) if team else 16
    row_idx, counts = A.plan_rows(populations(lpr, 4), R, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    V, N = row_idx.shape[0], 211
    att, gate = torch.rand(V, G, generator=gen), torch.rand(N, G, generator=gen)
    vp = torch.randint(0, N, (V,), generator=gen).int()
    gout = torch.randn(N, C, generator=gen).to(dtype)
    return row_idx, counts, att, gate, vp, gout


def call_rows_grad(dtype, C, G, R, row_idx, plan, gout, att=None, gate=None, vp=None, rec=None):
    from deepviewagg_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    grows = torch.full((R, C), float("nan"), device=DEV)
    keep = [t.to(DEV) if t is not None else None for t in (gout, att, gate, vp, rec)]
    rs = rec.shape[1] if rec is not None else 0
    _lib.check(lib.dva_view_gather_rows_grad(p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), p(plan[0]), p(plan[1]),
                                             p(keep[4]), rs, p(grows), R, row_idx.shape[0], C, G, A.DTYPE_CODE[dtype],
                                             None), "dva_view_gather_rows_grad")
    torch.cuda.synchronize()
    return grows


ROWS_GRAD = [(F32, 64, 4, 97), (BF16, 64, 2, 97), (F16, 64, 1, 97), (F32, 24, 3, 97),
             (F32, 64, 4, ROWS_SWEEP + 37), (F32, 24, 3, GENERIC_SWEEP // 24 + 37)]


@pytest.mark.parametrize("dtype,C,G,R", ROWS_GRAD, ids=lambda v: str(v).replace("torch.", ""))
def test_rows_grad_f64(dtype, C, G, R):
    """dva_view_gather_rows_grad: team form (C / VEC a power of two, G a power of two) and generic form (C = 24,
    G = 3); inputs as att / gate / view_point with and without a gate, and as fp32 records; rows of 0, 1,
    slots U, slots U + 1 and 300 views; R below and above one sweep of the capped grid."""
    row_idx, counts, att, gate, vp, gout = rows_grad_inputs(dtype, C, G, R, 7 * C + G + R)
    assert R == 97 or (R * C > GENERIC_SWEEP if C == 24 else R > ROWS_SWEEP)
    plan = plan_on_device(row_idx.to(DEV), R)
    assert torch.equal((plan[1][1:] - plan[1][:-1]).cpu().long(), counts)
    rep = P.Report(f"dva_view_gather_rows_grad against float64: {dtype} C = {C} G = {G} R = {R} V = {row_idx.shape[0]}")
    rec = A.make_records(att, gate, vp, 8)
    rec0 = A.make_records(att, None, vp, 8)
    for label, kw in (("att+gate", dict(att=att, gate=gate, view_point=vp)), ("att", dict(att=att, view_point=vp)),
                      ("records", dict(rec=rec)), ("records, no gate", dict(rec=rec0))):
        dev_kw = {("vp" if k == "view_point" else k): v for k, v in kw.items()}
        got = call_rows_grad(dtype, C, G, R, row_idx, plan, gout, **dev_kw)
        r64 = A.rows_grad_ref(gout, row_idx, R, C, G, **kw)
        r32 = A.rows_grad_ref(gout, row_idx, R, C, G, dtype=F32, **kw)
        rep.hold("rows_grad", label, "grad_in", got, r64, r32)
        assert bool((got[(counts == 0).to(DEV)] == 0).all())
    rep.check()


def test_rows_grad_is_deterministic():
    dtype, C, G, R = BF16, 64, 2, 97
    row_idx, counts, att, gate, vp, gout = rows_grad_inputs(dtype, C, G, R, 5)
    plan = plan_on_device(row_idx.to(DEV), R)
    a = call_rows_grad(dtype, C, G, R, row_idx, plan, gout, att=att, gate=gate, vp=vp)
    b = call_rows_grad(dtype, C, G, R, row_idx, plan, gout, att=att, gate=gate, vp=vp)
    assert torch.equal(bits(a), bits(b))


ROWS_SUM = [(F32, 64, 97), (BF16, 64, 97), (F16, 128, 97), (F32, 24, 97), (F16, 40, 97), (BF16, 64, ROWS_SWEEP + 37),
            (F32, 24, GENERIC_SWEEP // 24 + 37)]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights-shift2"])
@pytest.mark.parametrize("dtype,C,R", ROWS_SUM, ids=lambda v: str(v).replace("torch.", ""))
def test_rows_sum_f64(dtype, C, R, weighted):
    """dva_gather_rows_sum: team form and generic form (C = 24 fp32, C = 40 fp16: C / VEC no power of two), entries
    = atoms, and entries = 4 weighted taps per atom (atom_shift 2)."""
    from deepviewagg_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    vec = A.vec_of(dtype)
    lpr = C // vec if C % vec == 0 and (C // vec) & (C // vec - 1) == 0 else 16
    row_idx, counts = A.plan_rows(populations(lpr, 4), R, 3 * C + R + weighted)
    E = row_idx.shape[0]
    gen = torch.Generator().manual_seed(E)
    shift = 2 if weighted else 0
    gout = torch.randn((E + (1 << shift) - 1) >> shift, C, generator=gen).to(dtype)
    weights = torch.rand(E, generator=gen) if weighted else None
    plan = plan_on_device(row_idx.to(DEV), R)
    gout_d, w_d = gout.to(DEV), (weights.to(DEV) if weighted else None)
    grows = torch.full((R, C), float("nan"), device=DEV)
    _lib.check(lib.dva_gather_rows_sum(p(gout_d), p(plan[0]), p(plan[1]), p(w_d), shift, p(grows), R, E, C,
                                       A.DTYPE_CODE[dtype], None), "dva_gather_rows_sum")
    torch.cuda.synchronize()
    rep = P.Report(f"dva_gather_rows_sum against float64: {dtype} C = {C} R = {R} entries = {E} shift = {shift}")
    rep.hold("rows_sum", "grad_rows", "grad_in", grows, A.rows_sum_ref(gout, row_idx, R, weights, shift),
             A.rows_sum_ref(gout, row_idx, R, weights, shift, dtype=F32))
    assert bool((grows[(counts == 0).to(DEV)] == 0).all())
    rep.check()


@pytest.mark.parametrize("dtype,C,R", [(F32, 64, 97), (BF16, 64, 97), (F32, 32, ROWS_SWEEP + 37)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_anchor_rows_sum_f64(dtype, C, R):
    """dva_anchor_rows_sum (the plain form, two views per slot and step): S[a][k] = sum_v w[v][k] gout[v]."""
    from deepviewagg_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    anchors, counts = A.plan_rows(populations(C // A.vec_of(dtype), 2), R, 11 * C + R)
    V = anchors.shape[0]
    gen = torch.Generator().manual_seed(V)
    gout = torch.randn(V, C, generator=gen).to(dtype)
    w4 = torch.rand(V, 4, generator=gen)
    plan = plan_on_device(anchors.to(DEV), R)
    gout_d, w_d = gout.to(DEV), w4.to(DEV)
    S = torch.full((R, 4, C), float("nan"), device=DEV)
    _lib.check(lib.dva_anchor_rows_sum(p(gout_d), p(plan[0]), p(plan[1]), p(w_d), p(S), R, V, C, A.DTYPE_CODE[dtype],
                                       None), "dva_anchor_rows_sum")
    torch.cuda.synchronize()
    rep = P.Report(f"dva_anchor_rows_sum against float64: {dtype} C = {C} anchors = {R} V = {V}")
    rep.hold("anchor_rows_sum", "S", "grad_in", S, A.anchor_rows_sum_ref(gout, anchors, R, w4),
             A.anchor_rows_sum_ref(gout, anchors, R, w4, dtype=F32))
    assert bool((S[(counts == 0).to(DEV)] == 0).all())
    rep.check()
