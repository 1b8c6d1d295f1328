"""Row-wise comparison of the bf16 pooling path with its emulation oracle (gates: tolerances.py).

A relative L2 norm over a whole [N, C] tensor cannot see a defect confined to a few of its N rows, and the chain's
kernels go wrong exactly there: the point that closes a 32-view tile, a point cut into fragment tiles, a point at a
chunk boundary of the tile-table construction, the last point of the cloud, a point next to an unseen one, a map row
that a single view reads.  This module gives

* ``row_err``: one error per row, ``|got_i - ref_i|_2 / max(|ref_i|_2, rms_j |ref_j|_2)`` in float64.  The floor is
  the rms row norm of the live rows: in eval cases the gate tanh(relu(.)) is exactly 0 for more than half the points,
  so a plain per-row relative error is 0 / 0; below the floor the statistic is an absolute error in units of the
  typical row, on purpose;
* ``strata`` / ``read_strata``: boolean masks over the points (the map rows) by the position classes above, from the
  CSR pointers and the DEVICE's own tile table;
* ``gate_rows``: per stratum the max, and for strata of >= ``P99_MIN_ROWS`` rows the p99, of the device's row error
  against the float64 emulation, each held to ``headroom`` x the SAME statistic of a plain evaluation's own error
  (bf16(float32 emulation) against the float64 emulation) taken over ALL live rows of the case -- a small stratum's
  own noise max is too lucky a draw.  No row tolerance is typed in.

Plain Python (not a conftest): tests import it by name, like tolerances.py."""
import copy
import os

import torch

from tolerances import FP32_HEADROOM, P99_MIN_ROWS, ROW_MAX, ROW_P99

VIEWS_PER_CHUNK = 512           # == fused_chain.VIEWS_PER_CHUNK (asserted by the GPU tests that pass the table in)


def _rows64(t):
    t = t.detach().double().cpu()
    return t.reshape(t.shape[0], -1)


def row_err(got, ref, live=None):
    """float64 [n]: ``|got_i - ref_i| / max(|ref_i|, rms_j |ref_j|)`` (j over the live rows); NaN outside ``live``."""
    g, r = _rows64(got), _rows64(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    live = torch.ones(r.shape[0], dtype=torch.bool) if live is None else live.cpu()
    nr = r.norm(dim=1)
    floor = float(nr[live].pow(2).mean().sqrt()) if bool(live.any()) else 0.0
    err = (g - r).norm(dim=1) / nr.clamp_min(floor).clamp_min(1e-300)
    return torch.where(live, err, torch.full_like(err, float("nan")))


def score_err(got, ref, csr):
    """float64 [N]: per point, ``max_v |got - ref|`` over its views (and groups) over ``max |ref|``; NaN for points
    without views."""
    g, r = _rows64(got), _rows64(ref)
    N = csr.shape[0] - 1
    sizes = (csr[1:] - csr[:-1]).cpu()
    pid = torch.arange(N).repeat_interleave(sizes)
    d = (g - r).abs().amax(dim=1)
    worst = torch.zeros(N, dtype=torch.float64).scatter_reduce(0, pid, d, "amax", include_self=True)
    worst = worst / max(float(r.abs().max()), 1e-300)
    return torch.where(sizes > 0, worst, torch.full_like(worst, float("nan")))


def chunk_step(V, views_per_chunk=VIEWS_PER_CHUNK):
    """The view step of the tile-table construction (fused_chain.build_tiles): chunk c takes the points whose views
    start in [c step, (c + 1) step)."""
    n_chunks = max(1, min(1 << 17, (V + views_per_chunk - 1) // views_per_chunk))
    return (V + n_chunks - 1) // n_chunks if V > 0 else 1


def strata(csr, tiles=None, views_per_chunk=VIEWS_PER_CHUNK):
    """{name: bool [N]} over the points.  ``tiles``: int [T, 2] = (first view, n_views | frag << 8), the device's own
    table (fused_chain.build_tiles, cut to its n_tiles); None for a path without one (the tile strata are left out and
    ``fragmented`` is read off the pointers: more than 32 views)."""
    csr = csr.cpu().long()
    N = csr.shape[0] - 1
    start, end = csr[:-1], csr[1:]
    sizes = end - start
    seen = sizes > 0
    V = int(csr[-1])
    s = {"views_1": sizes == 1, "views_2_31": (sizes >= 2) & (sizes <= 31), "views_32": sizes == 32,
         "views_33_64": (sizes >= 33) & (sizes <= 64), "views_ge65": sizes >= 65}
    if tiles is not None:
        t = tiles.cpu().long()
        v0, nv, frag = t[:, 0].contiguous(), t[:, 1] & 0xff, t[:, 1] >> 8
        ti = (torch.searchsorted(v0, start, right=True) - 1).clamp_min(0)     # the tile that holds the point's first view
        whole = seen & (frag[ti] == 0)
        first = whole & (start == v0[ti])
        last = whole & (end == v0[ti] + nv[ti])
        s["tile_first"], s["tile_last"] = first, last
        s["tile_interior"] = whole & ~first & ~last
        s["fragmented"] = seen & (frag[ti] != 0)
    else:
        s["fragmented"] = sizes > 32
    # views [start, end) touch or cross a positive multiple m of the chunk step: start <= m <= end
    edge = torch.zeros(N, dtype=torch.bool)
    for step in {views_per_chunk, chunk_step(V, views_per_chunk)}:
        m = torch.div(end, step, rounding_mode="floor") * step            # the largest multiple <= end
        edge |= seen & (m >= start) & (m > 0)
    s["chunk_edge"] = edge
    ids = torch.nonzero(seen).flatten()
    s["cloud_first"], s["cloud_last"] = torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
    if ids.numel():
        s["cloud_first"][ids[0]] = True
        s["cloud_last"][ids[-1]] = True
    unseen = ~seen
    nxt = torch.zeros(N, dtype=torch.bool)
    nxt[:-1] |= unseen[1:]
    nxt[1:] |= unseen[:-1]
    s["next_to_unseen"] = seen & nxt
    return s


def read_strata(row_idx, R):
    """({name: bool [R]}, live [R]) over the map rows by the number of views that read the row (a bucket of
    plan_split.hip holds 512 map rows)."""
    n = torch.bincount(row_idx.cpu().long().flatten(), minlength=R)
    return ({"read_1": n == 1, "read_2_31": (n >= 2) & (n <= 31), "read_32_511": (n >= 32) & (n <= 511),
             "read_ge512": n >= 512}, n > 0)


def stats(err, mask):
    """(max, p99 or None when the stratum has fewer than P99_MIN_ROWS rows, number of rows)."""
    e = err[mask]
    assert not bool(torch.isnan(e).any()), "a stratum holds rows that are not live"
    k = int(e.numel())
    if k == 0:
        return None, None, 0
    return float(e.max()), (float(torch.quantile(e, 0.99)) if k >= P99_MIN_ROWS else None), k


def gate_rows(report, case, tensor, err, noise, masks, live, headroom=FP32_HEADROOM, open_findings=None,
              plain_noise=None):
    """One report row per stratum x statistic: the device's ``err`` in the stratum against ``headroom`` x the statistic
    of ``noise`` over all live rows.  ``open_findings``: {(tensor, stratum, "max" | "p99"): (measured, cause)} -- rows
    entered with ``Report.add_open`` (they must still miss the gate and not grow).  ``plain_noise``: the noise of the
    emulation WITHOUT the set-branch split, when ``noise`` is the one with it: the report notes by how much the
    yardstick of this tensor grew.  Returns the worst err / noise ratio."""
    live = live.cpu()
    n_max, n_p99, n_live = stats(noise, live)
    worst = 0.0
    if plain_noise is not None:
        q_max, q_p99, _ = stats(plain_noise, live)
        report.notes.append(f"{case} {tensor}: noise with the set-branch split max {n_max:.2e} p99 {n_p99 or 0:.2e}; "
                            f"without it max {q_max:.2e} p99 {q_p99 or 0:.2e} (yardstick x {n_max / max(q_max, 1e-300):.1f} / "
                            f"x {(n_p99 or 0) / max(q_p99 or 0, 1e-300):.1f})")

    def add(name, k, stat, cls, e, n):
        key = (tensor, name, stat)
        label = f"{tensor} [{name}: {k}] {stat}"
        if open_findings and key in open_findings:
            measured, why = open_findings[key]
            report.add_open(case, label, cls, e, n, measured, why)
        else:
            report.add(case, label, cls, e, fp32_err=n, headroom=headroom)
        return e / max(n, 1e-300)
    for name, mask in [("all", live)] + [(k, m & live) for k, m in masks.items()]:
        e_max, e_p99, k = stats(err, mask)
        if k == 0:
            continue
        worst = max(worst, add(name, k, "max", ROW_MAX, e_max, n_max))
        if e_p99 is not None and n_p99 is not None:
            worst = max(worst, add(name, k, "p99", ROW_P99, e_p99, n_p99))
    return worst


def failing_rows(err, noise, live, headroom=FP32_HEADROOM):
    """Indices of the live rows whose own error is above the max gate (``headroom`` x the noise max over the live
    rows): where a failed stratum statistic comes from."""
    n_max, _, _ = stats(noise, live.cpu())
    return torch.nonzero(live.cpu() & (torch.nan_to_num(err, nan=0.0) > headroom * n_max)).flatten()


def as_device_rounds(t, like):
    """The float32 emulation's tensor rounded to the dtype the kernel stores (bf16 / fp16 rows), back in float64."""
    return t.detach().to(like.dtype).double().cpu()


def double_twin(module):
    """A float64 copy of an oracle module in the same train / eval mode (parameters and buffers are the fp32 values)."""
    return copy.deepcopy(module).double()


def emulate(ref, sd, rows, row_idx, x_map, csr, w, dtype=torch.float32, dev_invstd=None, dev_scores=None, set_split=True):
    """One evaluation of the chain's emulation oracle in ``dtype`` (float64: the same bf16 operand roundings, everything
    else double) from the state ``sd``: dict(out_own, scores = the emulation's OWN output and scores, out and
    rows_grad = output and gradient of sum(out w) with respect to the map rows, evaluated at ``dev_scores`` when
    given).  ``set_split``: the set branch with the three-term split of chain_set.hip (oracle/chain_emulation.py)."""
    from oracle.chain_emulation import emulated_chain
    ref.load_state_dict(sd)
    mod = ref if dtype == torch.float32 else double_twin(ref)
    r = rows.detach().to(dtype).cpu().requires_grad_()
    xm = x_map.to(dtype)
    kw = dict(dev_invstd=dev_invstd, set_split=set_split)
    res = {}
    if dev_scores is not None:      # the forward statement is about the emulation's own scores: one more evaluation
        with torch.no_grad():
            res["out_own"], res["scores"] = emulated_chain(mod, r[row_idx.long()], xm, csr, return_scores=True, **kw)
        out = emulated_chain(mod, r[row_idx.long()], xm, csr, dev_scores=dev_scores.to(dtype), **kw)
    else:
        out, sc = emulated_chain(mod, r[row_idx.long()], xm, csr, return_scores=True, **kw)
        res["out_own"], res["scores"] = out.detach(), sc.detach()
    res["out"] = out.detach()
    res["rows_grad"], = torch.autograd.grad((out * w.to(dtype)).sum(), [r])
    ref.load_state_dict(sd)
    return res


def emulate_all(ref, sd, rows, row_idx, x_map, csr, w, dev_invstd, dev_scores):
    """{(set_split, dtype): emulate(...)} for the plain and the split set branch, float32 and float64."""
    return {(sp, dt): emulate(ref, sd, rows, row_idx, x_map, csr, w, dtype=dt, dev_invstd=dev_invstd,
                              dev_scores=dev_scores, set_split=sp)
            for sp in (False, True) for dt in (torch.float32, torch.float64)}


def gate_chain(rep, label, ev, csr, masks, out, dev_scores, rows_grad=None, read=None, read_live=None):
    """The row-wise statements of one chain case (``ev`` from ``emulate_all``); returns {tensor: worst ratio}.

    * ``out@dev_scores`` and ``rows_grad`` -- the tail evaluated at the device's scores, nothing of the set branch's
      rounding decisions left in them -- are held to the PLAIN yardstick: device against the plain float64 emulation,
      gate = headroom x bf16(plain float32 emulation) against it.  This statement does not grow with the split.
    * ``out`` (the emulation's own scores) and ``scores`` are compared with the float64 emulation whose set branch has
      the three-term split of chain_set.hip, and gated by the noise of the split pair.  That noise is LARGER than the
      plain one (the bf16 rounding of `lo` is one more discontinuity that an fp32-level change flips): the report notes
      both, per case."""
    p32, p64, s32, s64 = (ev[(sp, dt)] for sp in (False, True) for dt in (torch.float32, torch.float64))
    seen = (csr[1:] > csr[:-1]).cpu()
    worst = {}
    for e64 in (p64, s64):
        for key in ("out_own", "out"):
            assert float(e64[key][~seen].abs().max() if (~seen).any() else 0.0) == 0.0
    noise = row_err(as_device_rounds(p32["out"], out), p64["out"], seen)
    worst["out@dev_scores"] = gate_rows(rep, label, "out@dev_scores", row_err(out, p64["out"], seen), noise, masks, seen)
    noise = row_err(as_device_rounds(s32["out_own"], out), s64["out_own"], seen)
    plain = row_err(as_device_rounds(p32["out_own"], out), p64["out_own"], seen)
    worst["out"] = gate_rows(rep, label, "out", row_err(out, s64["out_own"], seen), noise, masks, seen, plain_noise=plain)
    worst["scores"] = gate_rows(rep, label, "scores", score_err(dev_scores, s64["scores"], csr),
                                score_err(s32["scores"], s64["scores"], csr), masks, seen,
                                plain_noise=score_err(p32["scores"], p64["scores"], csr))
    if rows_grad is not None:
        assert float(rows_grad.detach().float().cpu()[~read_live].abs().max() if (~read_live).any() else 0.0) == 0.0
        noise = row_err(as_device_rounds(p32["rows_grad"], rows_grad), p64["rows_grad"], read_live)
        worst["rows_grad"] = gate_rows(rep, label, "rows_grad", row_err(rows_grad, p64["rows_grad"], read_live), noise,
                                       read, read_live)
    return worst


def edges(N, gen):
    """View counts at the edges of the tile table: 0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 100, 511, 512, 513 and 5000,
    planted at the start of the cloud, at its end and around multiples of 512 views (a point that ends on one, one
    that starts on one, one that crosses one), unseen points first, last and in runs.  The total is a multiple of 512,
    so that the construction's chunk step IS 512 and the planted positions are its chunk boundaries."""
    special = [1, 2, 31, 32, 33, 63, 64, 65, 96, 100, 511, 512, 513]
    out = []

    def total():
        return sum(out)

    def filler(k):
        out.extend(torch.randint(0, 9, (k,), generator=gen).tolist())

    def align(residue):
        """points of at most 31 views until total % 512 == residue"""
        while (residue - total()) % 512:
            gap = (residue - total()) % 512
            out.append(min(gap, int(torch.randint(20, 32, (1,), generator=gen))))

    out += [0, 0, 0] + special + [5000, 0]                          # start of the cloud: an unseen run first
    for rep in range(16):
        for k in special + ([5000] if rep == 7 else []):
            filler(int(torch.randint(1, 6, (1,), generator=gen)))
            if rep % 4 == 1:
                out.extend([0] * (1 + rep % 3))                     # an unseen run in front of the planted point
            if rep % 2 == 0:
                align((512 - k) % 512 if rep % 4 == 0 else 512 - (k % 512) // 2)   # ends on a multiple / crosses one
            out.append(k)
            if rep % 4 == 0:
                out.append(special[(rep // 4 + k) % len(special)])      # ... and the next one starts on it
    tail = special[::-1] + [5000, 70, 0, 0]                         # end of the cloud: unseen points last
    room = N - len(out) - len(tail)
    assert room > 600, (N, len(out), len(tail))
    filler(room - 520)
    # the rest of the points brings the total to a multiple of 512: ones, then zeros
    need = (-(total() + sum(tail))) % 512
    left = N - len(out) - len(tail)
    assert need <= left
    out += [1] * need + [0] * (left - need)
    out += tail
    sizes = torch.tensor(out, dtype=torch.long)
    assert sizes.numel() == N and int(sizes.sum()) % 512 == 0
    return sizes


def write_report(report):
    """Append the table to the file named by DVA_ROWWISE_REPORT (how profiles/rowwise_report.txt is produced)."""
    path = os.environ.get("DVA_ROWWISE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(report.table() + "\n")
