#!/usr/bin/env python
"""Time the two device ops of the image-only model tail against the compositions they replace, on the same device.

  fill      ops.fill_unseen(x, pos, seen)           vs  compact pos by the mask twice, ops.knn_query(pos[~seen],
            pos[seen], 1), index-put of the rows (the composition available before; knn_query is unchanged)
  view_nll  ops.view_nll(lazy, labels, csr_idx)     vs  ops.log_softmax_nll(lazy.materialize(),
            labels.repeat_interleave(views per point)), forward + backward to the map rows

Sizes: N = 3 x 10^5 and 2^20 points in a 40 x 40 x 5 box; seen fractions 0.9 / 0.5 / 0.01; K = 13 and 20; 4 and 32
views per point over 2^18 map rows, 10 % of the labels ignored.  Both sides of a part run alternately in one process
after --warmup untimed rounds.  Every call is timed with the host clock around a synchronised call (the compositions
end their steps on the host), reported as the median and [min, max] over --reps; ``host_syncs`` counts what torch's
synchronisation debug mode reports during one call, ``peak_mib`` is the peak of allocated device memory above the
inputs during one call.  The results of the two sides are compared (``agree``).  One JSON line on stdout; --out writes
it (profiles/no3d_tail_bench.json).

Usage:  python tools/no3d_tail_bench.py [--reps 7] [--warmup 2] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import measure  # noqa: E402

POINTS = (300000, 1 << 20)
FRACTIONS = (0.9, 0.5, 0.01)
CLASSES = (13, 20)
VIEWS = (4, 32)
MAP_ROWS = 1 << 18
IGNORE = -1


def alternate(ours, theirs, reps, warmup):
    """[timing and counters of ours, of theirs]: host clock around a synchronised call, the two alternating."""
    arms = {"ours": ours, "theirs": theirs}
    ms, _ = measure.alternate(arms, reps, measure.host_window, warmup=warmup)
    sides = []
    for key, fn in arms.items():
        s, profile = measure.summarise(ms[key], 3), measure.profile_once(fn)
        sides.append({"median_ms": s["median"], "min_ms": s["min"], "max_ms": s["max"], "host_syncs": profile["syncs"],
                      "peak_mib": round(profile["peak_bytes"] / 2 ** 20, 1)})
    return sides


def run_fill(n, frac, K, reps, warmup, gen):
    from deepviewagg_amd import ops
    dev = torch.device("cuda", 0)
    pos = (torch.rand(n, 3, generator=gen) * torch.tensor([40.0, 40.0, 5.0])).to(dev)
    seen = (torch.rand(n, generator=gen) < frac).to(dev)
    x = torch.randn(n, K, generator=gen).to(dev)

    def ours():
        return ops.fill_unseen(x, pos, seen)[0]

    def composition():
        unseen = ~seen
        nbr, _ = ops.knn_query(pos[unseen], pos[seen], 1)
        out = x.clone()
        out[unseen] = x[seen][nbr[:, 0].long()]
        return out

    equal = bool(torch.equal(ours(), composition()))
    a, b = alternate(ours, composition, reps, warmup)
    return {"N": n, "seen_fraction": frac, "K": K, "fill_unseen": a, "composition": b,
            "speedup": round(b["median_ms"] / a["median_ms"], 2), "agree": {"rows_equal": equal}}


def run_view(n, views, K, reps, warmup, gen):
    from deepviewagg_amd import ops
    dev = torch.device("cuda", 0)
    V = n * views
    rows = torch.randn(MAP_ROWS, K, generator=gen).to(dev).requires_grad_(True)
    row_idx = torch.randint(0, MAP_ROWS, (V,), generator=gen, dtype=torch.int32).to(dev)
    csr_idx = (torch.arange(n + 1, dtype=torch.int64) * views).to(dev)
    labels = torch.randint(0, K, (n,), generator=gen)
    labels[torch.rand(n, generator=gen) < 0.1] = IGNORE
    labels = labels.to(dev)
    lazy = ops.GatheredFeatures(rows, row_idx, torch.zeros(MAP_ROWS, dtype=torch.int32, device=dev), True)

    def ours():
        rows.grad = None
        loss = ops.view_nll(lazy, labels, csr_idx, ignore_index=IGNORE)
        loss.backward()
        return loss

    def composition():
        rows.grad = None
        target = labels.repeat_interleave(csr_idx[1:] - csr_idx[:-1])
        _, loss = ops.log_softmax_nll(lazy.materialize(), target, ignore_index=IGNORE)
        loss.backward()
        return loss

    la = ours(); ga = rows.grad.clone()
    lb = composition(); gb = rows.grad.clone()
    rel = lambda p, q: float((p.double() - q.double()).abs().max() / q.double().abs().max().clamp_min(1e-300))
    a, b = alternate(ours, composition, reps, warmup)
    return {"N": n, "views_per_point": views, "V": V, "K": K, "map_rows": MAP_ROWS, "view_nll": a,
            "composition": b, "speedup": round(b["median_ms"] / a["median_ms"], 2),
            "agree": {"loss": rel(la.detach(), lb.detach()), "grad": rel(ga, gb)}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "no3d_tail_bench needs a HIP device"
    gen = torch.Generator().manual_seed(0)
    result = measure.header(
        "no3d_tail_bench", reps=args.reps, warmup=args.warmup, host_cpu_threads=torch.get_num_threads(),
        timing="host clock around a synchronised call, both sides alternating in one process; median and "
               "[min, max] over reps; view_nll is forward + backward")
    result["kernel_sources_sha256"] = result["source_sha256"]               # the name earlier records carry
    result["fill"] = [run_fill(n, f, K, args.reps, args.warmup, gen) for n in POINTS for f in FRACTIONS for K in CLASSES]
    result["view_nll"] = [run_view(n, v, K, args.reps, args.warmup, gen) for n in POINTS for v in VIEWS for K in CLASSES]
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
