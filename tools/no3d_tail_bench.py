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
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

POINTS = (300000, 1 << 20)
FRACTIONS = (0.9, 0.5, 0.01)
CLASSES = (13, 20)
VIEWS = (4, 32)
MAP_ROWS = 1 << 18
IGNORE = -1


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def alternate(ours, theirs, reps, warmup):
    for _ in range(warmup):
        ours()
        theirs()
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((ours, theirs)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return stats(ms[0]), stats(ms[1])


def observe(fn):
    """(host synchronisations that torch reports, peak MiB allocated above what is resident) of one call."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    syncs = sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in seen)
    return syncs, round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def side(timing, fn):
    syncs, peak = observe(fn)
    return dict(timing, host_syncs=syncs, peak_mib=peak)


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
    return {"N": n, "seen_fraction": frac, "K": K, "fill_unseen": side(a, ours), "composition": side(b, composition),
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
    return {"N": n, "views_per_point": views, "V": V, "K": K, "map_rows": MAP_ROWS, "view_nll": side(a, ours),
            "composition": side(b, composition), "speedup": round(b["median_ms"] / a["median_ms"], 2),
            "agree": {"loss": rel(la.detach(), lb.detach()), "grad": rel(ga, gb)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "no3d_tail_bench needs a HIP device"
    from deepviewagg_amd import _lib
    gen = torch.Generator().manual_seed(0)
    result = {"tool": "no3d_tail_bench", "device": torch.cuda.get_device_name(0),
              "dva_version": _lib.load().dva_version(), "kernel_sources_sha256": _lib.source_sha256(),
              "reps": args.reps, "warmup": args.warmup, "host_cpu_threads": torch.get_num_threads(),
              "timing": "host clock around a synchronised call, both sides alternating in one process; median and "
                        "[min, max] over reps; view_nll is forward + backward",
              "fill": [run_fill(n, f, K, args.reps, args.warmup, gen) for n in POINTS for f in FRACTIONS for K in CLASSES],
              "view_nll": [run_view(n, v, K, args.reps, args.warmup, gen) for n in POINTS for v in VIEWS for K in CLASSES]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
