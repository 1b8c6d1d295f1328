#!/usr/bin/env python
"""Time the voted / full-resolution evaluation tail on the device against what a user runs without it.

Sizes: raw clouds of 2^22 and 2^24 points (uniform in a 40 x 40 x 4 box), 30 % of them voted, C = 13 and 20 classes,
batches of 3 x 10^5 rows of fp32 outputs resident on the device; every voted point is in one batch, and one more batch
overlaps the others.  Two parts, three arms each:

  accumulate  new     metrics.full_res.VoteAccumulator.add per batch (ops.vote_add)
              torch   ``votes[ids] += out; counts[ids] += 1`` on the same device
              host    the reference's dataflow: ``out.cpu()`` and the same two lines on the host
  finalise    new     VoteAccumulator.full_res_predictions(pos, labels=y) and the C x C matrix read back (S3DIS: k = 1)
              torch   ops.knn_query + gather + argmax + ConfusionMatrix.count_predicted_batch on the same device, the
                      [N, C] interpolated tensor materialised as the reference does
              host    votes and positions on the host, scipy.spatial.cKDTree 1-NN on 16 threads, numpy argmax / bincount

The arms of a part run alternately after --warmup untimed rounds; the time is the median over --reps of device events
around one call for ``accumulate`` (new, torch), and of the host clock around a synchronised call wherever an arm ends
on the host.  The host arm of ``finalise`` runs --host-reps times without a warm-up: it takes seconds.  ``agree`` holds
the comparison of the results at the sizes timed; ``peak_mib`` the peak device memory of the two device arms of
``finalise`` above what was allocated before the call.  One JSON line on stdout; --out writes it
(profiles/full_res_vote_bench.json).

Usage:  python tools/full_res_vote_bench.py [--reps 5] [--warmup 1] [--host-reps 1] [--sizes 22,24] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import measure  # noqa: E402

BATCH = 300000
VOTED = 0.3
CLASSES = (13, 20)


def timed(fn, host_clock):
    if host_clock:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(arms, reps, warmup):
    """arms: [(fn, host_clock, reps or None)]; median ms per arm, the arms run alternately."""
    for _ in range(warmup):
        for fn, _, own in arms:
            if own is None:
                fn()
    ms = [[] for _ in arms]
    for r in range(reps):
        for i, (fn, host_clock, own) in enumerate(arms):
            if own is None or r < own:
                ms[i].append(timed(fn, host_clock))
    return [round(statistics.median(m), 3) for m in ms]


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def run_size(N, C, reps, warmup, host_reps, gen):
    from scipy.spatial import cKDTree
    from deepviewagg_amd import ops
    from deepviewagg_amd.metrics.confusion_matrix import ConfusionMatrix
    from deepviewagg_amd.metrics.full_res import VoteAccumulator
    dev = torch.device("cuda", 0)
    pos_h = torch.rand(N, 3, generator=gen) * torch.tensor([40.0, 40.0, 4.0])
    y_h = torch.randint(0, C, (N,), generator=gen)
    voted = torch.randperm(N, generator=gen)[:int(VOTED * N)]
    batches = [voted[a:a + BATCH] for a in range(0, voted.numel(), BATCH)]
    batches.append(voted[torch.randperm(voted.numel(), generator=gen)[:BATCH]])          # overlaps the others
    pos, y = pos_h.to(dev), y_h.to(dev)
    ids = [b.to(dev) for b in batches]
    outs = [torch.rand(b.numel(), C, generator=gen).to(dev) for b in batches]
    rows = sum(b.numel() for b in batches)
    out = {"N": N, "C": C, "voted": int(voted.numel()), "batches": len(batches), "rows": rows}

    # --- accumulate --------------------------------------------------------------------------------------------
    acc = VoteAccumulator(N, C, dev)
    tv, tc = torch.zeros(N, C, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
    hv, hc = torch.zeros(N, C), torch.zeros(N, dtype=torch.int32)

    def add_new():
        for i, o in zip(ids, outs):
            acc.add(i, o)

    def add_torch():
        for i, o in zip(ids, outs):
            tv[i] += o
            tc[i] += 1

    def add_host():
        for i, o in zip(ids, outs):
            ih, oh = i.cpu(), o.cpu()
            hv[ih] += oh
            hc[ih] += 1

    t_new, t_torch, t_host = alternate([(add_new, False, None), (add_torch, False, None), (add_host, True, None)],
                                       reps, warmup)
    out["accumulate"] = {"new_ms": t_new, "torch_ms": t_torch, "host_ms": t_host,
                         "agree": {"votes_equal_torch": bool(torch.equal(acc.votes, tv)),
                                   "counts_equal_torch": bool(torch.equal(acc.counts, tc)),
                                   "votes_equal_host": bool(torch.equal(acc.votes.cpu(), hv))}}

    # --- finalise ----------------------------------------------------------------------------------------------
    res = {}

    def fin_new():
        pred, cm = acc.full_res_predictions(pos, labels=y)
        res["new"] = (pred, cm.confusion_matrix)

    def fin_torch():
        has = tc > 0
        x = tv[has]
        nbr, d2 = ops.knn_query(pos, pos[has], 1)                                       # all queries in one call
        w = 1.0 / torch.clamp(d2, min=1e-16)
        full = (x[nbr[:, 0].long()] * w) / w                                            # [N, C], as the reference
        pred = full.argmax(1)
        cm = ConfusionMatrix(C)
        cm.count_predicted_batch(y, pred)
        res["torch"] = (pred, cm.confusion_matrix)

    def fin_host():
        votes, counts = acc.votes.cpu().numpy(), acc.counts.cpu().numpy()
        has = counts > 0
        _, nn = cKDTree(pos_h.numpy()[has]).query(pos_h.numpy(), k=1, workers=16)
        pred = np.argmax(votes[has][nn], 1)
        res["host"] = (pred, np.bincount(y_h.numpy() * C + pred, minlength=C * C).reshape(C, C))

    mem_new, mem_torch = peak_mib(fin_new), peak_mib(fin_torch)
    t_new, t_torch, t_host = alternate([(fin_new, True, None), (fin_torch, True, None), (fin_host, True, host_reps)],
                                       max(reps, host_reps), warmup)
    p_new, p_host = res["new"][0].cpu().numpy(), res["host"][0]
    out["finalise"] = {"new_ms": t_new, "torch_ms": t_torch, "host_ms": t_host,
                       "peak_mib": {"new": mem_new, "torch": mem_torch},
                       "agree": {"pred_equal_torch": bool(torch.equal(res["new"][0], res["torch"][0])),
                                 "matrix_equal_torch": bool(np.array_equal(res["new"][1], res["torch"][1])),
                                 # the KD-tree measures in float64 and leaves ties open: a fraction, not a flag
                                 "pred_equal_host_fraction": float((p_new == p_host).mean())}}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--sizes", default="22,24", help="log2 of the raw cloud sizes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "full_res_vote_bench needs a HIP device"
    gen = torch.Generator().manual_seed(0)
    sizes = [(1 << int(s), C) for s in args.sizes.split(",") for C in CLASSES]
    rows = []
    for N, C in sizes:
        rows.append(run_size(N, C, args.reps, args.warmup, args.host_reps, gen))
        print(f"done N={N} C={C}", file=sys.stderr, flush=True)
    result = measure.header(
        "full_res_vote_bench", reps=args.reps, warmup=args.warmup, host_reps=args.host_reps,
        host_cpu_threads=torch.get_num_threads(),
        timing="median ms; accumulate new / torch: device events around all batches; every other arm: host "
               "clock around a synchronised call; the arms of a part alternate in one process",
        sizes=rows)
    result["kernel_sources_sha256"] = result["source_sha256"]               # the name earlier records carry
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
