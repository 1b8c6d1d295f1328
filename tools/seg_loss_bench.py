#!/usr/bin/env python
"""Time the tail of the segmentation step on the device against what a user runs without it.

Sizes: P = 3 x 10^5 and 2^20 points, C = 13 and 20 classes, 10 % of the labels ignored, class weights, fp32 logits
resident on the device.  Three parts, each forward + backward where it has a backward:

  nll       ops.log_softmax_nll                     vs  F.log_softmax + F.nll_loss (torch, same device)
  lovasz    ops.lovasz_softmax_flat on the probas   vs  the plain torch composition of the loss (the restatement of
            tools/gen_golden_seg_loss.py: a Python loop of one sort, two cumsum and a dot per class) on the same device
  tracker   metrics.segmentation_tracker.compute_metrics (counts on the device, C x C read back)
            vs  the copy-to-host path: mask, ``.cpu().numpy()`` of the [P, C] outputs, np.argmax, np.bincount

Both sides of a part run alternately in the same call after --warmup untimed rounds; the time is the median over --reps
of device events around one call (the tracker, which ends on the host, is timed with the host clock around a
synchronised call).  The results of the two sides are compared at the sizes timed (``agree``).  One JSON line on
stdout; --out writes it (profiles/seg_loss_bench.json).

Usage:  python tools/seg_loss_bench.py [--reps 9] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import gen_golden_seg_loss as GEN  # noqa: E402
import measure  # noqa: E402

SIZES = [(300000, 13), (300000, 20), (1 << 20, 13), (1 << 20, 20)]
IGNORE = -1


def alternate(ours, theirs, reps, warmup, host_clock=False):
    """median ms of ``ours()`` and of ``theirs()``, run alternately."""
    ms, _ = measure.alternate({"ours": ours, "theirs": theirs}, reps,
                              measure.host_window if host_clock else measure.event_window, warmup=warmup)
    return [measure.summarise(m, 3)["median"] for m in ms.values()]


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def run_size(P, C, reps, warmup, gen):
    from deepviewagg_amd import ops
    from deepviewagg_amd.metrics.confusion_matrix import ConfusionMatrix
    from deepviewagg_amd.metrics.segmentation_tracker import compute_metrics
    dev = torch.device("cuda", 0)
    logits = (2 * torch.randn(P, C, generator=gen)).to(dev).requires_grad_(True)
    labels = torch.randint(0, C, (P,), generator=gen)
    labels[torch.rand(P, generator=gen) < 0.1] = IGNORE
    labels = labels.to(dev)
    weight = (torch.rand(C, generator=gen) + 0.5).to(dev)
    probas = F.softmax(logits.detach(), -1).requires_grad_(True)
    out = {"P": P, "C": C}

    # --- NLL ---------------------------------------------------------------------------------------------------
    def nll_ours():
        logits.grad = None
        _, loss = ops.log_softmax_nll(logits, labels, weight, IGNORE)
        loss.backward()
        return loss

    def nll_torch():
        logits.grad = None
        loss = F.nll_loss(F.log_softmax(logits, dim=-1), labels, weight=weight, ignore_index=IGNORE)
        loss.backward()
        return loss

    a = nll_ours(); ga = logits.grad.clone()
    b = nll_torch(); gb = logits.grad.clone()
    ours, theirs = alternate(nll_ours, nll_torch, reps, warmup)
    out["nll"] = {"device_ms": ours, "torch_ms": theirs, "speedup": round(theirs / ours, 2),
                  "agree": {"loss": rel(a, b), "grad": rel(ga, gb)}}

    # --- Lovasz ------------------------------------------------------------------------------------------------
    def lov_ours():
        probas.grad = None
        loss = ops.lovasz_softmax_flat(probas, labels, classes="present", ignore=IGNORE)
        loss.backward()
        return loss

    def lov_torch():
        probas.grad = None
        loss = GEN.lovasz_restated(probas, labels, "present", IGNORE, torch.float32)
        loss.backward()
        return loss

    a = lov_ours(); ga = probas.grad.clone()
    b = lov_torch(); gb = probas.grad.clone()
    ours, theirs = alternate(lov_ours, lov_torch, reps, warmup)
    # the torch side's gradient carries the fp32 Jaccard differences (its error grows with P); the loss is the check
    out["lovasz"] = {"device_ms": ours, "torch_ms": theirs, "speedup": round(theirs / ours, 2),
                     "agree": {"loss": rel(a, b), "grad": rel(ga, gb)}}

    # --- tracker -----------------------------------------------------------------------------------------------
    outputs = F.log_softmax(logits.detach(), -1)

    def tracker(n):
        return types.SimpleNamespace(_confusion_matrix=ConfusionMatrix(n), _num_classes=n, _ignore_label=IGNORE,
                                     _acc=0, _macc=0, _miou=0, _miou_per_class={})

    tr_dev, tr_host = tracker(C), tracker(C)

    def track_ours():
        compute_metrics(tr_dev, outputs, labels)

    def track_host():                                   # SegmentationTracker._compute_metrics, restated
        mask = labels != IGNORE
        o = outputs[mask].detach().cpu().numpy()
        l = labels[mask].detach().cpu().numpy()
        cm = tr_host._confusion_matrix
        cm.count_predicted_batch(l, np.argmax(o, 1))
        tr_host._acc = 100 * cm.get_overall_accuracy()
        tr_host._macc = 100 * cm.get_mean_class_accuracy()
        tr_host._miou = 100 * cm.get_average_intersection_union()
        tr_host._miou_per_class = {i: "{:.2f}".format(100 * v)
                                   for i, v in enumerate(cm.get_intersection_union_per_class()[0])}

    ours, theirs = alternate(track_ours, track_host, reps, warmup, host_clock=True)
    same = bool(np.array_equal(tr_dev._confusion_matrix.confusion_matrix, tr_host._confusion_matrix.confusion_matrix))
    out["tracker"] = {"device_ms": ours, "host_copy_ms": theirs, "speedup": round(theirs / ours, 2),
                      "agree": {"matrix_equal": same, "miou_equal": bool(tr_dev._miou == tr_host._miou)}}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "seg_loss_bench needs a HIP device"
    gen = torch.Generator().manual_seed(0)
    result = measure.header(
        "seg_loss_bench", reps=args.reps, warmup=args.warmup, host_cpu_threads=torch.get_num_threads(),
        timing="median ms of forward + backward, device events (tracker: host clock around a synchronised "
               "call), both sides alternating in one process",
        sizes=[run_size(P, C, args.reps, args.warmup, gen) for P, C in SIZES])
    result["kernel_sources_sha256"] = result["source_sha256"]               # the name earlier records carry
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
