"""The segmentation tail on the device (csrc/segloss.hip through ops.log_softmax_nll / lovasz_softmax_flat /
confusion_counts and deepviewagg_amd.metrics) against float64 and the reference's fixtures tests/golden/seg_loss_*.npz.

Gates: ``tolerances.gate("out" | "grad_in", e32)`` with e32 = the error of the reference's own fp32 evaluation of the
same case against float64 -- the class gate, or 4 x the reference's error, never more.  Tie order inside a class is
ours (stable, ascending point index) and torch's is unspecified, so only tie-invariant quantities are compared.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden
from tolerances import Report, rel_err
from deepviewagg_amd import ops
from deepviewagg_amd.metrics import lovasz_loss as LL
from deepviewagg_amd.metrics.confusion_matrix import ConfusionMatrix
from deepviewagg_amd.metrics.losses import segmentation_loss
from deepviewagg_amd.metrics.segmentation_tracker import compute_metrics

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_seg_loss as GEN  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IGNORE = -1


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _classes(g, prefix=""):
    s = str(g[prefix + "classes"])
    return s if s in ("present", "all") else [int(c) for c in s.split(",")]


def _device_lovasz(g, prefix="", fn=None):
    probas = _t(g[prefix + "probas"]).to(DEV).requires_grad_(True)
    labels = _t(g[prefix + "labels"]).to(DEV)
    loss = (fn or LL.lovasz_softmax)(probas, labels, classes=_classes(g, prefix), ignore=int(g[prefix + "ignore"]))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    loss.backward()
    return loss.detach().cpu(), probas.grad.cpu()


def _add_lovasz_rows(rep, case, g, prefix, loss, grad):
    loss64, grad64 = _t(g[prefix + "loss64"]), _t(g[prefix + "grad64"])
    e_loss = rel_err(_t(g[prefix + "loss32"]), loss64)
    e_grad = rel_err(_t(g[prefix + "grad32"]), grad64)
    rep.add(case, "loss_lovasz", "out", rel_err(loss, loss64), e_loss)
    rep.add(case, "dloss/dprobas", "grad_in", rel_err(grad, grad64), e_grad)


def test_lovasz_order_exact_inputs_meet_the_float64_gates():
    """P around the wave, around one tile of the segmented pass and across three tiles (block carry); C = 2 .. 64."""
    tile = ops.LOVASZ_TILE
    assert tile == GEN.TILE
    cases = [(1, 13), (63, 2), (64, 20), (65, 64), (tile - 1, 13), (tile, 20), (tile + 1, 13), (3 * tile + 5, 13)]
    assert cases == GEN.LOVASZ_CASES
    rep = Report("Lovasz-softmax, order-exact inputs: device vs float64 (fp32 column: the reference's own error)")
    for P, C in cases:
        g = load_golden(f"seg_loss_lovasz_p{P}_c{C}")
        loss, grad = _device_lovasz(g)
        ignored = _t(g["labels"]) == IGNORE
        assert not bool(grad[ignored].any())                    # ignored points get no gradient
        _add_lovasz_rows(rep, f"P={P} C={C}", g, "", loss, grad)
    # no label ignored: the number of valid points, which the pass tiles, is itself 63 / 64 / 65, tile - 1 / + 0 / + 1
    # and exactly two tiles
    full = [(63, 3), (64, 3), (65, 3), (tile - 1, 2), (tile, 3), (tile + 1, 2), (2 * tile, 2)]
    assert full == GEN.FULL_CASES
    for P, C in full:
        g = load_golden(f"seg_loss_lovasz_full_p{P}_c{C}")
        assert int((_t(g["labels"]) != IGNORE).sum()) == P
        loss, grad = _device_lovasz(g)
        _add_lovasz_rows(rep, f"V=P={P} C={C}", g, "", loss, grad)
    rep.check()


def test_wrappers_refuse_shapes_beyond_the_kernels_limits():
    """C > 64 and P C >= 2^31 raise a ValueError that names the limit, before any launch (expanded views: no memory)."""
    one, lab = torch.zeros(1, 1, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    wide = (one.expand(1, 65), lab)
    huge = (one.expand(1 << 26, 32), lab.expand(1 << 26))
    for scores, labels in (wide, huge):
        match = "1 <= C <= 64" if scores.shape[1] == 65 else "fewer than 2\\^31"
        with pytest.raises(ValueError, match=match):
            ops.log_softmax_nll(scores, labels)
        with pytest.raises(ValueError, match=match):
            ops.lovasz_softmax_flat(scores, labels)
        with pytest.raises(ValueError, match=match):
            ops.confusion_counts(scores, labels, scores.shape[1])


def test_lovasz_structure_cases():
    g = load_golden("seg_loss_structure")
    rep = Report("Lovasz-softmax, structure cases: device vs float64")
    for name in ("present", "all", "list", "same", "one", "exact"):
        loss, grad = _device_lovasz(g, name + "/")
        _add_lovasz_rows(rep, name, g, name + "/", loss, grad)
        if name == "present":
            assert not bool(grad[:, 3].any())                   # the absent class takes no part
        if name == "all":
            assert bool(grad[:, 3].any())                       # ... and does under 'all'
        if name == "list":
            assert not bool(grad[:, [1, 2, 4]].any())
        if name == "exact":
            hit = _t(g["exact/hit"])
            assert int(hit.sum()) == 3 and not bool(grad[hit].any())        # abs'(0) = 0
    rep.check()
    # one valid point: the float64 restatement, evaluated here (the reference raises IndexError on it)
    probas, labels = _t(g["one/probas"]), _t(g["one/labels"])
    assert int((labels != IGNORE).sum()) == 1
    want = GEN.lovasz_restated(probas.double(), labels, "present", IGNORE, torch.float64)
    assert rel_err(_device_lovasz(g, "one/")[0], want) <= 1e-6


def test_lovasz_all_labels_ignored():
    probas = torch.rand(70, 5, device=DEV, requires_grad=True)
    labels = torch.full((70,), IGNORE, device=DEV)
    out = LL.lovasz_softmax(probas, labels, ignore=IGNORE)
    assert tuple(out.shape) == (0, 5)                           # the reference's shape quirk
    loss = ops.lovasz_softmax_flat(probas, labels, ignore=IGNORE)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not bool(probas.grad.any())


def test_lovasz_ties():
    g = load_golden("seg_loss_ties")
    rep = Report("Lovasz-softmax, duplicated rows: loss and per-tie-group sorted gradients vs float64")
    loss, grad = _device_lovasz(g)
    loss64 = _t(g["loss64"])
    rep.add("ties", "loss_lovasz", "out", rel_err(loss, loss64), rel_err(_t(g["loss32"]), loss64))
    order = torch.argsort(_t(g["group"]), stable=True)
    P2, C = grad.shape

    def grouped(x):                                             # [P, 2, C], the two rows of a group sorted by value
        return x[order].reshape(P2 // 2, 2, C).sort(dim=1).values

    grad64 = grouped(_t(g["grad64"]))
    rep.add("ties", "sorted dloss/dprobas per group", "grad_in", rel_err(grouped(grad), grad64),
            rel_err(grouped(_t(g["grad32"])), grad64))
    s = load_golden("seg_loss_saturated")
    loss, _ = _device_lovasz(s)
    rep.add("saturated", "loss_lovasz", "out", rel_err(loss, _t(s["loss64"])), rel_err(_t(s["loss32"]), _t(s["loss64"])))
    rep.check()


def test_lovasz_loss_across_more_tiles_than_one_prefix_chunk():
    """257 tiles + 3 valid points per class: the exclusive prefix of the per-tile counts runs over two chunks of 256
    tiles.  Entries are multiples of 2^-12, so errors tie massively across foreground and background: the loss, which
    does not depend on the tie order, is compared (a wrong carry moves it in the first digits)."""
    gen = torch.Generator().manual_seed(3)
    P, C = 257 * ops.LOVASZ_TILE + 3, 2
    probas = torch.randint(0, 4097, (P, C), generator=gen).float() / 4096
    labels = torch.randint(0, C, (P,), generator=gen)
    loss64 = GEN.lovasz_restated(probas.double(), labels, "present", None, torch.float64)
    loss32 = GEN.lovasz_restated(probas, labels, "present", None, torch.float32)
    loss = LL.lovasz_softmax(probas.to(DEV), labels.to(DEV), ignore=None)
    rep = Report("Lovasz-softmax over 257 tiles per class: loss vs float64")
    rep.add(f"P={P} C={C}", "loss_lovasz", "out", rel_err(loss.cpu(), loss64), rel_err(loss32, loss64))
    rep.check()


def _composition(x, labels, weight, up, dtype64):
    """The reference's composition in torch; x is the leaf."""
    z = x.to(dtype64)
    out = F.log_softmax(z, dim=-1)
    ce = F.nll_loss(out, labels, weight=weight.to(dtype64), ignore_index=IGNORE)
    lov = GEN.lovasz_restated(out.exp(), labels, "present", IGNORE, dtype64)
    total = ce + lov + (out * up.to(dtype64)).sum()
    total.backward()
    return out.detach(), ce.detach(), torch.as_tensor(lov).detach(), x.grad.detach()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_end_to_end_from_logits(dtype):
    """segmentation_loss with weights, ignored labels and an upstream gradient on ``output``, against float64 torch on
    the same rounded logits; e32 = the same composition on the CPU in float32 from logits of that dtype."""
    rep = Report(f"segmentation_loss from {dtype} logits: device vs float64")
    gen = torch.Generator().manual_seed(77)
    for P in (1, 65, 1029):
        for C in (13, 20):
            logits = (2 * torch.randn(P, C, generator=gen)).to(dtype)
            labels = torch.randint(0, C, (P,), generator=gen)
            if P > 1:
                labels[torch.rand(P, generator=gen) < 0.15] = IGNORE
            weight = torch.rand(C, generator=gen) + 0.5
            up = torch.randn(P, C, generator=gen) / P
            out64, ce64, lov64, grad64 = _composition(logits.double().requires_grad_(True), labels, weight, up,
                                                      torch.float64)
            out32, ce32, lov32, grad32 = _composition(logits.clone().requires_grad_(True), labels, weight, up,
                                                      torch.float32)
            assert grad32.dtype == dtype
            x = logits.to(DEV).requires_grad_(True)
            output, loss_seg, ce, lov = segmentation_loss(x, labels.to(DEV), weight.to(DEV), True, True)
            assert output.dtype == torch.float32 and ce.dim() == 0 and lov.dim() == 0
            assert torch.equal(loss_seg, ce + lov)
            (loss_seg + (output * up.to(DEV)).sum()).backward()
            assert x.grad.dtype == dtype
            case = f"P={P} C={C}"
            rep.add(case, "output (log-probs)", "out", rel_err(output.cpu(), out64), rel_err(out32, out64))
            rep.add(case, "loss_cross_entropy", "out", rel_err(ce.cpu(), ce64), rel_err(ce32, ce64))
            rep.add(case, "loss_lovasz", "out", rel_err(lov.cpu(), lov64), rel_err(lov32, lov64))
            rep.add(case, "dloss/dlogits", "grad_in", rel_err(x.grad.cpu(), grad64), rel_err(grad32, grad64))
    rep.check()


def test_nll_is_nan_when_every_label_is_ignored():
    x = torch.randn(33, 13, device=DEV, requires_grad=True)
    labels = torch.full((33,), IGNORE, device=DEV)
    output, loss_seg, ce, lov = segmentation_loss(x, labels, None, True, False)
    assert lov is None and bool(torch.isnan(ce)) and bool(torch.isnan(loss_seg))
    assert rel_err(output.cpu(), F.log_softmax(x.detach().cpu().double(), -1)) <= 1e-6
    want = F.nll_loss(F.log_softmax(x.detach().cpu(), -1), labels.cpu(), ignore_index=IGNORE)
    assert bool(torch.isnan(want))                              # as torch


def _fake_tracker(n):
    return types.SimpleNamespace(_confusion_matrix=ConfusionMatrix(n), _num_classes=n, _ignore_label=IGNORE,
                                 _acc=0, _macc=0, _miou=0, _miou_per_class={})


def test_confusion_counts_equal_the_reference_matrices():
    g = load_golden("seg_loss_confusion")
    n = int(g["n"])
    cm, tracker = ConfusionMatrix(n), _fake_tracker(n)
    for b in range(3):                                          # accumulation over three calls
        outputs, labels = _t(g[f"b{b}_outputs"]).to(DEV), _t(g[f"b{b}_labels"]).to(DEV)
        cm.count_outputs(outputs, labels, IGNORE)
        compute_metrics(tracker, outputs, labels)
        assert cm._dev is not None and cm._dev.is_cuda          # still on the device
        assert np.array_equal(cm.confusion_matrix, g[f"b{b}_matrix"])
        assert cm.confusion_matrix.dtype == np.int64
        assert np.array_equal(tracker._confusion_matrix.confusion_matrix, g[f"b{b}_matrix"])
    m = g["b0_matrix"]
    assert m[1, 4] >= 1 and m[1, 0] >= 1 and m[1, 5] >= 1 and m[1, 2] >= 1     # tied maxima, all equal, NaN rows
    assert cm.get_overall_accuracy() == float(g["acc"]) and cm.get_mean_class_accuracy() == float(g["macc"])
    assert cm.get_average_intersection_union() == float(g["miou"])
    assert cm.get_average_intersection_union(missing_as_one=True) == float(g["miou_missing_as_one"])
    iou, existing = cm.get_intersection_union_per_class()
    assert np.array_equal(iou, g["iou"]) and np.array_equal(existing, g["existing"])
    assert int(cm.count_gt(1)) == int(g["count_gt_1"]) and int(cm.get_count(1, 4)) == int(g["count_1_4"])
    assert tracker._acc == 100 * float(g["acc"]) and tracker._macc == 100 * float(g["macc"])
    assert tracker._miou == 100 * float(g["miou"])
    assert tracker._miou_per_class == {i: "{:.2f}".format(100 * v) for i, v in enumerate(g["iou"])}
    # predictions already on the device go through count_predicted_batch
    dev_cm = ConfusionMatrix(n)
    labels = _t(g["b0_labels"])
    keep = labels != IGNORE
    pred = _t(np.argmax(g["b0_outputs"][keep.numpy()], 1))
    dev_cm.count_predicted_batch(labels[keep].to(DEV), pred.to(DEV))
    assert np.array_equal(dev_cm.confusion_matrix, g["b0_matrix"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_confusion_counts_half_precision_and_many_blocks(dtype):
    gen = torch.Generator().manual_seed(5)
    P, C = 70001, 20
    outputs = torch.randn(P, C, generator=gen).to(dtype)        # rounding makes tied maxima common
    labels = torch.randint(-1, C, (P,), generator=gen)
    want = GEN.confusion_restated(outputs.float().numpy(), labels.numpy(), C, IGNORE)
    counts, n_bad = ops.confusion_counts(outputs.to(DEV), labels.to(DEV), C, ignore_index=IGNORE)
    assert counts.dtype == torch.int64 and counts.is_cuda and n_bad.is_cuda
    assert np.array_equal(counts.cpu().numpy(), want) and int(n_bad) == 0


def test_confusion_out_of_range_label_raises_on_read():
    cm = ConfusionMatrix(5)
    outputs = torch.randn(40, 5, device=DEV)
    labels = torch.randint(0, 5, (40,), device=DEV)
    labels[7], labels[9], labels[11] = 5, -2, IGNORE
    cm.count_outputs(outputs, labels, IGNORE)                   # no error yet: nothing was read
    with pytest.raises(ValueError, match="2 counted rows"):
        cm.confusion_matrix
    with pytest.raises(ValueError, match="2 counted rows"):        # the counts stay pending: it keeps raising
        cm.get_overall_accuracy()
    assert cm._dev is not None
    cm.confusion_matrix = None                                      # until the caller resets
    assert cm.confusion_matrix is None
    counts, n_bad = ops.confusion_counts(outputs, labels, 5, ignore_index=IGNORE)
    assert int(n_bad) == 2 and int(counts.sum()) == 37
    # predictions on the device: a bad label or a bad prediction is refused as on the host, but on read
    pairs = ConfusionMatrix(5)
    pairs.count_predicted_batch(torch.tensor([0, 5, 1, 2], device=DEV), torch.tensor([0, 1, -1, 2], device=DEV))
    with pytest.raises(ValueError, match="2 counted rows"):
        pairs.confusion_matrix


def test_tracker_step_leaves_the_metrics_alone_when_every_label_is_ignored():
    tracker = _fake_tracker(5)
    outputs = torch.randn(40, 5, device=DEV)
    compute_metrics(tracker, outputs, torch.full((40,), IGNORE, device=DEV))
    assert tracker._miou_per_class == {} and tracker._acc == 0              # as the reference: it returns early
    labels = torch.randint(0, 5, (40,), device=DEV)
    compute_metrics(tracker, outputs, labels)
    seen = dict(tracker._miou_per_class)
    assert len(seen) == 5 and int(tracker._confusion_matrix.confusion_matrix.sum()) == 40
    compute_metrics(tracker, outputs, torch.full((40,), IGNORE, device=DEV))
    assert tracker._miou_per_class == seen and int(tracker._confusion_matrix.confusion_matrix.sum()) == 40


def _run_all_ops(x, labels, weight, up, cm):
    x.grad = None
    output, loss_seg, ce, lov = segmentation_loss(x, labels, weight, True, True)
    lov_list = ops.lovasz_softmax_flat(output.exp(), labels, classes=[0, 2], ignore=IGNORE)
    (loss_seg + lov_list + (output * up).sum()).backward()
    cm.count_outputs(output, labels, IGNORE)
    return output.detach(), ce.detach(), lov.detach(), lov_list.detach(), x.grad.clone(), cm._dev.clone()


def test_two_runs_give_identical_bits():
    gen = torch.Generator().manual_seed(11)
    P, C = 2 * ops.LOVASZ_TILE + 77, 13
    x = (2 * torch.randn(P, C, generator=gen)).to(DEV).requires_grad_(True)
    labels = torch.randint(-1, C, (P,), generator=gen).to(DEV)
    weight = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    up = (torch.randn(P, C, generator=gen) / P).to(DEV)
    first = _run_all_ops(x, labels, weight, up, ConfusionMatrix(C))
    second = _run_all_ops(x, labels, weight, up, ConfusionMatrix(C))
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def test_no_host_synchronisation():
    gen = torch.Generator().manual_seed(12)
    P, C = ops.LOVASZ_TILE + 9, 13
    x = (2 * torch.randn(P, C, generator=gen)).to(DEV).requires_grad_(True)
    labels = torch.randint(-1, C, (P,), generator=gen).to(DEV)
    weight = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    up = (torch.randn(P, C, generator=gen) / P).to(DEV)
    cm = ConfusionMatrix(C)
    _run_all_ops(x, labels, weight, up, cm)                     # warm: library load, allocator
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        live = False
        try:
            labels[0].item()                                    # a deliberate synchronisation: the mode must object
        except RuntimeError:
            live = True
        if not live:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not intercept .item() on this build")
        _run_all_ops(x, labels, weight, up, cm)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    torch.cuda.synchronize()
    assert int(cm.confusion_matrix.sum()) == 2 * int((labels != IGNORE).sum())
