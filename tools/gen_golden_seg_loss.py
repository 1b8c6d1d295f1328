#!/usr/bin/env python
"""Write tests/golden/seg_loss_*.npz by running the REFERENCE's own metrics/lovasz_loss.py and
metrics/confusion_matrix.py on the CPU.

TEST INFRASTRUCTURE: needs the reference source tree (argument 1, default ../reference next to this repository);
nothing in the package, smoke() or bench.py runs it; the tests read the committed .npz files and import the
restatements below (``lovasz_restated``, ``confusion_restated``) as their float64 yardstick.

The reference cannot run in float64 (its ``lovasz_grad`` calls ``.float()``), so the tool carries a restatement of the
loss with a ``dtype`` argument.  At float32 it is asserted ``torch.equal`` to the reference's loss and gradient on
every case; at float64 it is the yardstick.  Both go into the fixtures (``loss32`` / ``grad32`` from the reference,
``loss64`` / ``grad64`` from the restatement; gradients are with respect to the full ``probas``, zero on ignored rows).

Cases (keys: probas, labels, ignore, classes, loss32, grad32, loss64, grad64, plus what a case adds):
  seg_loss_lovasz_p{P}_c{C}   order-exact inputs: every entry of probas is a multiple of 2^-12 and the errors within a
                              class are distinct (k / 4096, k from a permutation of 1 .. 4095), so float32 and float64
                              sort identically; about 10 % of the labels ignored.  P around the wave (63, 64, 65), around
                              one tile of the segmented pass (ops.LOVASZ_TILE - 1, + 0, + 1) and 3 tiles + 5.
  seg_loss_lovasz_full_p{P}_c{C}  the same with no label ignored, so that the number of valid points itself is 63, 64, 65,
                              one tile - 1, + 0, + 1 and exactly two tiles
  seg_loss_structure          small order-exact cloud with class 3 absent: 'present', 'all', a list, all labels the same
                              class, one valid point, entries with p == fg exactly
  seg_loss_ties               rows duplicated together with their labels (``group`` = the original row of every row):
                              tie groups exact in any precision and foreground-homogeneous
  seg_loss_saturated          errors exactly 0 and 1, foreground and background tied: only the loss is defined
  seg_loss_confusion          three batches of outputs / labels (tied maxima, a NaN row, ignored labels), the reference's
                              matrix after every batch and its metrics at the end

Usage:  python tools/gen_golden_seg_loss.py [REFERENCE_ROOT]
"""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MAX_KIB = 700
IGNORE = -1
TILE = 1024                     # ops.LOVASZ_TILE (asserted by the tests)
LOVASZ_CASES = [(1, 13), (63, 2), (64, 20), (65, 64), (TILE - 1, 13), (TILE, 20), (TILE + 1, 13), (3 * TILE + 5, 13)]
# no label ignored: the number of valid points V, which is what the segmented pass tiles, sits on the boundaries itself
FULL_CASES = [(63, 3), (64, 3), (65, 3), (TILE - 1, 2), (TILE, 3), (TILE + 1, 2), (2 * TILE, 2)]


# ---------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------
def lovasz_restated(probas, labels, classes="present", ignore=None, dtype=torch.float32):
    """Lovasz-softmax of ``probas`` [P, C] in ``dtype`` over the points whose label is not ``ignore``: per class taking
    part, the errors |fg - p_c| sorted descending, weighted by the increments of the Jaccard index along that order,
    averaged over the classes.  Differentiable with respect to ``probas``.  Zero points kept: ``probas[:0] * 0``."""
    keep = torch.ones_like(labels, dtype=torch.bool) if ignore is None else labels != ignore
    p, lab = probas[keep].to(dtype), labels[keep]
    if p.numel() == 0:
        return p * 0.
    n_classes = p.shape[1]
    wanted = range(n_classes) if isinstance(classes, str) else classes
    terms = []
    for c in wanted:
        fg = (lab == c).to(dtype)
        total_fg = fg.sum()
        if classes == "present" and total_fg == 0:
            continue
        err, order = torch.sort((fg - p[:, c]).abs(), 0, descending=True)
        fg_along = fg[order]
        jaccard = 1. - (total_fg - fg_along.cumsum(0)) / (total_fg + (1 - fg_along).cumsum(0))
        step = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        terms.append(torch.dot(err, step))
    if not terms:
        return 0
    if len(terms) == 1:
        return terms[0]
    acc = terms[0]
    for term in terms[1:]:
        acc = acc + term
    return acc / len(terms)


def loss_and_grad(fn, probas):
    """(loss, dloss / dprobas) of ``fn(probas)`` with the gradient in the dtype of ``probas``; zero when fn does not
    depend on it."""
    x = probas.clone().requires_grad_(True)
    loss = fn(x)
    if not torch.is_tensor(loss) or not loss.requires_grad or loss.numel() != 1:
        return torch.as_tensor(0. if not torch.is_tensor(loss) or loss.numel() != 1 else float(loss)), torch.zeros_like(probas)
    loss.backward()
    return loss.detach(), x.grad.detach()


def confusion_restated(outputs, labels, n, ignore):
    """The batch matrix of SegmentationTracker._compute_metrics: mask, np.argmax, np.bincount."""
    keep = labels != ignore
    pred = np.argmax(outputs[keep], 1)
    return np.bincount(n * labels[keep].astype(int) + pred, minlength=n * n).reshape(n, n)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def order_exact(gen, P, C, labels=None, ignored=0.1):
    """probas float32 [P, C], every entry a multiple of 2^-12, the errors within a class distinct; labels int64 [P]."""
    assert P <= 4095
    if labels is None:
        labels = torch.randint(0, C, (P,), generator=gen)
        if P >= 10:
            labels[torch.rand(P, generator=gen) < ignored] = IGNORE
    k = torch.stack([torch.randperm(4095, generator=gen)[:P] + 1 for _ in range(C)], 1).to(torch.float32) / 4096
    fg = labels[:, None] == torch.arange(C)[None, :]
    probas = torch.where(fg, 1 - k, k)
    assert torch.equal(probas * 4096, (probas * 4096).round())
    return probas.contiguous(), labels


def evaluate(ref, probas, labels, classes, ignore):
    """The four result arrays of a case; ``ref`` = the reference's module or None (then the float32 restatement, which
    main() asserts equal to the reference, stands in for it)."""
    r32 = lambda x: lovasz_restated(x, labels, classes, ignore, torch.float32)
    r64 = lambda x: lovasz_restated(x, labels, classes, ignore, torch.float64)
    loss32, grad32 = loss_and_grad(r32, probas)
    loss64, grad64 = loss_and_grad(r64, probas.double())
    if ref is not None:
        keep = labels != ignore
        if int(keep.sum()) == 1:        # the reference's flatten_probas drops the point axis of a single valid point
            def theirs(x):
                return ref.lovasz_softmax_flat(x[keep], labels[keep], classes=classes)
        else:
            def theirs(x):
                return ref.lovasz_softmax(x, labels, classes=classes, ignore=ignore)
        ref_loss, ref_grad = loss_and_grad(theirs, probas)
        assert torch.equal(ref_loss.float(), loss32.float()) and torch.equal(ref_grad, grad32), "restatement != reference"
        loss32, grad32 = ref_loss, ref_grad
    cls = classes if isinstance(classes, str) else ",".join(str(c) for c in classes)
    return dict(probas=probas, labels=labels, ignore=np.int64(ignore), classes=np.array(cls),
                loss32=loss32.float(), grad32=grad32.float(), loss64=loss64.double(), grad64=grad64.double())


def prefixed(prefix, d):
    return {f"{prefix}/{k}": v for k, v in d.items()}


def build(ref=None, ref_cm=None):
    """name -> dict of arrays, every fixture of this tool."""
    gen = torch.Generator().manual_seed(20240611)
    out = {}
    for P, C in LOVASZ_CASES:
        probas, labels = order_exact(gen, P, C)
        case = evaluate(ref, probas, labels, "present", IGNORE)
        case["tile"] = np.int64(TILE)
        out[f"seg_loss_lovasz_p{P}_c{C}"] = case
    full_gen = torch.Generator().manual_seed(20240612)
    for P, C in FULL_CASES:
        probas, labels = order_exact(full_gen, P, C, ignored=0.0)
        assert not bool((labels == IGNORE).any())
        case = evaluate(ref, probas, labels, "present", IGNORE)
        case["tile"] = np.int64(TILE)
        out[f"seg_loss_lovasz_full_p{P}_c{C}"] = case

    # structure: 40 points, 5 classes, class 3 absent
    P, C = 40, 5
    labels = torch.randint(0, C - 2, (P,), generator=gen)
    labels[labels == 2] = 4
    labels[::3] = 2
    labels[torch.rand(P, generator=gen) < 0.1] = IGNORE
    probas, labels = order_exact(gen, P, C, labels=labels)
    assert not bool((labels == 3).any())
    st = {}
    st.update(prefixed("present", evaluate(ref, probas, labels, "present", IGNORE)))
    st.update(prefixed("all", evaluate(ref, probas, labels, "all", IGNORE)))
    st.update(prefixed("list", evaluate(ref, probas, labels, [0, 3], IGNORE)))
    same = torch.full((P,), 2, dtype=torch.int64)
    st.update(prefixed("same", evaluate(ref, order_exact(gen, P, C, labels=same)[0], same, "present", IGNORE)))
    one = torch.full((P,), IGNORE, dtype=torch.int64)
    one[17] = 1
    st.update(prefixed("one", evaluate(ref, probas, one, "present", IGNORE)))
    exact = probas.clone()
    hit = torch.zeros(P, C, dtype=torch.bool)
    hit[5, 0] = hit[6, 2] = hit[11, int(labels[11]) if int(labels[11]) >= 0 else 0] = True
    fg = (labels[:, None] == torch.arange(C)[None, :]).float()
    exact[hit] = fg[hit]
    case = evaluate(ref, exact, labels, "all", IGNORE)
    case["hit"] = hit
    st.update(prefixed("exact", case))
    out["seg_loss_structure"] = st

    # ties: every row twice, with its label
    P, C = 150, 4
    probas, labels = order_exact(gen, P, C)
    group = torch.cat([torch.arange(P), torch.arange(P)])
    shuffle = torch.randperm(2 * P, generator=gen)
    group = group[shuffle]
    case = evaluate(ref, probas[group].contiguous(), labels[group], "present", IGNORE)
    case["group"] = group
    out["seg_loss_ties"] = case

    # saturated: probas in {0, 1}
    P, C = 130, 3
    labels = torch.randint(0, C, (P,), generator=gen)
    labels[torch.rand(P, generator=gen) < 0.1] = IGNORE
    probas = (torch.rand(P, C, generator=gen) < 0.5).float()
    out["seg_loss_saturated"] = evaluate(ref, probas, labels, "present", IGNORE)

    # confusion: three batches
    n = 13
    cm = {"n": np.int64(n), "ignore": np.int64(IGNORE)}
    their = ref_cm.ConfusionMatrix(n) if ref_cm is not None else None
    total = np.zeros((n, n), dtype=np.int64)
    for b, P in enumerate((300, 1, 257)):
        outputs = torch.randn(P, n, generator=gen)
        labels = torch.randint(0, n - 1, (P,), generator=gen)          # class 12 never labelled ...
        outputs[:, n - 1] = -10.                                        # ... and never predicted: a missing class
        if P > 10:
            labels[torch.rand(P, generator=gen) < 0.15] = IGNORE
            outputs[3, 4] = outputs[3, 9] = outputs[3].max() + 1       # tied maxima: the first wins
            outputs[4, :] = 0.25                                        # all equal
            outputs[7, 5] = float("nan")                                # a NaN is the maximum
            outputs[8, 2] = outputs[8, 6] = float("nan")                # the first NaN wins
            labels[3] = labels[4] = labels[7] = labels[8] = 1
        outputs, labels = outputs.numpy(), labels.numpy()
        batch = confusion_restated(outputs, labels, n, IGNORE)
        total = total + batch
        if their is not None:
            keep = labels != IGNORE
            their.count_predicted_batch(labels[keep], np.argmax(outputs[keep], 1))
            assert np.array_equal(their.confusion_matrix, total)
        cm[f"b{b}_outputs"], cm[f"b{b}_labels"], cm[f"b{b}_matrix"] = outputs, labels, total.copy()
    if their is None:
        from deepviewagg_amd.metrics.confusion_matrix import ConfusionMatrix
        their = ConfusionMatrix.create_from_matrix(total.copy())
    iou, existing = their.get_intersection_union_per_class()
    cm.update(acc=np.float64(their.get_overall_accuracy()), macc=np.float64(their.get_mean_class_accuracy()),
              miou=np.float64(their.get_average_intersection_union()),
              miou_missing_as_one=np.float64(their.get_average_intersection_union(missing_as_one=True)),
              iou=np.asarray(iou, dtype=np.float64), existing=np.asarray(existing), count_gt_1=np.int64(their.count_gt(1)),
              count_1_4=np.int64(their.get_count(1, 4)))
    out["seg_loss_confusion"] = cm
    return {name: {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
                   for k, v in arrays.items()} for name, arrays in out.items()}


def load_reference(ref_root):
    mods = []
    for name in ("lovasz_loss", "confusion_matrix"):
        path = os.path.join(ref_root, "torch_points3d", "metrics", name + ".py")
        spec = importlib.util.spec_from_file_location("reference_" + name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    from deepviewagg_amd import ops
    assert ops.LOVASZ_TILE == TILE, "the cases are sized by the tile of the segmented pass"
    ref, ref_cm = load_reference(ref_root)
    for name, arrays in build(ref, ref_cm).items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        kib = os.path.getsize(path) / 1024
        assert kib < MAX_KIB, (name, kib)
        note = ""
        if "loss64" in arrays:
            e = abs(float(arrays["loss32"]) - float(arrays["loss64"])) / max(abs(float(arrays["loss64"])), 1e-300)
            g = np.abs(arrays["grad32"] - arrays["grad64"]).max() / max(np.abs(arrays["grad64"]).max(), 1e-300)
            note = f"  reference fp32 vs float64: loss {e:.2e}  grad {g:.2e}"
        print(f"  {name}.npz  {kib:.1f} KiB{note}")


if __name__ == "__main__":
    main()
