"""The segmentation tail without a GPU: the C-ABI argument checks of the dva_seg_* / dva_confusion_* / dva_lovasz_*
entries, the host paths of deepviewagg_amd.metrics, the drop-in names, and the committed fixtures
tests/golden/seg_loss_*.npz (tools/gen_golden_seg_loss.py)."""
import glob
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden
from deepviewagg_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_seg_loss as GEN  # noqa: E402


def test_abi_entries_reject_bad_arguments():
    lib = _lib.load()
    assert lib.dva_version() >= 314
    one, big = 1, 1 << 40
    F32 = _lib.DVA_F32
    assert lib.dva_seg_nll_workspace_bytes() >= 2 * 8
    fwd = lib.dva_seg_logsoftmax_nll_fwd
    assert fwd(None, F32, one, None, -1, 10, 13, one, one, one, one, big, None) == -1       # logits
    assert fwd(one, F32, None, None, -1, 10, 13, one, one, one, one, big, None) == -1       # labels
    assert fwd(one, F32, one, None, -1, 10, 13, None, one, one, one, big, None) == -1       # log_probs
    assert fwd(one, F32, one, None, -1, 10, 13, one, None, one, one, big, None) == -1       # loss
    assert fwd(one, F32, one, None, -1, 10, 13, one, one, None, one, big, None) == -1       # numden
    assert fwd(one, F32, one, None, -1, 10, 13, one, one, one, None, big, None) == -1       # workspace
    assert fwd(one, F32, one, None, -1, 10, 13, one, one, one, one, 8, None) == -1          # workspace size
    assert fwd(one, 7, one, None, -1, 10, 13, one, one, one, one, big, None) == -1          # dtype
    assert fwd(one, F32, one, None, -1, -1, 13, one, one, one, one, big, None) == -1
    assert fwd(one, F32, one, None, -1, 10, 0, one, one, one, one, big, None) == -1         # C = 0
    assert fwd(one, F32, one, None, -1, 10, 65, one, one, one, one, big, None) == -2        # C = 65
    assert fwd(one, F32, one, None, -1, 1 << 27, 16, one, one, one, one, big, None) == -2   # P C = 2^31
    bwd = lib.dva_seg_logsoftmax_nll_bwd
    assert bwd(None, one, None, one, one, None, -1, 10, 13, one, F32, None) == -1
    assert bwd(one, None, None, one, one, None, -1, 10, 13, one, F32, None) == -1
    assert bwd(one, one, None, None, one, None, -1, 10, 13, one, F32, None) == -1
    assert bwd(one, one, None, one, one, None, -1, 10, 13, None, F32, None) == -1
    assert bwd(one, one, None, one, one, None, -1, 10, 13, one, 3, None) == -1
    assert bwd(one, one, None, one, one, None, -1, 10, 0, one, F32, None) == -1
    assert bwd(one, one, None, one, one, None, -1, 10, 65, one, F32, None) == -2
    assert bwd(one, one, None, one, one, None, -1, 1 << 25, 64, one, F32, None) == -2
    conf = lib.dva_confusion_counts
    assert conf(None, F32, one, -1, 10, 13, one, one, None) == -1
    assert conf(one, F32, None, -1, 10, 13, one, one, None) == -1
    assert conf(one, F32, one, -1, 10, 13, None, one, None) == -1
    assert conf(one, F32, one, -1, 10, 13, one, None, None) == -1
    assert conf(one, 9, one, -1, 10, 13, one, one, None) == -1
    assert conf(one, F32, one, -1, 10, 0, one, one, None) == -1
    assert conf(one, F32, one, -1, 10, 65, one, one, None) == -2
    assert conf(one, F32, one, -1, 1 << 30, 2, one, one, None) == -2
    assert conf(None, F32, None, -1, 0, 13, one, one, None) == 0                            # no rows: nothing to do
    assert lib.dva_lovasz_workspace_bytes(-1, 13) == -1
    assert lib.dva_lovasz_workspace_bytes(10, 0) == -1
    assert lib.dva_lovasz_workspace_bytes(10, 65) == -2
    assert lib.dva_lovasz_workspace_bytes(1 << 27, 16) == -2
    lov = lib.dva_lovasz_softmax
    assert lov(None, one, 10, 13, -1, 1, None, 1, one, one, one, big, None) == -1
    assert lov(one, None, 10, 13, -1, 1, None, 1, one, one, one, big, None) == -1
    assert lov(one, one, 10, 13, -1, 1, None, 1, None, one, one, big, None) == -1
    assert lov(one, one, 10, 13, -1, 1, None, 1, one, None, one, big, None) == -1
    assert lov(one, one, 10, 13, -1, 1, None, 1, one, one, None, big, None) == -1
    assert lov(one, one, 10, 0, -1, 1, None, 1, one, one, one, big, None) == -1
    assert lov(one, one, 10, 65, -1, 1, None, 1, one, one, one, big, None) == -2
    assert lov(one, one, 1 << 27, 16, -1, 1, None, 1, one, one, one, big, None) == -2
    assert lov(one, one, -1, 13, -1, 1, None, 1, one, one, one, big, None) == -1


def test_ops_reject_bad_arguments_before_any_device_work():
    from deepviewagg_amd import ops
    assert ops.LOVASZ_TILE == _lib.load().dva_lovasz_tile() == GEN.TILE
    x, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    for call in (lambda: ops.log_softmax_nll(x, y), lambda: ops.lovasz_softmax_flat(x, y),
                 lambda: ops.confusion_counts(x, y, 3)):
        with pytest.raises(_lib.DvaError, match="HIP device only"):          # the require_device policy
            call()


def test_confusion_matrix_host_path_equals_the_reference_values():
    from deepviewagg_amd.metrics.confusion_matrix import ConfusionMatrix
    g = load_golden("seg_loss_confusion")
    n, ignore = int(g["n"]), int(g["ignore"])
    cm = ConfusionMatrix(n)
    assert cm.confusion_matrix is None
    for b in range(3):
        outputs, labels = g[f"b{b}_outputs"], g[f"b{b}_labels"]
        keep = labels != ignore
        pred = np.argmax(outputs[keep], 1)
        if b == 1:                                              # CPU tensors take the host path too
            cm.count_predicted_batch(torch.from_numpy(labels[keep]), torch.from_numpy(pred))
        else:
            cm.count_predicted_batch(labels[keep], pred)
        assert np.array_equal(cm.confusion_matrix, g[f"b{b}_matrix"])
        assert np.array_equal(cm.get_confusion_matrix(), g[f"b{b}_matrix"])
    _check_metrics(cm, g)
    again = ConfusionMatrix.create_from_matrix(g["b2_matrix"].copy())
    assert again.number_of_labels == n
    _check_metrics(again, g)
    # a label or a prediction outside [0, n) is refused whole, on either side of the pair, and counts nothing
    for gt, pred in (([0, n], [0, 1]), ([0, -2], [0, 1]), ([0, 1], [0, n]), ([0, 1], [-1, 1])):
        with pytest.raises(ValueError, match=f"1 pairs .* outside \\[0, {n}\\)"):
            cm.count_predicted_batch(np.array(gt), np.array(pred))
    assert np.array_equal(cm.confusion_matrix, g["b2_matrix"])


def _check_metrics(cm, g):
    assert cm.get_overall_accuracy() == float(g["acc"])
    assert cm.get_mean_class_accuracy() == float(g["macc"])
    assert cm.get_average_intersection_union() == float(g["miou"])
    assert cm.get_average_intersection_union(missing_as_one=True) == float(g["miou_missing_as_one"])
    iou, existing = cm.get_intersection_union_per_class()
    assert np.array_equal(iou, g["iou"]) and np.array_equal(existing, g["existing"])
    assert not existing[12] and existing[:12].all()             # class 12 is never labelled and never predicted
    assert int(cm.count_gt(1)) == int(g["count_gt_1"]) and int(cm.get_count(1, 4)) == int(g["count_1_4"])


def test_per_image_raises_and_host_quirks():
    from deepviewagg_amd.metrics import lovasz_loss as L
    with pytest.raises(NotImplementedError, match="per_image"):
        L.lovasz_softmax(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), per_image=True)
    out = L.lovasz_softmax(torch.rand(4, 3), torch.full((4,), -1), ignore=-1)        # every point ignored
    assert tuple(out.shape) == (0, 3)
    assert tuple(L.lovasz_softmax_flat(torch.zeros(0, 3), torch.zeros(0, dtype=torch.int64)).shape) == (0, 3)
    from deepviewagg_amd.metrics.losses import segmentation_loss
    with pytest.raises(AssertionError, match="at least one"):
        segmentation_loss(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), use_cross_entropy=False)


def _clear():
    for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
        del sys.modules[k]


@pytest.mark.parametrize("patch_existing", [False, True])
def test_dropin_aliases_resolve(patch_existing):
    from deepviewagg_amd import dropin
    from deepviewagg_amd.metrics import confusion_matrix as CM, lovasz_loss as LL
    _clear()
    try:
        names = dropin.install(patch_existing=patch_existing)
        assert "torch_points3d.metrics.lovasz_loss" in names and "torch_points3d.metrics.confusion_matrix" in names
        assert importlib.import_module("torch_points3d.metrics.lovasz_loss").lovasz_softmax is LL.lovasz_softmax
        assert importlib.import_module("torch_points3d.metrics.confusion_matrix").ConfusionMatrix is CM.ConfusionMatrix
        from torch_points3d.metrics.lovasz_loss import lovasz_softmax       # the model file's own import line
        assert lovasz_softmax is LL.lovasz_softmax
    finally:
        _clear()


def test_dropin_binds_the_tracker_step_when_the_tracker_is_importable():
    import types
    from deepviewagg_amd import dropin
    from deepviewagg_amd.metrics.confusion_matrix import ConfusionMatrix
    from deepviewagg_amd.metrics.segmentation_tracker import compute_metrics
    _clear()
    try:
        for name in ("torch_points3d", "torch_points3d.metrics"):
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
        theirs = types.ModuleType("torch_points3d.metrics.segmentation_tracker")

        class SegmentationTracker:
            def _compute_metrics(self, outputs, labels):
                raise AssertionError("the host path")

        theirs.SegmentationTracker, theirs.ConfusionMatrix = SegmentationTracker, object
        sys.modules[theirs.__name__] = theirs
        dropin.install(patch_existing=True)
        assert SegmentationTracker._compute_metrics is compute_metrics and theirs.ConfusionMatrix is ConfusionMatrix
    finally:
        _clear()


def test_fixtures_are_what_the_tool_writes():
    """The inputs, integer results and the float64 yardstick regenerate from the tool's seed.  Without the reference's
    source the tool's float32 restatement stands in for it (the tool asserts the two torch.equal when it writes the
    files).  Integers and inputs are compared exactly; float results to a few ulp of their format, because the host's
    dot product may sum in another order on another CPU."""
    files = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "seg_loss_*.npz")))
    built = GEN.build()
    assert files == sorted(built)
    for name in files:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < GEN.MAX_KIB * 1024, name
        g = load_golden(name)
        assert sorted(g) == sorted(built[name]), name
        for k, v in g.items():
            w = built[name][k]
            assert v.dtype == w.dtype and v.shape == w.shape and v.dtype.kind in "fiubU", (name, k, v.dtype, w.dtype)
            leaf = k.split("/")[-1]
            if leaf in ("loss32", "grad32", "loss64", "grad64"):
                tol = 4 * np.finfo(v.dtype).eps
                scale = max(float(np.abs(v).max()) if v.size else 0.0, 1e-30)
                assert float(np.abs(v.astype(np.float64) - w).max()) <= tol * scale if v.size else True, (name, k)
            elif v.dtype.kind == "f":
                assert v.tobytes() == w.tobytes() or np.array_equal(v, w, equal_nan=True), (name, k)
            else:
                assert np.array_equal(v, w), (name, k)


def test_order_exact_fixtures_are_order_exact():
    """Every entry a multiple of 2^-12, the errors within a class distinct: float32 and float64 sort identically."""
    for full, (P, C) in [(False, pc) for pc in GEN.LOVASZ_CASES] + [(True, pc) for pc in GEN.FULL_CASES]:
        g = load_golden(f"seg_loss_lovasz_{'full_' if full else ''}p{P}_c{C}")
        assert int(g["tile"]) == GEN.TILE and g["probas"].shape == (P, C) and g["probas"].dtype == np.float32
        k = g["probas"].astype(np.float64) * 4096
        assert np.array_equal(k, np.round(k))
        fg = g["labels"][:, None] == np.arange(C)[None, :]
        err = np.abs(fg - g["probas"].astype(np.float64))[g["labels"] != int(g["ignore"])]
        assert np.array_equal(err, np.abs(fg.astype(np.float32) - g["probas"])[g["labels"] != int(g["ignore"])])
        for c in range(C):
            assert np.unique(err[:, c]).size == err.shape[0], (P, C, c)
        n_ignored = int((g["labels"] == int(g["ignore"])).sum())
        if full:                                                # the valid points themselves sit on the boundaries
            assert n_ignored == 0
        elif P >= 63:
            assert 0 < n_ignored < P // 4


def test_integer_count_increments_equal_the_float64_yardstick():
    """The arithmetic csrc/segloss.hip implements, restated in numpy: J_k = 1 - (G - n_k) / (G + k - n_k) from integer
    counts in float64 along the stable descending order, grad = sign(p - fg) (J_k - J_{k-1}) / n_used."""
    g = load_golden(f"seg_loss_lovasz_p{GEN.TILE + 1}_c13")
    probas, labels = g["probas"], g["labels"]
    keep = labels != int(g["ignore"])
    rows = np.nonzero(keep)[0]
    C = probas.shape[1]
    used = [c for c in range(C) if (labels[keep] == c).any()]
    grad, loss = np.zeros(probas.shape, dtype=np.float64), 0.0
    for c in used:
        fg = (labels[rows] == c)
        p = probas[rows, c]
        err = np.abs(fg.astype(np.float32) - p)
        order = np.argsort(-err.astype(np.float64), kind="stable")
        n = np.cumsum(fg[order]).astype(np.float64)
        k = np.arange(1, len(order) + 1, dtype=np.float64)
        G = float(fg.sum())
        J = 1.0 - (G - n) / (G + k - n)
        step = np.diff(np.concatenate([[0.0], J]))
        loss += float((err[order].astype(np.float64) * step).sum())
        grad[rows[order], c] = np.sign(p[order].astype(np.float64) - fg[order]) * step / len(used)
    loss /= len(used)
    assert abs(loss - float(g["loss64"])) <= 1e-13 * abs(float(g["loss64"]))
    assert np.abs(grad - g["grad64"]).max() <= 1e-12 * np.abs(g["grad64"]).max()
