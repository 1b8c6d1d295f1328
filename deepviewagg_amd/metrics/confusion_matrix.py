"""ConfusionMatrix of the reference (metrics/confusion_matrix.py) whose counts can stay on the device.

``count_outputs`` takes the model's [P, C] outputs and the labels as they are on the device (mask, argmax and count
in one kernel, ``ops.confusion_counts``); the matrix moves to the host, C x C integers, only when a metric or
``.confusion_matrix`` is read.  The metrics are computed from the host matrix with the reference's formulas.
"""
import numpy as np
import torch

from .. import ops

__all__ = ["ConfusionMatrix"]


class ConfusionMatrix:
    """Counts (label, predicted class) pairs batch by batch; the matrix and the metrics are read at any time.
    ``confusion_matrix[label, predicted]`` = number of samples of class ``label`` reported as ``predicted``."""

    def __init__(self, number_of_labels=2):
        self.number_of_labels = number_of_labels
        self._host = None           # numpy int [C, C], or whatever create_from_matrix was given
        self._dev = None            # int64 [C, C] on the device: counts not yet added to _host
        self._bad = None            # int64 [1] on the device: rows with a label outside [0, C)

    @staticmethod
    def create_from_matrix(confusion_matrix):
        rows, cols = confusion_matrix.shape
        assert rows == cols, "a confusion matrix is square"
        out = ConfusionMatrix(rows)
        out._host = confusion_matrix
        return out

    # the reference's public attribute; reading it brings the device counts home
    @property
    def confusion_matrix(self):
        if self._dev is not None:
            n_bad = int(self._bad.item())
            if n_bad != 0:          # the device counts stay pending: every read raises until the caller resets
                raise ValueError(f"ConfusionMatrix: {n_bad} counted rows carry a label (other than the ignored "
                                 f"one) or a predicted class outside [0, {self.number_of_labels})")
            batch = self._dev.cpu().numpy()
            self._dev = self._bad = None
            self._host = batch if self._host is None else self._host + batch.astype(self._host.dtype, copy=False)
        return self._host

    @confusion_matrix.setter
    def confusion_matrix(self, value):
        self._host, self._dev, self._bad = value, None, None

    def count_predicted_batch(self, ground_truth_vec, predicted):
        """Counts a batch of (label, predicted class) pairs: numpy arrays or CPU tensors on the host, device tensors
        on the device.  Both branches take the same pairs: a label or a prediction outside [0, C) is a ValueError
        (the reference asserts on ``predicted >= C`` only and miscounts the rest).  The host branch raises at once and
        counts nothing of the batch; the device branch, which must not synchronise, counts the pairs in range and
        makes every later read of the matrix raise, as ``count_outputs`` does."""
        n = self.number_of_labels
        if torch.is_tensor(predicted) and predicted.is_cuda:
            gt = ground_truth_vec.to(predicted.device).reshape(-1).to(torch.int64)
            pred = predicted.reshape(-1).to(torch.int64)
            ok = (gt >= 0) & (gt < n) & (pred >= 0) & (pred < n)
            if self._dev is None:
                self._dev = torch.zeros((n, n), dtype=torch.int64, device=pred.device)
                self._bad = torch.zeros(1, dtype=torch.int64, device=pred.device)
            self._dev.view(-1).index_add_(0, torch.where(ok, n * gt + pred, torch.zeros_like(gt)), ok.to(torch.int64))
            self._bad += (~ok).sum()
            return
        gt, pred = (np.asarray(v.numpy() if torch.is_tensor(v) else v) for v in (ground_truth_vec, predicted))
        gt, pred = gt.reshape(-1).astype(np.int64), pred.reshape(-1).astype(np.int64)
        n_bad = int(((gt < 0) | (gt >= n) | (pred < 0) | (pred >= n)).sum())
        if n_bad != 0:
            raise ValueError(f"ConfusionMatrix: {n_bad} pairs carry a label or a predicted class outside [0, {n})")
        cell = gt * n + pred
        batch = np.bincount(cell, minlength=n * n).reshape(n, n)
        self._host = batch if self._host is None else self._host + batch

    def count_outputs(self, outputs, labels, ignore_label):
        """Counts ``argmax(outputs, 1)`` [P, C] against ``labels`` [P] over the rows whose label is not
        ``ignore_label``, on the device and without a host synchronisation.  A label outside [0, C) other than
        ``ignore_label`` makes every later read of the matrix raise."""
        if self._dev is None:
            self._dev = torch.zeros((self.number_of_labels,) * 2, dtype=torch.int64, device=outputs.device)
            self._bad = torch.zeros(1, dtype=torch.int64, device=outputs.device)
        _, n_bad = ops.confusion_counts(outputs, labels.reshape(-1), self.number_of_labels, ignore_index=ignore_label,
                                        out=self._dev)
        self._bad += n_bad

    def get_count(self, ground_truth, predicted):
        return self.confusion_matrix[ground_truth][predicted]

    def get_confusion_matrix(self):
        return self.confusion_matrix

    def get_intersection_union_per_class(self):
        """``(iou, existing)``: per class hits / (labelled + predicted - hits), regularised by 1e-8 in the quotient and
        on the result as the reference does, and the mask of the classes that are labelled or predicted at all."""
        cm = self.confusion_matrix
        hits = np.diagonal(cm)
        union = cm.sum(axis=0) + cm.sum(axis=1) - hits
        return 1e-8 + hits / (union + 1e-8), union > 1e-3

    def get_overall_accuracy(self):
        """Fraction of the counted samples on the diagonal, a Python float; 0 for an empty matrix."""
        cm = self.confusion_matrix
        return float(int(np.trace(cm))) / max(int(cm.sum()), 1)

    def get_average_intersection_union(self, missing_as_one=False):
        """Mean IoU over the classes that occur (over all classes, the missing ones at 1, with ``missing_as_one``);
        0 when no class occurs."""
        iou, existing = self.get_intersection_union_per_class()
        n_existing = np.sum(existing)
        if n_existing == 0:
            return 0
        if missing_as_one:
            return np.sum(np.where(existing, iou, 1.0)) / existing.size
        return np.sum(iou[existing]) / n_existing

    def get_mean_class_accuracy(self):
        """Mean over the labelled classes of hits / labelled; 0 when nothing is labelled."""
        cm = self.confusion_matrix
        labelled = cm.sum(axis=1)
        present = labelled > 0
        if not present.any():
            return 0
        recall = np.diagonal(cm)[present] / labelled[present]
        return sum(recall.tolist()) / int(present.sum())         # summed in class order, as the fixture values were

    def count_gt(self, ground_truth):
        return self.confusion_matrix[ground_truth].sum()
