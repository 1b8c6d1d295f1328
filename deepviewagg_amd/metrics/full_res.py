"""The voted and the full-resolution metrics on the device: the core the reference's three dataset trackers share
(metrics/s3dis_tracker.py:56-61, 94-118; metrics/scannet_segmentation_tracker.py:110-135 through SegmentationVoter;
metrics/kitti360_tracker.py:144-152, 188-222).

Predictions of overlapping samples are accumulated on the raw cloud (``ops.vote_add``), carried to every raw point by
nearest-neighbour interpolation and counted there (``ops.knn_interpolate_labels``): no batch of outputs is copied to
the host and no [N_raw, C] tensor is formed to take its ``argmax``.  The counts end in ``metrics.ConfusionMatrix``, whose
formulas are the reference's.
"""
import torch

from .. import ops
from .confusion_matrix import ConfusionMatrix

__all__ = ["VoteAccumulator"]

_NEVER = -(1 << 63)      # an ignore value no label carries: rows masked with it take no part and raise no error


class VoteAccumulator:
    """``votes`` float32 [num_points, num_classes] and ``counts`` int32 [num_points] on ``device``.

    Duplicate rule: an id that occurs several times in one ``add`` is counted once, as the reference warns, and it is
    always its last occurrence (torch leaves open which one)."""

    def __init__(self, num_points, num_classes, device):
        self.num_points, self.num_classes = int(num_points), int(num_classes)
        self.device = torch.device(device)
        self.votes = torch.zeros((self.num_points, self.num_classes), dtype=torch.float32, device=self.device)
        self.counts = torch.zeros(self.num_points, dtype=torch.int32, device=self.device)
        self._slots = ops.vote_slots(self.num_points, self.device)          # cleared once, here
        self._bad = torch.zeros(1, dtype=torch.int64, device=self.device)

    def add(self, ids, outputs):
        """Adds the rows of ``outputs`` [P, C] (float32, bfloat16 or float16, on the device) to the points ``ids``
        ([P], or [P, 1] as the trackers flatten it).  No host synchronisation: an id outside the cloud writes nothing
        and makes ``check_ids`` (and every finalisation) raise."""
        ids = ids.to(self.device).reshape(-1)
        self._bad += ops.vote_add(self.votes, self.counts, ids, outputs, self._slots)

    def check_ids(self):
        """The reference's "Origin ids are larger than the number of points" check, made once instead of per batch."""
        n_bad = int(self._bad.item())
        if n_bad:
            raise ValueError(f"VoteAccumulator: {n_bad} origin ids lie outside the raw cloud of {self.num_points} points")

    @property
    def has_prediction(self):
        return self.counts > 0

    @property
    def coverage(self):
        """The fraction of the raw points that carry a vote (synchronises)."""
        return float(int((self.counts > 0).sum())) / self.num_points

    def _masked_labels(self, labels, ignore_label, mask=None):
        lab = labels.to(self.device).reshape(-1).to(torch.int64)
        if lab.shape[0] != self.num_points:
            raise ValueError(f"VoteAccumulator: {lab.shape[0]} labels for {self.num_points} points")
        if ignore_label is not None:
            lab = torch.where(lab == int(ignore_label), _NEVER, lab)
        if mask is not None:
            lab = torch.where(mask, lab, _NEVER)
        return lab

    def vote_confusion(self, labels, ignore_label=None):
        """The ``argmax`` of the voted rows against their labels (the reference's vote mIoU), as a ``ConfusionMatrix``:
        the points without a vote, and those labelled ``ignore_label``, take no part; another label outside
        [0, num_classes) makes reading the matrix raise."""
        self.check_ids()
        cm = ConfusionMatrix(self.num_classes)
        cm.count_outputs(self.votes, self._masked_labels(labels, ignore_label, self.counts > 0), _NEVER)
        return cm

    def full_res_predictions(self, pos, k=1, normalise=False, fill_only=False, labels=None, ignore_label=None):
        """The predicted class of every raw point, int64 [num_points]: the votes of the points that have some are
        interpolated at ``pos`` [num_points, 3] from their ``k`` nearest voted points and the first maximum is taken.

        The default call is S3DIS (sums of votes, k = 1); ``normalise=True`` divides the votes by their counts first
        (ScanNet and SegmentationVoter); ``fill_only=True`` is KITTI-360: a point with a vote keeps the ``argmax`` of its
        own row and only the others are interpolated.  With ``labels`` [num_points] the return value is ``(pred,
        ConfusionMatrix)``, the matrix counted over all points whose label is not ``ignore_label``.

        Raises ValueError when no point has a prediction (the reference crashes inside its K-NN).  Compacting
        ``pos[has_prediction]`` synchronises once per finalisation, and the K-NN reads one scalar per chunk of 2^22
        queries."""
        self.check_ids()
        pos = pos.to(self.device)
        if pos.dim() != 2 or tuple(pos.shape) != (self.num_points, 3):
            raise ValueError(f"VoteAccumulator: pos must be [{self.num_points}, 3], got {tuple(pos.shape)}")
        idx = torch.nonzero(self.counts > 0).reshape(-1)                      # the one synchronisation
        if idx.numel() == 0:
            raise ValueError("VoteAccumulator: no point has a prediction, there is nothing to interpolate")
        x = self.votes[idx]
        if normalise:
            x = x.div(self.counts[idx].to(torch.float32).unsqueeze(-1))
        lab = None if labels is None else self._masked_labels(labels, ignore_label)
        pred, counts, n_bad = ops.knn_interpolate_labels(
            x, pos[idx], pos, k=k, labels=lab, num_classes=self.num_classes, ignore_index=_NEVER,
            keep_counts=self.counts if fill_only else None)
        if labels is None:
            return pred
        cm = ConfusionMatrix(self.num_classes)
        cm._dev, cm._bad = counts, n_bad
        return pred, cm
