"""SegmentationVoter of the reference (metrics/segmentation_helpers.py) with the votes on the device.

The votes, their counts and the raw cloud live on the device of ``raw_data.pos``; ``add_vote`` never copies the outputs
to the host, and ``full_res_preds`` interpolates and takes the ``argmax`` in one kernel per chunk of raw points
(``metrics.full_res.VoteAccumulator``).
"""
import torch

from .. import ops
from ..core.data_transform.grid_transform import SaveOriginalPosId
from .full_res import VoteAccumulator

__all__ = ["SegmentationVoter"]


class SegmentationVoter:
    """Full point cloud prediction from votes interpolated with K-NN."""

    def __init__(self, raw_data, num_classes, conv_type, class_seg_map=None, k: int = 1):
        assert k > 0
        self._raw_data = raw_data
        self._num_pos = raw_data.pos.shape[0]
        self._acc = VoteAccumulator(self._num_pos, num_classes, raw_data.pos.device)
        self._full_res_preds = None
        self._conv_type = conv_type
        self._class_seg_map = class_seg_map
        self._k = k
        self._num_votes = 0

    @property
    def k(self):
        return self._k

    @k.setter
    def k(self, k):
        if isinstance(k, int):
            if k > 0:
                self._k = k
            else:
                raise Exception("k should be >= 1")
        else:
            raise Exception("k used for knn_interpolate should be an int")

    @property
    def num_votes(self):
        return self._num_votes

    @property
    def coverage(self):
        return self._acc.coverage

    @property
    def full_res_labels(self):
        return self._raw_data.y

    @property
    def full_res_preds(self):
        """The predicted class of every raw point, int64 on the device.  With ``class_seg_map`` only those columns
        compete and the result is shifted by ``class_seg_map[0]``, as in the reference."""
        acc = self._acc
        acc.check_ids()
        idx = torch.nonzero(acc.counts > 0).reshape(-1)                       # the one synchronisation
        if idx.numel() == 0:
            raise ValueError("SegmentationVoter: no point has a prediction, there is nothing to interpolate")
        votes = acc.votes[idx].div(acc.counts[idx].to(torch.float32).unsqueeze(-1))
        shift = 0
        if self._class_seg_map:                             # the columns are interpolated independently of each other
            votes = votes[:, self._class_seg_map].contiguous()
            shift = self._class_seg_map[0]
        pos = self._raw_data.pos
        pred, _, _ = ops.knn_interpolate_labels(votes, pos[idx], pos, k=self._k)
        self._full_res_preds = pred + shift
        return self._full_res_preds

    def add_vote(self, data, output, batch_mask):
        """Adds the scores ``output`` [N, nb_classes] of the points ``data[SaveOriginalPosId.KEY][batch_mask]``.  A point
        that occurs several times is counted once: its last occurrence."""
        idx = data[SaveOriginalPosId.KEY][batch_mask]
        self._acc.add(idx, output)
        self._num_votes += 1

    def __repr__(self):
        return "{}(num_pos={})".format(self.__class__.__name__, self._num_pos)
