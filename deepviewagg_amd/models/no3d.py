"""The tail of the image-only models (reference models/segmentation/multimodal/no3d.py:102-154: No3DFeatureFusion,
No3DLogitFusion, the view-loss variants No3DImageFeatureFusion and No3DImageLogitFusion): head, log-softmax,
nearest-seen fill in eval mode, labels of unseen points ignored, point-level or view-level NLL.

Nothing here reads a value back to the host when the search cell is given (``ops.fill_unseen``); the reference's
``torch.any(seen_mask)`` branch becomes a ``torch.where`` on the device flag the fill returns.
"""
import torch
import torch.nn as nn

from .. import ops
from ..metrics.losses import IGNORE_LABEL


def _linear_head(head):
    """True when ``head`` is a Linear or a Sequential of Linears (the reference's head, no3d.py:37-38): row-wise, so it
    commutes with a row gather."""
    if isinstance(head, nn.Linear):
        return True
    return isinstance(head, nn.Sequential) and len(head) > 0 and all(isinstance(m, nn.Linear) for m in head)


def view_logits(head, view_features):
    """``head(last_view_x_mod)`` (no3d.py:146-149).  A lazy gather under a Linear head stays lazy: the head runs on the
    map rows (the ``mlp_on_gathered_rows`` pattern), so no [V, K] tensor appears."""
    if head is None:
        return view_features
    if isinstance(view_features, ops.GatheredFeatures):
        if _linear_head(head):
            return view_features.with_rows(head(view_features.rows))
        return head(view_features.materialize())
    if isinstance(view_features, ops.LAZY_TYPES):
        return head(view_features.materialize())
    return head(view_features)


def _tail(features, seen, pos, labels, head, training, view, weight, ignore_label, cell):
    logits = head(features) if head is not None else features                                  # :102
    n = logits.shape[0]
    if seen is None:                                                                           # :83-84
        seen = torch.zeros(n, dtype=torch.bool, device=logits.device)
    seen = seen.to(torch.bool)
    if training:
        keep = seen                                                                            # :131-134
    else:
        # :105-125.  The fill runs on the logits: a row-wise log-softmax of a copied row is the copy of its
        # log-softmax, bit for bit
        logits, any_seen = ops.fill_unseen(logits, pos, seen, cell=cell)
        keep = seen | any_seen                                                                 # :126-129
    if labels is not None:
        labels = torch.where(keep, labels, torch.full_like(labels, ignore_label))
    point_labels = labels if labels is not None else torch.full((n,), ignore_label, dtype=torch.int64,
                                                                device=logits.device)
    output, loss = ops.log_softmax_nll(logits, point_labels, weight=weight, ignore_index=ignore_label)   # :103, :154
    if labels is None:
        return output, None, None
    if view is not None:                                                                       # :145-152
        view_features, csr_idx = view
        loss = ops.view_nll(view_logits(head, view_features), labels, csr_idx, weight=weight,
                            ignore_index=ignore_label)
    return output, loss, labels


def no3d_tail(features, seen, pos, labels=None, head=None, training=False, view=None, weight=None,
              ignore_label=IGNORE_LABEL, cell=None):
    """``(output, loss)`` of ``No3D.forward`` (no3d.py:102-154): ``output`` float32 [N, K] log-probabilities, ``loss``
    the segmentation loss or None without labels.

    ``features`` [N, C] are the backbone's point features, ``head`` the segmentation head (None: the features are the
    logits), ``seen`` the bool [N] mask of points that some image sees (None: none is), ``pos`` [N, 3].  In eval mode
    every unseen point takes the output of its nearest seen point (``ops.fill_unseen``: across the whole batch, as the
    reference; not differentiable, the logits are detached there).  Labels of unseen points become ``ignore_label``
    in training, and in eval mode only when no point is seen; the caller's ``labels`` tensor is left as it is.  With
    ``view = (last_view_x_mod, last_view_csr_idx)`` the loss is the view-level one (``ops.view_nll``), with the head
    applied per map row when ``last_view_x_mod`` is a lazy gather (``UnimodalBranch.KEEP_LAST_VIEW_LAZY``); else the
    point-level NLL.  ``weight`` are optional class weights, ``cell`` the grid cell of the search (None: sized from
    the extent of ``pos``, the one host read of the tail)."""
    output, loss, _ = _tail(features, seen, pos, labels, head, training, view, weight, ignore_label, cell)
    return output, loss


def forward(self, *args, **kwargs):
    """``No3D.forward`` on the device tail; ``dropin.install()`` binds it on the reference's class."""
    data = self.backbone(self.input)
    features, seen_mask = data.x, data.seen
    if features.device != self.device:                                                         # :80-81
        features = features.to(self.device)
    has_head = bool(self._HAS_HEAD)
    for m in self.modalities:                                                                  # :89-100
        for i in range(self.input.modalities[m].num_settings):
            if has_head:
                f_map = data[m][i].x
                s = f_map.shape
                f_map = self.head(f_map.permute(1, 0, 2, 3).reshape(s[1], -1).T)
                self.input.modalities[m][i].pred = f_map.T.reshape(f_map.shape[1], s[0], s[2], s[3]).permute(1, 0, 2, 3)
                self.input.modalities[m][i].feat = data[m][i].x
            else:
                self.input.modalities[m][i].pred = data[m][i].x
    view = None
    if self._MODALITY_VIEW_LOSS is not None and self.labels is not None:
        mod = data[self._MODALITY_VIEW_LOSS]
        view = (mod.last_view_x_mod, mod.last_view_csr_idx)
    self.output, loss, labels = _tail(features, seen_mask, data.pos, self.labels, self.head if has_head else None,
                                      self.training, view, None, IGNORE_LABEL, None)
    if labels is not None:
        self.labels = labels           # the reference masks self.labels in place (:129, :134)
        self.loss_seg = loss
