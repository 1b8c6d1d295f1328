"""The loss composition of the segmentation models (reference models/segmentation/sparseconv3d.py:42-55)."""
from .. import ops

IGNORE_LABEL = -1       # torch_points3d.datasets.segmentation.IGNORE_LABEL


def segmentation_loss(logits, labels, weight_classes=None, use_cross_entropy=True, use_lovasz=False):
    """``(output, loss_seg, loss_cross_entropy, loss_lovasz)`` of ``APIModel.forward``: ``output`` = the float32
    log-probabilities of ``logits`` [P, C] (float32, or bfloat16 / float16 as the head emits under autocast),
    ``loss_cross_entropy`` = the NLL of ``output`` weighted by ``weight_classes`` with IGNORE_LABEL ignored,
    ``loss_lovasz`` = Lovasz-softmax of ``output.exp()`` over the classes present, ``loss_seg`` their sum.  A loss that
    is switched off is None.  log-softmax and NLL are one kernel forward and one backward; nothing synchronises with
    the host.  When every label is ignored the NLL is NaN (as torch) and the Lovasz term is 0 with a zero gradient
    (the reference returns a [0, C] tensor there, on which its ``backward()`` fails)."""
    assert use_cross_entropy or use_lovasz, "Choose at least one between Cross-Entropy loss and Lovasz loss."
    output, nll = ops.log_softmax_nll(logits, labels, weight=weight_classes, ignore_index=IGNORE_LABEL)
    loss_seg, loss_cross_entropy, loss_lovasz = 0, None, None
    if use_cross_entropy:
        loss_cross_entropy = nll
        loss_seg = loss_seg + loss_cross_entropy
    if use_lovasz:
        loss_lovasz = ops.lovasz_softmax_flat(output.exp(), labels, classes='present', ignore=IGNORE_LABEL)
        loss_seg = loss_seg + loss_lovasz
    return output, loss_seg, loss_cross_entropy, loss_lovasz
