"""Lovasz-softmax on the device (reference metrics/lovasz_loss.py:155-215; Berman et al., CVPR 2018).

The reference's names and signatures, bodies of our own over ``ops.lovasz_softmax_flat`` (csrc/segloss.hip): one stable
radix sort of all (point, class) errors and one segmented pass, the Jaccard increments formed from integer counts in
float64, instead of a Python loop of one ``torch.sort`` and two ``cumsum`` per class.
"""
import torch

from .. import ops

__all__ = ["lovasz_softmax", "lovasz_softmax_flat"]


def lovasz_softmax(probas, labels, classes='present', per_image=False, ignore=None):
    """Multi-class Lovasz-softmax loss of ``probas`` float32 [P, C] against ``labels`` [P].

    ``classes``: 'all', 'present' (classes that occur among the labels kept) or a list of classes to average;
    ``ignore``: the void label, whose points take no part.  ``per_image=True`` raises NotImplementedError: on [P, C]
    input the reference would treat every point as an image of its own.

    Differences from the reference, all on inputs it handles badly:
      * every point ignored: returns ``probas[:0] * 0.`` (shape [0, C]) as the reference does.  The shape of the
        result depends on the data, so EVERY call with ``ignore`` set reads one flag back from the device (one host
        synchronisation per call).  ``ops.lovasz_softmax_flat`` and ``metrics.losses.segmentation_loss`` return a
        zero loss with a zero gradient in that case and never synchronise: a training step should call those;
      * exactly one valid point: the reference raises IndexError (its ``squeeze()`` drops the point axis); here the
        loss is computed (|fg - p| of that point, averaged over the classes taking part);
      * equal errors within a class are ordered by ascending point index; torch's sort leaves their order open.  The
        loss does not depend on it, the gradient of the tied points does.
    """
    if per_image:
        raise NotImplementedError("lovasz_softmax(per_image=True): [P, C] input has no image axis "
                                  "(the reference would treat every point as an image)")
    labels = labels.view(-1)
    if ignore is not None and labels.numel() and not bool((labels != ignore).any()):
        return probas[:0] * 0.
    return ops.lovasz_softmax_flat(probas, labels, classes=classes, ignore=ignore)


def lovasz_softmax_flat(probas, labels, classes='present'):
    """The loss over all points of ``probas`` [P, C], ``labels`` [P] (no void label)."""
    if probas.numel() == 0:
        return probas * 0.
    return ops.lovasz_softmax_flat(probas, labels, classes=classes, ignore=None)
