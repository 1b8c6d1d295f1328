"""The tracker step of the segmentation models without the host copy of the outputs
(reference metrics/segmentation_tracker.py:71-91)."""
from .confusion_matrix import ConfusionMatrix

__all__ = ["compute_metrics"]


def compute_metrics(self, outputs, labels):
    """Replacement for ``SegmentationTracker._compute_metrics(self, outputs, labels)``: the [P, C] outputs stay on the
    device, where one kernel masks the ignored rows, takes the argmax and counts (``ConfusionMatrix.count_outputs``);
    the metrics are then read from the C x C matrix as the reference reads them (that read is the step's one
    synchronisation).  A batch whose labels are all ignored leaves the metrics as they were, as in the reference.  ``dropin.install()`` binds it onto
    the reference's class."""
    if labels.numel() == 0:
        return
    cm = self._confusion_matrix
    if not hasattr(cm, "count_outputs"):            # a tracker built before install(): keep what it counted
        counted = cm.confusion_matrix
        cm = ConfusionMatrix(self._num_classes) if counted is None else ConfusionMatrix.create_from_matrix(counted)
        self._confusion_matrix = cm
    before = cm.confusion_matrix                    # on the host since the previous step's metrics
    n_before = 0 if before is None else int(before.sum())
    cm.count_outputs(outputs.detach(), labels, self._ignore_label)
    if int(cm.confusion_matrix.sum()) == n_before:  # every label ignored: the reference returns before its metrics
        return

    self._acc = 100 * cm.get_overall_accuracy()
    self._macc = 100 * cm.get_mean_class_accuracy()
    self._miou = 100 * cm.get_average_intersection_union()
    self._miou_per_class = {
        i: "{:.2f}".format(100 * v) for i, v in enumerate(cm.get_intersection_union_per_class()[0])
    }
