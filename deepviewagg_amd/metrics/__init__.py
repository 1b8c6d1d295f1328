"""Losses and trackers of the segmentation step on the device (reference ``torch_points3d/metrics``)."""
