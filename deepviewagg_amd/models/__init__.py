"""Model-level pieces on the device (reference ``torch_points3d/models``)."""
