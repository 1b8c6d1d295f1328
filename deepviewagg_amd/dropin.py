"""Make the reference's plugin lookups resolve to the HIP-backed classes.

The reference finds its modules by name at the dotted paths
``torch_points3d.modules.multimodal.{pooling,fusion}`` (ModalityFactory.get_module,
models/base_architectures/unet.py:69-101), ``torch_points3d.core.multimodal.visibility``
(MapImages, core/data_transform/multimodal/image.py:214-215), finds its pre-transforms
(PCAComputePointwise, EigenFeatures) in ``torch_points3d.core.data_transform.features``, GridSampling3D,
SaveOriginalPosId and ElasticDistortion in ``torch_points3d.core.data_transform.grid_transform``, the sphere and
cylinder samplers (SphereSampling, CylinderSampling, GridSphereSampling, GridCylinderSampling, Select) in
``torch_points3d.core.data_transform.transforms``, the 3D augmentations of ``core/data_transform/augment.py`` in the
reference's ``transforms`` and ``features`` modules (``RandomRotate`` and ``Center`` on the package alone), and all groups on the package
``torch_points3d.core.data_transform`` itself (``instantiate_transform`` and ``cT.GridSampling3D`` look them up there),
and imports the data classes from
``torch_points3d.core.multimodal.{csr,image,data}`` (``MMData`` / ``MMBatch`` in the last), and takes ``lovasz_softmax`` and ``ConfusionMatrix`` from
``torch_points3d.metrics.{lovasz_loss,confusion_matrix}`` and ``SegmentationVoter`` from
``torch_points3d.metrics.segmentation_helpers``; where the reference's ``SegmentationTracker`` can be imported,
its ``_compute_metrics`` becomes ``deepviewagg_amd.metrics.segmentation_tracker.compute_metrics``; where
``torch_points3d.models.segmentation.multimodal.no3d`` is loaded or can be imported, ``No3D.forward`` becomes
``deepviewagg_amd.models.no3d.forward`` (nearest-seen fill and view-level loss on the device).  The image transforms
of the data configs resolve on ``torch_points3d.core.data_transform.multimodal.image``, which is aliased whole: with
``ColorJitter``, ``Normalize`` and ``ToImageData`` every per-sample image transform the shipped chains name is there, and
with ``LoadImages`` and ``NonStaticMask`` (decode on the host, Pillow's resample, roll, crop and the mask comparison on
the device) every image ``pre_transform`` the shipped multimodal data configs name as well; they stand next
to ``FusedImageTail`` and ``fuse_image_tail`` (one pass for the tail of a chain) and to ``DeferImages`` and
``defer_image_windows`` (image selection, roll and crop deferred into that pass; the deferred setting is
``WindowedSameSettingImageData`` / ``SameSettingImageData.windowed()`` in ``core.multimodal.image``).  ``install()`` either patches an importable
``torch_points3d`` in place (attribute by attribute) or, when the package is absent, registers alias
modules under those dotted names in ``sys.modules``.
"""
import importlib
import sys
import types

_ALIASES = {
    "torch_points3d.modules.multimodal.pooling": "deepviewagg_amd.modules.multimodal.pooling",
    "torch_points3d.modules.multimodal.fusion": "deepviewagg_amd.modules.multimodal.fusion",
    "torch_points3d.modules.multimodal.dropout": "deepviewagg_amd.modules.multimodal.dropout",
    "torch_points3d.modules.multimodal.modules": "deepviewagg_amd.modules.multimodal.modules",
    "torch_points3d.core.data_transform.multimodal.image": "deepviewagg_amd.core.data_transform.multimodal.image",
    "torch_points3d.core.data_transform.features": "deepviewagg_amd.core.data_transform.features",
    "torch_points3d.core.data_transform.grid_transform": "deepviewagg_amd.core.data_transform.grid_transform",
    "torch_points3d.core.data_transform.transforms": "deepviewagg_amd.core.data_transform.transforms",
    "torch_points3d.core.multimodal.csr": "deepviewagg_amd.core.multimodal.csr",
    "torch_points3d.core.multimodal.image": "deepviewagg_amd.core.multimodal.image",
    "torch_points3d.core.multimodal.data": "deepviewagg_amd.core.multimodal.data",
    "torch_points3d.core.multimodal.visibility": "deepviewagg_amd.core.multimodal.visibility",
    "torch_points3d.utils.multimodal": "deepviewagg_amd.utils.multimodal",
    "torch_points3d.modules.SparseConv3d.modules": "deepviewagg_amd.modules.SparseConv3d.modules",
    "torch_points3d.modules.SparseConv3d.nn": "deepviewagg_amd.modules.SparseConv3d.nn",
    "torch_points3d.metrics.lovasz_loss": "deepviewagg_amd.metrics.lovasz_loss",
    "torch_points3d.metrics.confusion_matrix": "deepviewagg_amd.metrics.confusion_matrix",
    "torch_points3d.metrics.segmentation_helpers": "deepviewagg_amd.metrics.segmentation_helpers",
}

# (package, our module, names): set on the package after the aliases above
_PACKAGE_NAMES = [
    ("torch_points3d.core.data_transform", "deepviewagg_amd.core.data_transform.grid_transform",
     ("GridSampling3D", "SaveOriginalPosId", "ElasticDistortion")),
    # our module serves this name through its __getattr__: on a patched reference module it has to be set by name
    ("torch_points3d.core.data_transform.grid_transform", "deepviewagg_amd.core.data_transform.grid_transform",
     ("ElasticDistortion",)),
    ("torch_points3d.core.data_transform", "deepviewagg_amd.core.data_transform.transforms",
     ("SphereSampling", "CylinderSampling", "GridSphereSampling", "GridCylinderSampling", "Select")),
    # the 3D augmentations of augment.py, which our transforms / features modules serve through their __getattr__: by
    # name on a patched reference module and on the package
    ("torch_points3d.core.data_transform.transforms", "deepviewagg_amd.core.data_transform.transforms",
     ("RandomNoise", "RandomScaleAnisotropic", "RandomSymmetry", "ShiftVoxels")),
    ("torch_points3d.core.data_transform", "deepviewagg_amd.core.data_transform.transforms",
     ("RandomNoise", "RandomScaleAnisotropic", "RandomSymmetry", "ShiftVoxels")),
    ("torch_points3d.core.data_transform.features", "deepviewagg_amd.core.data_transform.features",
     ("Random3AxisRotation", "XYZFeature", "AddFeatsByKeys", "AddFeatByKey")),
    ("torch_points3d.core.data_transform", "deepviewagg_amd.core.data_transform.features",
     ("Random3AxisRotation", "XYZFeature", "AddFeatsByKeys", "AddFeatByKey")),
    # torch_geometric's, which the reference re-exports on the package alone
    ("torch_points3d.core.data_transform", "deepviewagg_amd.core.data_transform.augment", ("RandomRotate", "Center")),
]


def install(patch_existing=True):
    """Returns the list of dotted names that now resolve to deepviewagg_amd code."""
    done = []
    for ref_name, our_name in _ALIASES.items():
        ours = importlib.import_module(our_name)
        target = None
        if patch_existing:
            try:
                target = importlib.import_module(ref_name)
            except Exception:
                target = None
        if target is not None:
            for k, v in vars(ours).items():
                if not k.startswith("_"):
                    setattr(target, k, v)
        else:
            parts = ref_name.split(".")
            for i in range(1, len(parts)):
                pkg = ".".join(parts[:i])
                if pkg not in sys.modules:
                    m = types.ModuleType(pkg)
                    m.__path__ = []
                    sys.modules[pkg] = m
            sys.modules[ref_name] = ours
            setattr(sys.modules[".".join(parts[:-1])], parts[-1], ours)
        done.append(ref_name)
    # names the reference re-exports on a package: its transform lookups read them there
    for pkg_name, our_name, names in _PACKAGE_NAMES:
        ours = importlib.import_module(our_name)
        pkg = sys.modules.get(pkg_name)
        if pkg is None:
            pkg = importlib.import_module(pkg_name)
        if pkg is ours:
            continue
        for k in names:
            setattr(pkg, k, getattr(ours, k))
    _bind_tracker(patch_existing)
    _bind_no3d(patch_existing)
    return done


def _bind_tracker(patch_existing):
    """The reference's SegmentationTracker, when it can be imported, counts on the device from now on."""
    name = "torch_points3d.metrics.segmentation_tracker"
    tracker = sys.modules.get(name)
    if tracker is None and patch_existing:
        try:
            tracker = importlib.import_module(name)
        except Exception:
            tracker = None
    cls = getattr(tracker, "SegmentationTracker", None)
    if cls is None:
        return
    from .metrics.confusion_matrix import ConfusionMatrix
    from .metrics.segmentation_tracker import compute_metrics
    cls._compute_metrics = compute_metrics
    tracker.ConfusionMatrix = ConfusionMatrix


def _bind_no3d(patch_existing):
    """The reference's image-only models (models/segmentation/multimodal/no3d.py), when the module is loaded or can be
    imported, run their tail on the device from now on: nearest-seen fill and view-level loss (models.no3d)."""
    name = "torch_points3d.models.segmentation.multimodal.no3d"
    module = sys.modules.get(name)
    if module is None and patch_existing:
        try:
            module = importlib.import_module(name)
        except Exception:
            module = None
    cls = getattr(module, "No3D", None)
    if cls is None:
        return
    from .models.no3d import forward
    cls.forward = forward
