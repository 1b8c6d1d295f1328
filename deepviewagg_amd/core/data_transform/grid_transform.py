"""GridSampling3D and SaveOriginalPosId: voxel-grid subsampling of a point cloud.

Mirror of the reference's transforms (torch_points3d/core/data_transform/grid_transform.py:24-191), which every
multimodal data config runs: pre-collate in mode ``mean`` (producer of ``full_pos``), per sample in mode ``last`` with
``quantize_coords`` (producer of the sparse backbone's ``coords``, carrying ``mapping_index`` through), and to build
the datasets' sampling centres.  The reference composes torch_cluster ``grid_cluster``, torch_geometric
``voxel_grid`` + ``consecutive_cluster`` and torch_scatter on the CPU; here the quantisation, the sort, the unique and
the reductions are HIP kernels (``ops.grid_cluster`` / ``grid_mean`` / ``grid_majority``, csrc/grid.hip) and only
the ``last`` gathers are ``index_select``.  Results are the reference's, bit for bit:

- ``coords = round(pos / size)`` with the division correctly rounded in the dtype of ``pos``, ties to even;
- voxels in ascending (batch, z, y, x);
- mode ``last`` draws the reference's ``torch.randperm(N)`` from the default CPU generator, before any other draw, and
  takes the member of largest position in it (the reference physically shuffles, then keeps the last point); under
  ``torch.manual_seed`` the same points are selected.  ``full_pos`` is then the shuffled ``pos``, as in the reference;
- mode ``mean``: floating attributes are torch_scatter's CPU ``scatter_mean`` (sequential sum in the attribute's dtype,
  divided by the count in that dtype), ``y`` / ``instance_labels`` the majority label (ties to the smallest), bool
  attributes True when every member is True, other integers the integer mean rounded toward zero (the reference's
  ``floor_divide`` of its time; floor and truncation differ only for negative means); ``batch``, ``origin_id`` and
  ``mapping_index`` take the representative's row.

Results land on the input's device (CPU data in gives CPU tensors out, which the reference's ``ShiftVoxels`` needs);
the work runs on the current HIP device.  ``dropin.install()`` copies every public name of this module onto the
reference's module, so the public namespace is the two classes: everything else is imported under ``_`` names.

``ElasticDistortion`` (reference grid_transform.py:194-256), the augmentation that opens the ScanNet
``train_transform``, is the third class of the reference's module.  It is defined at the end of this file, kept out
of the eagerly listed names above and served by the module's ``__getattr__``: ``grid_transform.ElasticDistortion``,
``from ...grid_transform import ElasticDistortion`` and pickling by name all resolve, and ``dropin.install()`` sets it
on the reference's module and package by name.
"""
import logging as _logging
import random as _random
import re as _re

import torch as _torch

from ...utils.multimodal import MAPPING_KEY as _MAPPING_KEY
from .multimodal.image import _get, _num_nodes, _set

_log = _logging.getLogger(__name__)

# Label will be the majority label in each voxel
_INTEGER_LABEL_KEYS = ["y", "instance_labels"]


def _apply(transform, data):
    if isinstance(data, list):
        return [transform._process(d) for d in data]
    return transform._process(data)


def _has(data, key):
    if isinstance(data, dict):
        return key in data
    return hasattr(data, key)


def _keys(data):
    """Attribute names of a Data, a dict or a SimpleNamespace."""
    if isinstance(data, dict):
        return list(data.keys())
    keys = getattr(data, "keys", None)
    if callable(keys):
        keys = keys()
    if keys is None:
        keys = [k for k in vars(data) if not k.startswith("_")]
    return list(keys)


class GridSampling3D:
    """Clusters points into voxels with size :attr:`size`.

    Parameters
    ----------
    size: float
        Size of a voxel (in each dimension).
    quantize_coords: bool
        If True, the points' integer coordinates in the grid are stored in a new ``coords`` attribute (int32).
    mode: string:
        ``mean``: all the points and their features within a cell are averaged.  ``last``: one random point per cell
        is selected with its associated features.
    setattr_full_pos: bool
        If True, the input point positions are saved into a new ``full_pos`` attribute.

    Raises ValueError for an empty cloud, non-finite positions, ``|pos / size| >= 2^24``, a voxel key of more than
    63 bits and attribute names containing ``edge``.
    """

    def __init__(self, size, quantize_coords=False, mode="mean", verbose=False, setattr_full_pos=False):
        if mode not in ("mean", "last"):
            raise ValueError(f"GridSampling3D: unknown mode '{mode}', expected 'mean' or 'last'")
        self._grid_size = size
        self._quantize_coords = quantize_coords
        self._mode = mode
        self._setattr_full_pos = setattr_full_pos
        if verbose:
            _log.warning(
                "If you need to keep track of the position of your points, use "
                "SaveOriginalPosId transform before using GridSampling3D.")
            if self._mode == "last":
                _log.warning(
                    "The tensors within data will be shuffled each time this "
                    "transform is applied. Be careful that if an attribute "
                    "doesn't have the size of num_points, it won't be shuffled")

    def _process(self, data):
        from ... import ops as _ops
        pos = _get(data, "pos")
        n = int(pos.shape[0])
        if n == 0:
            raise ValueError("GridSampling3D: the point cloud is empty (N = 0)")
        keys = _keys(data)
        for key in keys:
            if _re.search("edge", key):
                raise ValueError("Edges not supported. Wrong data type.")
        # the reference's shuffle_data: one randperm of the default CPU generator, the first draw of the transform
        perm = _torch.randperm(n) if self._mode == "last" else None

        device = _torch.device("cuda", _torch.cuda.current_device())
        pos_dev = pos.to(device)
        rank = None
        if perm is not None:
            perm_dev = perm.to(device)
            rank = _torch.empty_like(perm_dev)
            rank[perm_dev] = _torch.arange(n, device=device)     # the position of every point in the shuffle
        batch = _get(data, "batch") if _has(data, "batch") else None
        if batch is not None:
            batch = batch.to(device)
        clusters = _ops.grid_cluster(pos_dev, self._grid_size, batch=batch, rank=rank)

        num_nodes = _num_nodes(data)
        for key in keys:
            item = _get(data, key)
            if not _torch.is_tensor(item) or item.dim() == 0 or item.shape[0] != num_nodes:
                continue
            src = pos_dev if item is pos else item.to(device)
            if self._mode == "last" or key in ("batch", SaveOriginalPosId.KEY, _MAPPING_KEY):
                out = src.index_select(0, clusters.rep)
            elif key in _INTEGER_LABEL_KEYS:
                out = _ops.grid_majority(src, clusters)
            else:
                out = _ops.grid_mean(src, clusters)
            _set(data, key, out.to(item.device))

        if self._quantize_coords:
            _set(data, "coords", clusters.coords.to(pos.device))
        _set(data, "grid_size", _torch.tensor([self._grid_size]))
        if self._setattr_full_pos:
            _set(data, "full_pos", pos if perm is None else pos.index_select(0, perm.to(pos.device)))
        return data

    def __call__(self, data):
        return _apply(self, data)

    def __repr__(self):
        return "{}(grid_size={}, quantize_coords={}, mode={})".format(
            self.__class__.__name__, self._grid_size, self._quantize_coords, self._mode
        )


class SaveOriginalPosId:
    """Adds the index of every point (``arange(N)`` on the device of ``pos``) under ``KEY`` (default ``origin_id``),
    so that points can be traced from the output back to the input.  Data that already has the attribute is left
    as it is."""

    KEY = "origin_id"

    def __init__(self, key=None):
        self.KEY = key if key is not None else self.KEY

    def _process(self, data):
        if _has(data, self.KEY):
            return data
        pos = _get(data, "pos")
        _set(data, self.KEY, _torch.arange(0, pos.shape[0], device=pos.device))
        return data

    def __call__(self, data):
        return _apply(self, data)

    def __repr__(self):
        return self.__class__.__name__


class ElasticDistortion:
    """Apply elastic distortion on sparse coordinate space. First projects the position onto a
    voxel grid and then apply the distortion to the voxel grid.

    Parameters
    ----------
    granularity: List[float]
        Granularity of the noise in meters
    magnitude: List[float]
        Noise multiplier in meters

    Returns the same data object with a distorted ``pos``: the reference's result bit for bit under the same seeds of
    ``random`` (the 0.95 gate) and ``numpy.random`` (the noise volume of every level, drawn on the host exactly as the
    reference draws it).  The bounds, the smoothing of the noise and the interpolation at every point run on the
    current HIP device (``ops.elastic_distortion``, csrc/elastic.hip); every level reads six floats back, the bounds
    of the previous level's output.  ``pos`` is float32 [N, 3] on the CPU or on a device, and the result lands on
    the device ``pos`` came from.  An empty cloud raises ValueError, as numpy's reduction does in the reference;
    non-finite ``pos`` is not supported.
    """

    def __init__(self, apply_distorsion=True, granularity=[0.2, 0.8], magnitude=[0.4, 1.6]):
        assert len(magnitude) == len(granularity)
        self._apply_distorsion = apply_distorsion
        self._granularity = granularity
        self._magnitude = magnitude

    @staticmethod
    def elastic_distortion(coords, granularity, magnitude):
        from ... import ops as _ops
        return _ops.elastic_distortion(coords, granularity, magnitude).to(coords.device)

    def __call__(self, data):
        if self._apply_distorsion:
            if _random.random() < 0.95:
                from ... import ops as _ops
                pos = _get(data, "pos")
                out = pos
                for i in range(len(self._granularity)):
                    # a level's bounds are those of the previous level's output, which stays on the HIP device
                    out = _ops.elastic_distortion(out, self._granularity[i], self._magnitude[i])
                _set(data, "pos", out.to(pos.device))
        return data

    def __repr__(self):
        return "{}(apply_distorsion={}, granularity={}, magnitude={})".format(
            self.__class__.__name__, self._apply_distorsion, self._granularity, self._magnitude,
        )


_LAZY = {"ElasticDistortion": ElasticDistortion}
del ElasticDistortion


def __getattr__(name):
    try:
        return _LAZY[name]
    except KeyError:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}") from None
