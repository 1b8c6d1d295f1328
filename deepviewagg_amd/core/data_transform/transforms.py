"""SphereSampling, CylinderSampling, GridSphereSampling, GridCylinderSampling and Select: cutting samples out of a
point cloud around centres.

Mirror of the reference's transforms (torch_points3d/core/data_transform/transforms.py:99-232, :301-432), with which
the S3DIS, ScanNet and KITTI-360 datasets draw every training and evaluation sample.  The reference builds a
scikit-learn ``KDTree`` on the host and calls ``query_radius`` one centre at a time; here the members of ALL centres
come from one exact brute-force radius query on the device (``ops.radius_query``, csrc/ball.hip), whose membership
test is scikit-learn's own, so the same points are selected:

- the members of a sample are in ascending point index (the reference's KD-tree order is unspecified);
- every tensor whose first dimension is the number of points is indexed by the members, other tensors are cloned,
  other attributes are passed on;
- with ``align_origin`` the float32 centre is subtracted from ``pos`` (cylinder: from ``pos[:, :-1]``);
- the ``kd_tree`` attribute is neither read, set nor copied: no tree is built.  The Grid* transforms still delete an
  existing one from their input when ``delattr_kd_tree`` is set, as the reference does;
- the Grid* centres come from this package's ``GridSampling3D`` (the reference's, bit for bit), ``center_label`` is
  ``data.y`` of the point nearest to the centre (``ops.knn_query``, k = 1; cylinder: in the xy plane);
- ``grid_size=None`` means the radius, as the reference's docstring says (its constructor raises on None).

Results land on the input's device; the work runs on the current HIP device.  ``dropin.install()`` copies every
public name of this module onto the reference's module, so the public namespace is the five classes: everything else
is imported under ``_`` names.  Not provided: ``RandomSphere`` (it needs the reference's ``SamplingStrategy``),
``ComputeKDTree`` (there is no tree) and the crop / dropout augmentations of the reference's module.
"""
import itertools as _itertools

import numpy as _np
import torch as _torch

from .grid_transform import GridSampling3D as _GridSampling3D
from .grid_transform import _has, _keys
from .multimodal.image import _get, _set

_KDTREE_KEY = "kd_tree"     # the reference's KDTREE_KEY; public as the classes' KDTREE_KEY attribute


def _number(value):
    """A config value: a number, or a string holding an arithmetic expression (the reference evaluates strings)."""
    if isinstance(value, str):
        return eval(value, {"__builtins__": {}}, {})
    return float(value)


def _as_numpy(centre):
    if _torch.is_tensor(centre):
        centre = centre.detach().cpu().numpy()
    return _np.asarray(centre)


def _rows(centre):
    return _np.expand_dims(centre, 0) if centre.ndim == 1 else centre


def _delete(data, key):
    if isinstance(data, dict):
        del data[key]
    else:
        delattr(data, key)


def _clone(data):
    if callable(getattr(data, "clone", None)):
        return data.clone()
    out = type(data)()
    for key in _keys(data):
        item = _get(data, key)
        _set(out, key, item.clone() if _torch.is_tensor(item) else item)
    return out


def _per_point(item, num_points):
    return _torch.is_tensor(item) and item.dim() > 0 and item.shape[0] == num_points


def _select(data, num_points, index, shift=None, shift_cols=3):
    """New data of the input's type: per-point tensors indexed by ``index`` (a callable device -> index tensor), other
    tensors cloned; ``shift`` (float32 [1, shift_cols]) is subtracted from the leading columns of ``pos``."""
    new_data = type(data)()
    for key in _keys(data):
        if key == _KDTREE_KEY:
            continue
        item = _get(data, key)
        if _per_point(item, num_points):
            ix = index(item.device)
            item = item[ix] if _torch.is_tensor(ix) else item[ix].clone()
            if shift is not None and key == "pos":
                item[:, :shift_cols] -= shift.to(item.device)
        elif _torch.is_tensor(item):
            item = item.clone()
        _set(new_data, key, item)
    return new_data


class _Members:
    """The members of the centres of one radius query, handed out per device."""

    def __init__(self, ptr, idx):
        self._ptr = ptr.tolist()            # host read: the sample sizes
        self._idx = {idx.device: idx}

    def __len__(self):
        return len(self._ptr) - 1

    def of(self, b):
        lo, hi = self._ptr[b], self._ptr[b + 1]

        def index(device):
            if device not in self._idx:
                self._idx[device] = next(iter(self._idx.values())).to(device)
            return self._idx[device][lo:hi]
        return index


def _query(data, centres, radius, dims):
    from ... import ops as _ops
    pos = _get(data, "pos")
    return _Members(*_ops.radius_query(pos, centres, radius, dims=dims)), int(pos.shape[0])


class SphereSampling:
    """ Samples points within a sphere

    Parameters
    ----------
    radius : float
        Radius of the sphere
    sphere_centre : torch.Tensor or np.array
        Centre of the sphere (1D array that contains (x,y,z))
    align_origin : bool, optional
        move resulting point cloud to origin
    """

    KDTREE_KEY = _KDTREE_KEY
    _DIMS = 3

    def __init__(self, radius, sphere_centre, align_origin=True):
        self._radius = radius
        self._centre = _rows(_as_numpy(sphere_centre))
        self._align_origin = align_origin

    def _sample(self, data, num_points, index):
        shift = _torch.FloatTensor(self._centre[:1]) if self._align_origin else None
        return _select(data, num_points, index, shift, self._DIMS)

    def __call__(self, data):
        members, num_points = _query(data, self._centre[:1], self._radius, self._DIMS)
        return self._sample(data, num_points, members.of(0))

    def __repr__(self):
        return "{}(radius={}, center={}, align_origin={})".format(
            self.__class__.__name__, self._radius, self._centre, self._align_origin
        )


class CylinderSampling(SphereSampling):
    """ Samples points within a cylinder

    Parameters
    ----------
    radius : float
        Radius of the cylinder
    cylinder_centre : torch.Tensor or np.array
        Centre of the cylinder (1D array that contains (x,y,z) or (x,y))
    align_origin : bool, optional
        move resulting point cloud to origin
    """

    _DIMS = 2

    def __init__(self, radius, cylinder_centre, align_origin=True):
        cylinder_centre = _as_numpy(cylinder_centre)
        if cylinder_centre.shape[-1] == 3:
            cylinder_centre = cylinder_centre[..., :-1]
        super().__init__(radius, cylinder_centre, align_origin)


class GridSphereSampling:
    """Fits the point cloud to a grid and for each point in this grid,
    create a sphere with a radius r

    Parameters
    ----------
    radius: float
        Radius of the sphere to be sampled.
    grid_size: float, optional
        Grid_size to be used with GridSampling3D to select spheres center. If None, radius will be used
    delattr_kd_tree: bool, optional
        If True, KDTREE_KEY should be deleted as an attribute if it exists
    center: bool, optional
        If True, a centre transform is apply on each sphere.
    """

    KDTREE_KEY = _KDTREE_KEY
    _SAMPLER = SphereSampling

    def __init__(self, radius, grid_size=None, delattr_kd_tree=True, center=True):
        self._radius = _number(radius)
        grid_size = None if grid_size is None else _number(grid_size)
        self._grid_sampling = _GridSampling3D(size=grid_size if grid_size else self._radius)
        self._delattr_kd_tree = delattr_kd_tree
        self._center = center

    def _centres(self, grid_pos):
        """float32 numpy [B, dims] centres from the grid-sampled positions, in sample order."""
        return _np.asarray(grid_pos)

    def _process(self, data):
        from ... import ops as _ops
        if _has(data, self.KDTREE_KEY) and self._delattr_kd_tree:
            _delete(data, self.KDTREE_KEY)
        grid_data = self._grid_sampling(_clone(data))
        centres = self._centres(_get(grid_data, "pos").detach().cpu())
        dims = self._SAMPLER._DIMS
        members, num_points = _query(data, centres, self._radius, dims)

        # closest original point of every centre (cylinder: in the xy plane)
        pos = _get(data, "pos")
        device = _torch.device("cuda", _torch.cuda.current_device())
        search = pos.detach().to(device).float().clone()
        query = _torch.zeros((centres.shape[0], 3), dtype=_torch.float32, device=device)
        query[:, :dims] = _torch.from_numpy(_np.ascontiguousarray(centres)).to(device)
        search[:, dims:] = 0
        nearest = _ops.knn_query(query, search, 1)[0].long()
        y = _get(data, "y")
        labels = y[nearest[:, 0].to(y.device)]

        datas = []
        for b in range(len(members)):
            sampler = self._SAMPLER(self._radius, centres[b], align_origin=self._center)
            new_data = sampler._sample(data, num_points, members.of(b))
            _set(new_data, "center_label", labels[b:b + 1].clone())
            datas.append(new_data)
        return datas

    def __call__(self, data):
        if isinstance(data, list):
            data = [self._process(d) for d in data]
            data = list(_itertools.chain(*data))  # 2d list needs to be flatten
        else:
            data = self._process(data)
        return data

    def __repr__(self):
        return "{}(radius={}, center={})".format(self.__class__.__name__, self._radius, self._center)


class GridCylinderSampling(GridSphereSampling):
    """Fits the point cloud to a grid and for each point in this grid,
    create a cylinder with a radius r

    Parameters
    ----------
    radius: float
        Radius of the cylinder to be sampled.
    grid_size: float, optional
        Grid_size to be used with GridSampling3D to select cylinders center. If None, radius will be used
    delattr_kd_tree: bool, optional
        If True, KDTREE_KEY should be deleted as an attribute if it exists
    center: bool, optional
        If True, a centre transform is apply on each cylinder.
    """

    _SAMPLER = CylinderSampling

    def _centres(self, grid_pos):
        # the lexicographically sorted unique xy rows
        return _np.unique(_np.asarray(grid_pos[:, :-1]), axis=0)


class Select:
    """ Selects given points from a data object

    Parameters
    ----------
    indices : torch.Tensor
        indeices of the points to keep. Can also be a boolean mask
    """

    def __init__(self, indices=None):
        self._indices = indices

    def __call__(self, data):
        num_points = _get(data, "pos").shape[0]
        indices = self._indices

        def index(device):
            return indices.to(device) if _torch.is_tensor(indices) else indices
        return _select(data, num_points, index)


# The augmentations of the reference's module that augment.py provides: kept out of the eagerly listed names above and
# served by name, as grid_transform.py serves ElasticDistortion.
_LAZY = ("RandomNoise", "RandomScaleAnisotropic", "RandomSymmetry", "ShiftVoxels")


def __getattr__(name):
    if name in _LAZY:
        from . import augment as _augment
        return getattr(_augment, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
