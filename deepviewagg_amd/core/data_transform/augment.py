"""The 3D augmentations between the sampling and ``GridSampling3D`` in the shipped ``train_transform`` chains, for a
cloud that lives on the device.

Mirror of the reference's ``RandomNoise``, ``RandomScaleAnisotropic``, ``RandomSymmetry``, ``ShiftVoxels``
(torch_points3d/core/data_transform/transforms.py:463-563, :699-723), ``Random3AxisRotation``, ``AddFeatsByKeys``,
``AddFeatByKey`` and ``XYZFeature`` (features.py:30-81, :109-268, :604-637), and of torch_geometric's ``RandomRotate``
and ``Center``, which the S3DIS and KITTI-360 chains name.  Constructors, defaults, assertions and ``repr`` strings are
the reference's.  Every class takes a ``Data``, a dict or a ``SimpleNamespace``; a list is processed element by element.

The positional classes (``RandomNoise``, ``RandomRotate``, ``Random3AxisRotation``, ``RandomScaleAnisotropic``,
``RandomSymmetry``, ``Center``) each have ``draw(data)``: the class's random draws, made on the host from the same
generators (Python's ``random``, torch's default CPU generator), in the same order and with the same host arithmetic
as the reference, returned as the list of ``ops.cloud_augment`` steps of one application.  After a call both generators
are in the state the reference leaves them in.  One line differs: the two 3 x 3 products behind
``Random3AxisRotation``'s matrix are separately rounded float32 (``_mm3``) where the reference calls ``torch.mm``, whose
last bit depends on the host's BLAS kernel.

- On a float32 ``pos`` on a HIP device a class is one call of ``ops.cloud_augment`` (csrc/cloud_augment.hip), whose
  docstring states the arithmetic.
- On a CPU tensor, on a ``pos`` that is not float32, with ``CLOUD_AUGMENT_ON_DEVICE = False``, or beyond the kernel's
  size limit (``3 N >= 2^31``), it is the torch composition of the reference's lines: the fallback and the yardstick.
- ``RandomNoise``, ``RandomScaleAnisotropic`` on ``pos``, ``RandomSymmetry`` and ``ShiftVoxels`` give the composition's
  result bit for bit on either route.  Two deviations of the device route are inherent: a rotation is
  ``q_i = ((p_0 M_i0 + p_1 M_i1) + p_2 M_i2)`` where the composition calls a BLAS ``matmul`` (both lie within
  ``3 * 2^-24 * sum_j |p_j| |M_ij|`` of the exact value), and ``Center`` subtracts the correctly rounded mean (a float64
  sum) where torch's float32 ``mean`` carries its summation error.  The normalised ``norm`` of the scale is correctly
  rounded operation by operation; ``F.normalize`` agrees with it within a few ulp.
- Every class assigns new tensors and never writes its input.  The reference's ``RandomSymmetry`` and ``ShiftVoxels``
  write ``pos`` / ``coords`` in place.
- An empty cloud consumes the draws, launches nothing and keeps its empty ``pos``.  The reference's ``RandomSymmetry``
  raises there.

``RandomRotate`` and ``Center`` have no source on the reference's side (they are torch_geometric's, which is no
dependency here), so parity is UNPINNED and this is the contract.  ``RandomRotate(degrees, axis=0)``: a number ``d``
means the interval ``(-|d|, |d|)``; the angle is ``pi * random.uniform(*degrees) / 180`` with ``s, c = math.sin, math.cos``
of it; the float32 matrix ``A`` is ``[[1, 0, 0], [0, c, s], [0, -s, c]]`` for axis 0, ``[[c, 0, -s], [0, 1, 0], [s, 0, c]]``
for axis 1 and ``[[c, s, 0], [-s, c, 0], [0, 0, 1]]`` for axis 2; ``pos = pos @ A``; ``norm`` is left alone.
``Center()``: ``pos = pos - pos.mean(dim=-2, keepdim=True)``.

``fuse_cloud_augment(transforms)`` replaces every maximal run of positional classes by one ``FusedCloudAugment``: the
members' draws in the eager order, then ONE ``ops.cloud_augment`` per cloud, with the eager chain's results bit for bit.
"""
import math as _math
import numbers as _numbers
import random as _random

import numpy as _np
import torch as _torch

from .grid_transform import _has
from .multimodal.image import _get, _set

CLOUD_AUGMENT_ON_DEVICE = True

_MAX_STEPS = 16          # ops.CLOUD_MAX_STEPS


def _each(fn, data):
    if isinstance(data, list):
        return [fn(d) for d in data]
    return fn(data)


def _opt(data, key):
    """The attribute, or None when it is missing."""
    return _get(data, key) if _has(data, key) else None


def _delete(data, key):
    if isinstance(data, dict):
        del data[key]
    else:
        delattr(data, key)


def _is_iterable(entity):
    return isinstance(entity, (list, tuple)) or type(entity).__name__ == "ListConfig"


def _with_norm(data):
    return _opt(data, "norm") is not None


def _mm3(a, b):
    """``a @ b`` of two float32 3 x 3 host matrices, every product and sum rounded on its own, terms in ascending
    order: elementwise tensor operations, which no BLAS kernel reorders or fuses."""
    return (a[:, 0:1] * b[0:1, :] + a[:, 1:2] * b[1:2, :]) + a[:, 2:3] * b[2:3, :]


# ---------------------------------------------------------------------------------------------------------------
# one step list on one cloud: the device op, or the torch composition of the reference's lines
# ---------------------------------------------------------------------------------------------------------------
def _compose(pos, norm, steps):
    """The reference's lines, step by step (any device, any dtype)."""
    for step in steps:
        name = step[0]
        if name == "noise":
            pos = pos + step[1].to(pos.device)
        elif name == "linear":
            matrix, with_norm = step[1], step[2]
            pos = pos.float() @ matrix.to(pos.device).T
            if with_norm:
                norm = norm.float() @ matrix.to(norm.device).T
        elif name == "scale":
            scale = step[1]
            pos = pos * scale.to(pos.device)
            if norm is not None:
                norm = norm / scale.to(norm.device)
                norm = _torch.nn.functional.normalize(norm, dim=1)
        elif name == "flip":
            pos = pos.clone()
            for i, flagged in enumerate(step[1]):
                if flagged:
                    c_max = _torch.max(pos[:, i])
                    pos[:, i] = c_max - pos[:, i]
        else:
            pos = pos - pos.mean(dim=-2, keepdim=True)
    return pos, norm


def _on_device(pos, norm):
    if not (CLOUD_AUGMENT_ON_DEVICE and pos.is_cuda and pos.dtype == _torch.float32 and pos.dim() == 2
            and pos.shape[1] == 3):
        return False
    return norm is None or (norm.is_cuda and norm.dtype == _torch.float32 and norm.shape == pos.shape)


def _device_steps(pos, norm, steps):
    """One ``ops.cloud_augment`` call, or None where the kernel refuses the size (``3 N >= 2^31``)."""
    from ... import _lib, ops
    noises = [step[1] for step in steps if step[0] == "noise"]
    if len(noises) > 1:
        raise ValueError("one pass takes one noise tensor: fuse_cloud_augment splits a run in front of a second RandomNoise")
    noise = noises[0].to(pos.device) if noises else None
    out = _lib.unless_unsupported(ops.cloud_augment, pos, [s[:1] if s[0] == "noise" else s for s in steps], norm=norm,
                                  noise=noise)
    return None if out is None else out[:2]               # None: the composition takes over


def _run(data, steps):
    """Apply ``steps`` (the output of the members' ``draw``) to ``data.pos`` and, where a step touches it,
    ``data.norm``."""
    pos = _get(data, "pos")
    if not steps or pos.shape[0] == 0:
        return data                                   # the draws are made, nothing to launch
    norm_in = norm = _opt(data, "norm")
    out = _device_steps(pos, norm, steps) if _on_device(pos, norm) else None
    pos, norm = out if out is not None else _compose(pos, norm, steps)
    _set(data, "pos", pos)
    if norm is not norm_in:
        _set(data, "norm", norm)
    return data


class _Positional:
    """A transform of ``pos`` (and ``norm``) that is a list of ``ops.cloud_augment`` steps once its draws are made."""

    def draw(self, data):
        raise NotImplementedError

    def _process(self, data):
        return _run(data, self.draw(data))

    def __call__(self, data):
        return _each(self._process, data)


class RandomNoise(_Positional):
    """ Simple isotropic additive gaussian noise (Jitter)

    Parameters
    ----------
    sigma:
        Variance of the noise
    clip:
        Maximum amplitude of the noise
    """

    def __init__(self, sigma=0.01, clip=0.05):
        self.sigma = sigma
        self.clip = clip

    def draw(self, data):
        """``torch.randn(pos.shape)`` of the default CPU generator, scaled and clamped on the host."""
        noise = self.sigma * _torch.randn(_get(data, "pos").shape)
        noise = noise.clamp(-self.clip, self.clip)
        return [("noise", noise)]

    def __repr__(self):
        return "{}(sigma={}, clip={})".format(self.__class__.__name__, self.sigma, self.clip)


class RandomRotate(_Positional):
    """Rotates ``pos`` around ``axis`` by an angle drawn from ``degrees`` (a number ``d`` means ``(-|d|, |d|)``):
    ``pos @ A`` with the float32 matrix ``A`` of the module docstring (a ``pos`` of another dtype is converted to
    float32).  One ``random.uniform``.  ``norm`` is left alone."""

    def __init__(self, degrees, axis=0):
        if isinstance(degrees, _numbers.Number):
            degrees = (-abs(degrees), abs(degrees))
        assert isinstance(degrees, (tuple, list)) and len(degrees) == 2
        self.degrees = degrees
        self.axis = axis

    def matrix(self, degree):
        """The float32 matrix ``A`` of a rotation by ``degree`` degrees."""
        angle = _math.pi * degree / 180.0
        sin, cos = _math.sin(angle), _math.cos(angle)
        if self.axis == 0:
            matrix = [[1, 0, 0], [0, cos, sin], [0, -sin, cos]]
        elif self.axis == 1:
            matrix = [[cos, 0, -sin], [0, 1, 0], [sin, 0, cos]]
        else:
            matrix = [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]]
        return _torch.tensor(matrix, dtype=_torch.float32)

    def draw(self, data):
        return [("linear", self.matrix(_random.uniform(*self.degrees)).T, False)]

    def __repr__(self):
        return "{}({}, axis={})".format(self.__class__.__name__, self.degrees, self.axis)


class Random3AxisRotation(_Positional):
    """
    Rotate pointcloud with random angles along x, y, z axis

    The angles should be given `in degrees`.

    Parameters
    -----------
    apply_rotation: bool:
        Whether to apply the rotation
    rot_x: float
        Rotation angle in degrees on x axis
    rot_y: float
        Rotation anglei n degrees on y axis
    rot_z: float
        Rotation angle in degrees on z axis
    """

    def __init__(self, apply_rotation=True, rot_x=None, rot_y=None, rot_z=None):
        self._apply_rotation = apply_rotation
        if apply_rotation:
            if (rot_x is None) and (rot_y is None) and (rot_z is None):
                raise Exception("At least one rot_ should be defined")

        self._rot_x = _np.abs(rot_x) if rot_x else 0
        self._rot_y = _np.abs(rot_y) if rot_y else 0
        self._rot_z = _np.abs(rot_z) if rot_z else 0

        self._degree_angles = [self._rot_x, self._rot_y, self._rot_z]

    def generate_random_rotation_matrix(self):
        """One ``random.random()`` per axis whose angle is above 0, float32 thetas, then the host lines of the
        reference's ``euler_angles_to_rotation_matrix(thetas, random_order=True)`` (utils/geometry.py:5-22): float32
        ``cos`` / ``sin``, ``random.shuffle`` of the three axis matrices, and the two 3 x 3 products.  The reference
        takes those from ``torch.mm``, whose last bit depends on the BLAS kernel the host picks (fused multiply-add or
        not); here every entry is ``((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j)`` in separately rounded float32, which is
        ``torch.mm`` without fusion and the same matrix on every host (``_mm3``)."""
        thetas = _torch.zeros(3, dtype=_torch.float)
        for axis_ind, deg_angle in enumerate(self._degree_angles):
            if deg_angle > 0:
                rand_deg_angle = _random.random() * 2 * deg_angle - deg_angle
                rand_radian_angle = float(rand_deg_angle * _np.pi) / 180.0
                thetas[axis_ind] = rand_radian_angle
        cos = [float(_torch.cos(thetas[i])) for i in range(3)]
        sin = [float(_torch.sin(thetas[i])) for i in range(3)]
        r_x = _torch.tensor([[1, 0, 0], [0, cos[0], -sin[0]], [0, sin[0], cos[0]]], dtype=_torch.float32)
        r_y = _torch.tensor([[cos[1], 0, sin[1]], [0, 1, 0], [-sin[1], 0, cos[1]]], dtype=_torch.float32)
        r_z = _torch.tensor([[cos[2], -sin[2], 0], [sin[2], cos[2], 0], [0, 0, 1]], dtype=_torch.float32)
        matrices = [r_x, r_y, r_z]
        _random.shuffle(matrices)
        return _mm3(matrices[2], _mm3(matrices[1], matrices[0]))

    def draw(self, data):
        if not self._apply_rotation:
            return []
        return [("linear", self.generate_random_rotation_matrix(), _with_norm(data))]

    def __repr__(self):
        return "{}(apply_rotation={}, rot_x={}, rot_y={}, rot_z={})".format(
            self.__class__.__name__, self._apply_rotation, self._rot_x, self._rot_y, self._rot_z
        )


class RandomScaleAnisotropic(_Positional):
    r""" Scales node positions by a randomly sampled factor ``s1, s2, s3`` within a
    given interval, *e.g.*, resulting in the transformation matrix

    .. math::
        \left[
        \begin{array}{ccc}
            s1 & 0 & 0 \\
            0 & s2 & 0 \\
            0 & 0 & s3 \\
        \end{array}
        \right]


    for three-dimensional positions.  A ``norm`` attribute is divided by the factors and normalised.

    Parameters
    -----------
    scales:
        scaling factor interval, e.g. ``(a, b)``, then scale \
        is randomly sampled from the range \
        ``a <=  b``. \
    """

    def __init__(self, scales=None, anisotropic=True):
        assert _is_iterable(scales) and len(scales) == 2
        assert scales[0] <= scales[1]
        self.scales = scales

    def draw(self, data):
        scale = self.scales[0] + _torch.rand((3,)) * (self.scales[1] - self.scales[0])
        return [("scale", scale)]

    def __repr__(self):
        return "{}({})".format(self.__class__.__name__, self.scales)


class RandomSymmetry(_Positional):
    """ Apply a random symmetry transformation on the data

    Parameters
    ----------
    axis: Tuple[bool,bool,bool], optional
        axis along which the symmetry is applied

    One ``torch.rand(1) < 0.5`` per enabled axis; a drawn axis ``i`` becomes ``max(pos[:, i]) - pos[:, i]``.  The axes
    drawn in one call are one flip step.  ``pos`` is replaced, not written in place as the reference does.
    """

    def __init__(self, axis=[False, False, False]):
        self.axis = axis

    def draw(self, data):
        mask = [False, False, False]
        for i, ax in enumerate(self.axis):
            if ax:
                if _torch.rand(1) < 0.5:
                    mask[i] = True
        return [("flip", tuple(mask))] if any(mask) else []

    def __repr__(self):
        return "Random symmetry of axes: x={}, y={}, z={}".format(*self.axis)


class Center(_Positional):
    """Centers node positions around the origin: ``pos - pos.mean(dim=-2, keepdim=True)``.  No draws."""

    def draw(self, data):
        return [("center",)]

    def __repr__(self):
        return "{}()".format(self.__class__.__name__)


# ---------------------------------------------------------------------------------------------------------------
# the fuser
# ---------------------------------------------------------------------------------------------------------------
_POSITIONAL = (RandomNoise, RandomRotate, Random3AxisRotation, RandomScaleAnisotropic, RandomSymmetry, Center)


class FusedCloudAugment:
    """A run of positional augmentations as one pass: the members' ``draw()`` in the order the eager chain draws (member
    by member, and for a list of clouds every cloud within a member), then one ``ops.cloud_augment`` per cloud.  From the
    same generator states it gives the ``pos`` and ``norm`` of the eager chain of the same instances bit for bit, leaves
    the same generator states and passes every other attribute through untouched."""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, data):
        clouds = data if isinstance(data, list) else [data]
        steps = [[] for _ in clouds]
        for transform in self.transforms:
            for cloud, cloud_steps in zip(clouds, steps):
                cloud_steps.extend(transform.draw(cloud))
        out = [_run(cloud, cloud_steps) for cloud, cloud_steps in zip(clouds, steps)]
        return out if isinstance(data, list) else out[0]

    def __repr__(self):
        return "{}([{}])".format(self.__class__.__name__, ", ".join(repr(t) for t in self.transforms))


def fuse_cloud_augment(transforms):
    """A new list in which every maximal contiguous run of ``RandomNoise``, ``RandomRotate``, ``Random3AxisRotation``,
    ``RandomScaleAnisotropic``, ``RandomSymmetry`` and ``Center`` instances is replaced by one ``FusedCloudAugment``
    holding them.  Any other transform ends a run and stays as it is, in place (``XYZFeature`` reads ``pos``, so the
    S3DIS chain gives ``[noise, rotate, scale, symmetry]`` and ``[Center]``).  A member is at most one step, the op takes
    16 steps and one noise tensor: a run is split after 16 members and in front of a second ``RandomNoise``."""
    out, run = [], []

    def close():
        if run:
            out.append(FusedCloudAugment(run))
            run.clear()

    for transform in list(transforms):
        if type(transform) in _POSITIONAL:
            if len(run) == _MAX_STEPS or (type(transform) is RandomNoise and any(type(t) is RandomNoise for t in run)):
                close()
            run.append(transform)
        else:
            close()
            out.append(transform)
    close()
    return out


# ---------------------------------------------------------------------------------------------------------------
# host classes in plain torch: device-agnostic
# ---------------------------------------------------------------------------------------------------------------
class ShiftVoxels:
    """ Trick to make Sparse conv invariant to even and odds coordinates
    https://github.com/chrischoy/SpatioTemporalSegmentation/blob/master/lib/train.py#L78

    Parameters
    -----------
    apply_shift: bool:
        Whether to apply the shift on indices

    ``coords`` is int32 on any device (the reference takes a CPU ``torch.IntTensor`` alone); the shift is
    ``torch.rand(3) * 100`` truncated to int32 on the host.  ``coords`` is replaced, not written in place.
    """

    def __init__(self, apply_shift=True):
        self._apply_shift = apply_shift

    def _process(self, data):
        if self._apply_shift:
            if not _has(data, "coords"):
                raise Exception("should quantize first using GridSampling3D")
            coords = _get(data, "coords")
            if not _torch.is_tensor(coords) or coords.dtype != _torch.int32:
                raise Exception("The pos are expected to be coordinates, so torch.IntTensor")
            shift = (_torch.rand(3) * 100).to(_torch.int32)
            coords = coords.clone()
            coords[:, :3] += shift.to(coords.device)
            _set(data, "coords", coords)
        return data

    def __call__(self, data):
        return _each(self._process, data)

    def __repr__(self):
        return "{}(apply_shift={})".format(self.__class__.__name__, self._apply_shift)


class XYZFeature:
    """
    Add the X, Y and Z as a feature
    Parameters
    -----------
    add_x: bool [default: False]
        whether we add the x position or not
    add_y: bool [default: False]
        whether we add the y position or not
    add_z: bool [default: True]
        whether we add the z position or not
    """

    def __init__(self, add_x=False, add_y=False, add_z=True):
        self._axis = []
        axis_names = ["x", "y", "z"]
        if add_x:
            self._axis.append(0)
        if add_y:
            self._axis.append(1)
        if add_z:
            self._axis.append(2)

        self._axis_names = [axis_names[idx_axis] for idx_axis in self._axis]

    def _process(self, data):
        pos = _opt(data, "pos")
        assert pos is not None
        for axis_name, id_axis in zip(self._axis_names, self._axis):
            _set(data, "pos_{}".format(axis_name), pos[:, id_axis].clone())
        return data

    def __call__(self, data):
        return _each(self._process, data)

    def __repr__(self):
        return "{}(axis={})".format(self.__class__.__name__, self._axis_names)


class AddFeatByKey:
    """This transform is responsible to get an attribute under feat_name and add it to x if add_to_x is True

    Parameters
    ----------
    add_to_x: bool
        Control if the feature is going to be added/concatenated to x
    feat_name: str
        The feature to be found within data to be added/concatenated to x
    input_nc_feat: int, optional
        If provided, check if feature last dimension maches provided value.
    strict: bool, optional
        Recommended to be set to True. If False, it won't break if feat isn't found or dimension doesn t match. (default: ``True``)
    """

    def __init__(self, add_to_x, feat_name, input_nc_feat=None, strict=True):
        self._add_to_x = add_to_x
        self._feat_name = feat_name
        self._input_nc_feat = input_nc_feat
        self._strict = strict

    def _process(self, data):
        if not self._add_to_x:
            return data
        feat = _opt(data, self._feat_name)
        if feat is None:
            if self._strict:
                raise Exception("Data should contain the attribute {}".format(self._feat_name))
            return data
        if self._input_nc_feat:
            feat_dim = 1 if feat.dim() == 1 else feat.shape[-1]
            if self._input_nc_feat != feat_dim and self._strict:
                raise Exception("The shape of feat: {} doesn t match {}".format(feat.shape, self._input_nc_feat))
        x = _opt(data, "x")
        if x is None:
            if self._strict and _get(data, "pos").shape[0] != feat.shape[0]:
                raise Exception("We expected to have an attribute x")
            if feat.dim() == 1:
                feat = feat.unsqueeze(-1)
            _set(data, "x", feat)
        elif x.shape[0] == feat.shape[0]:
            if x.dim() == 1:
                x = x.unsqueeze(-1)
            if feat.dim() == 1:
                feat = feat.unsqueeze(-1)
            _set(data, "x", _torch.cat([x, feat], dim=-1))
        else:
            raise Exception(
                "The tensor x and {} can't be concatenated, x: {}, feat: {}".format(
                    self._feat_name, x.shape[0], feat.shape[0]
                )
            )
        return data

    def __call__(self, data):
        return _each(self._process, data)

    def __repr__(self):
        return "{}(add_to_x: {}, feat_name: {}, strict: {})".format(
            self.__class__.__name__, self._add_to_x, self._feat_name, self._strict
        )


class AddFeatsByKeys:
    """This transform takes a list of attributes names and if allowed, add them to x

    Example:

        Before calling "AddFeatsByKeys", if data.x was empty

        - transform: AddFeatsByKeys
          params:
              list_add_to_x: [False, True, True]
              feat_names: ['normal', 'rgb', "elevation"]
              input_nc_feats: [3, 3, 1]

        After calling "AddFeatsByKeys", data.x contains "rgb" and "elevation". Its shape[-1] == 4 (rgb:3 + elevation:1)
        If input_nc_feats was [4, 4, 1], it would raise an exception as rgb dimension is only 3.

    Paremeters
    ----------
    list_add_to_x: List[bool]
        For each boolean within list_add_to_x, control if the associated feature is going to be concatenated to x
    feat_names: List[str]
        The list of features within data to be added to x
    input_nc_feats: List[int], optional
        If provided, evaluate the dimension of the associated feature shape[-1] found using feat_names and this provided value. It allows to make sure feature dimension didn't change
    stricts: List[bool], optional
        Recommended to be set to list of True. If True, it will raise an Exception if feat isn't found or dimension doesn t match.
    delete_feats: List[bool], optional
        Whether we want to delete the feature from the data object. List length must match teh number of features added.
    """

    def __init__(self, list_add_to_x, feat_names, input_nc_feats=None, stricts=None, delete_feats=None):
        self._feat_names = feat_names
        self._list_add_to_x = list_add_to_x
        self._delete_feats = delete_feats
        if self._delete_feats:
            assert len(self._delete_feats) == len(self._feat_names)

        num_names = len(feat_names)
        if num_names == 0:
            raise Exception("Expected to have at least one feat_names")

        assert len(list_add_to_x) == num_names

        if input_nc_feats:
            assert len(input_nc_feats) == num_names
        else:
            input_nc_feats = [None for _ in range(num_names)]

        if stricts:
            assert len(stricts) == num_names
        else:
            stricts = [True for _ in range(num_names)]

        self.transforms = [
            AddFeatByKey(add_to_x, feat_name, input_nc_feat=input_nc_feat, strict=strict)
            for add_to_x, feat_name, input_nc_feat, strict in zip(list_add_to_x, feat_names, input_nc_feats, stricts)
        ]

    def _process(self, data):
        for transform in self.transforms:
            data = transform(data)
        if self._delete_feats:
            for feat_name, delete_feat in zip(self._feat_names, self._delete_feats):
                if delete_feat:
                    _delete(data, feat_name)
        return data

    def __call__(self, data):
        return _each(self._process, data)

    def __repr__(self):
        msg = ""
        for f, a in zip(self._feat_names, self._list_add_to_x):
            msg += "{}={}, ".format(f, a)
        return "{}({})".format(self.__class__.__name__, msg[:-2])
