"""Multimodal samples and their batch (reference: torch_points3d/core/multimodal/data.py:13-225).

``MMData`` holds the 3D points of a sample and, per modality, the data with its mappings to those points; ``MMBatch``
is what the collate function of every multimodal dataset returns (datasets/base_dataset_multimodal.py:46-68) and
what ``modules.multimodal.modules.multimodal_input`` takes.  Same surface as the reference: the keys of the 3D data
mirrored as attributes, ``modalities``, ``num_points``, ``to``, ``device``, ``clone``, point indexing, and the
``from_mm_data_list`` / ``to_mm_data_list`` round trip.  File loading (``load``) is outside this package, as it is for
the image holders.

The 3D data is whatever the transforms of this package accept: a torch_geometric ``Data`` when that package can be
imported, a ``dict`` or a ``types.SimpleNamespace``.  A list of ``Data`` is batched by torch_geometric's
``Batch.from_data_list``; dicts and namespaces by ``collate_data`` below, which states the same rule.  The mappings
are batched by ``ImageBatch.from_data_list``: for samples on a HIP device that is one ``ops.collate_mapping`` per
image setting, and neither it nor ``collate_data`` synchronises with the host.
"""
import copy
from types import SimpleNamespace

import numpy as np
import torch

from ...utils.multimodal import MAPPING_KEY, tensor_idx
from ..data_transform.grid_transform import _keys
from ..data_transform.multimodal.image import _get, _num_nodes, _set
from .image import ImageData

# Supported modalities
MODALITY_FORMATS = {"image": ImageData}
MODALITY_NAMES = list(MODALITY_FORMATS.keys())

_SLICES_KEY = '__slices__'      # bookkeeping of collate_data: key -> how each sample's value went into the batch


def _geometric():
    """(Data, Batch) of torch_geometric, or (None, None) when it cannot be imported."""
    try:
        from torch_geometric.data import Batch, Data
    except ImportError:
        return None, None
    return Data, Batch


def _data_keys(data):
    return [k for k in _keys(data) if not k.startswith('_')]


def _is_data(data):
    Data, _ = _geometric()
    return isinstance(data, (dict, SimpleNamespace)) or (Data is not None and isinstance(data, Data))


def _clone_data(data):
    """New container, cloned tensors (``Data.clone``)."""
    if not isinstance(data, (dict, SimpleNamespace)):
        return data.clone()
    items = vars(data) if isinstance(data, SimpleNamespace) else data
    out = {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in items.items()}
    return out if isinstance(data, dict) else SimpleNamespace(**out)


def _data_to(data, device):
    if not isinstance(data, (dict, SimpleNamespace)):
        return data.to(device)
    items = vars(data) if isinstance(data, SimpleNamespace) else data
    out = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in items.items()}
    return out if isinstance(data, dict) else SimpleNamespace(**out)


def collate_data(data_list):
    """Batch of a list of dicts or namespaces with the same keys, by the rule of torch_geometric's
    ``Batch.from_data_list`` for point clouds:

    - tensors are concatenated along dim 0 (0-dim tensors are stacked);
    - a tensor whose key contains ``index`` is first offset by the number of nodes of the samples in front of it, which
      is how ``mapping_index`` stays a valid point index of the batch;
    - an int64 ``batch`` vector, the sample of every node, is added;
    - numbers are stacked into a tensor (int64, or float64 so that ``uncollate_data`` returns a Python float as it
      came), except ``num_nodes``, which is summed;
    - every other value is kept as the list of the samples' values.

    The result has the type of the first sample.  Nothing here synchronises with the host: every size is a shape,
    and ``batch`` is a concatenation of constant vectors.  ``uncollate_data`` undoes it."""
    assert isinstance(data_list, list) and len(data_list) > 0
    first = data_list[0]
    assert all(isinstance(d, (dict, SimpleNamespace)) for d in data_list), \
        "collate_data takes dicts or SimpleNamespaces; torch_geometric Data goes through Batch.from_data_list."
    keys = _data_keys(first)
    assert all(set(_data_keys(d)) == set(keys) for d in data_list), "All samples must have the same keys."
    assert 'batch' not in keys, "The samples of a batch must not carry a 'batch' attribute of their own."
    sizes = [_num_nodes(d) for d in data_list]
    starts = [0]
    for n in sizes[:-1]:
        starts.append(starts[-1] + n)
    out, slices = {}, {}
    for key in keys:
        vals = [_get(d, key) for d in data_list]
        if key == 'num_nodes':
            out[key] = sum(sizes)
        elif all(torch.is_tensor(v) for v in vals):
            if any(v.dim() == 0 for v in vals):
                out[key], slices[key] = torch.stack(vals), None
                continue
            if 'index' in key:
                vals = [v + s for v, s in zip(vals, starts)]
            out[key], slices[key] = torch.cat(vals, dim=0), [v.shape[0] for v in vals]
        elif all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in vals):
            out[key] = torch.tensor(vals, dtype=torch.long if all(isinstance(v, int) for v in vals) else torch.float64)
        else:
            out[key] = vals
    device = _get(first, 'pos').device if 'pos' in keys else _get(first, MAPPING_KEY).device
    out['batch'] = torch.cat([torch.full((n,), i, dtype=torch.long, device=device) for i, n in enumerate(sizes)])
    out[_SLICES_KEY] = slices
    return out if isinstance(first, dict) else SimpleNamespace(**out)


def uncollate_data(batch, sizes):
    """The samples ``collate_data`` batched (``sizes``: their numbers of nodes), in the type of ``batch``."""
    is_dict = isinstance(batch, dict)
    slices = (batch.get(_SLICES_KEY) if is_dict else getattr(batch, _SLICES_KEY, None))
    if slices is None:
        raise RuntimeError('Cannot reconstruct the data list: the batch was not created using `collate_data()`.')
    sizes = [int(n) for n in sizes]
    starts = [0]
    for n in sizes[:-1]:
        starts.append(starts[-1] + n)
    samples = [{} for _ in sizes]
    for key in _data_keys(batch):
        val = _get(batch, key)
        if key == 'batch':
            continue
        if key == 'num_nodes':
            parts = sizes
        elif key in slices and slices[key] is not None:
            parts = list(torch.split(val, slices[key], dim=0))
            if 'index' in key:
                parts = [p - s for p, s in zip(parts, starts)]
        elif torch.is_tensor(val):
            parts = [v if key in slices else v.item() for v in val]
        else:
            parts = val
        for sample, part in zip(samples, parts):
            sample[key] = part
    return samples if is_dict else [SimpleNamespace(**s) for s in samples]


class MMData(object):
    """A holder for multimodal data: the 3D points of a sample in ``data`` and, as keyword arguments named after the
    supported modalities (``MODALITY_NAMES``), modality-specific data equipped with mappings to those points
    (reference data.py:13-141)."""

    def __init__(self, data, **kwargs):
        self.data = data
        self.modalities = kwargs
        self.mapping_key = MAPPING_KEY
        assert _is_data(data), f"Expected a Data, a dict or a SimpleNamespace but got {type(data)} instead."
        for k in _data_keys(self.data):
            setattr(self, k, _get(self.data, k))
        self.debug()

    def debug(self):
        """The reference's checks (data.py:35-70).  The check on the VALUES of the mapping key -- its distinct values
        are ``0 .. num_points - 1`` -- reads the tensor, so it runs for CPU tensors only: constructing an ``MMData``
        from data on the device does not synchronise with the host.  Sizes and types are checked everywhere."""
        assert _is_data(self.data), f"Expected a Data, a dict or a SimpleNamespace but got {type(self.data)} instead."
        # each point must have a mapping, even if empty; the same point may be used multiple times
        assert self.mapping_key in _data_keys(self.data)
        assert 'index' in self.mapping_key, \
            f"Key {self.mapping_key} must contain 'index' to benefit from Batch mechanisms."
        mapping_index = _get(self.data, self.mapping_key)
        assert mapping_index.dim() == 1 and mapping_index.shape[0] == self.num_points, \
            f"Data {self.mapping_key} has shape {tuple(mapping_index.shape)}, with {self.num_points} points in total."
        if not mapping_index.is_cuda and mapping_index.shape[0] > 0:
            idx = torch.unique(mapping_index)
            assert idx.max() + 1 == idx.shape[0] == self.num_points, \
                f"Discrepancy between the Data point indices and the mappings indices. Data {self.mapping_key} " \
                f"counts {idx.shape[0]} unique values with max={idx.max()}, with {self.num_points} points in total."
        for mod, data_mod in self.modalities.items():
            assert mod in MODALITY_NAMES, \
                f"Received kwarg={mod} but expected key to belong to supported modalities: {MODALITY_NAMES}."
            assert isinstance(data_mod, MODALITY_FORMATS[mod]), \
                f"Expected modality '{mod}' data to be of type {MODALITY_FORMATS[mod]} but got type " \
                f"{type(data_mod)} instead."
            assert self.num_points == data_mod.num_points or data_mod.num_points == 0, \
                f"Discrepancy between the Data point indices and the '{mod}' modality mappings. Data " \
                f"'{self.mapping_key}' counts {self.num_points} points in total, while '{mod}' mappings cover point " \
                f"indices in [0, {data_mod.num_points}]."

    def __len__(self):
        return _num_nodes(self.data)

    @property
    def num_points(self):
        return len(self)

    @property
    def num_node_features(self):
        x = _get(self.data, 'x') if 'x' in _data_keys(self.data) else None
        return 0 if x is None else (1 if x.dim() == 1 else x.shape[1])

    def _like(self, data, modalities):
        """An object of this class around other data."""
        return self.__class__(data, **modalities)

    def to(self, device):
        return self._like(_data_to(self.data, device), {mod: data_mod.to(device)
                                                        for mod, data_mod in self.modalities.items()})

    @property
    def device(self):
        for data_mod in self.modalities.values():
            return data_mod.device
        return _get(self.data, self.mapping_key).device

    def clone(self):
        return self._like(_clone_data(self.data), {mod: data_mod.clone() for mod, data_mod in self.modalities.items()})

    def __getitem__(self, idx):
        """Indexing mechanism on the points: a new ``MMData`` of the indexed points, with updated modality data and
        mappings (reference data.py:106-133).  Supports torch and numpy indexing."""
        idx = tensor_idx(idx).to(self.device)
        data = _clone_data(self.data)
        n = self.num_points
        for key in _data_keys(self.data):
            item = _get(self.data, key)
            if torch.is_tensor(item) and item.dim() > 0 and item.size(0) == n:
                _set(data, key, _get(data, key)[idx.to(item.device)])
        if 'num_nodes' in _data_keys(data):
            _set(data, 'num_nodes', int(idx.shape[0]))
        # update the modality data and mappings with respect to the data key indices
        modalities = {mod: data_mod.select_points(_get(data, self.mapping_key), mode='pick')
                      for mod, data_mod in self.modalities.items()}
        # the point indices follow the new mappings: this is what the batching mechanisms rely on
        _set(data, self.mapping_key, torch.arange(_num_nodes(data), device=self.device))
        return MMData(data, **modalities)

    def __repr__(self):
        info = [f"    data = {self.data}"] + [f"    {mod} = {data_mod}" for mod, data_mod in self.modalities.items()]
        info = '\n'.join(info)
        return f"{self.__class__.__name__}(\n{info}\n)"


class MMBatch(MMData):
    """A batch of ``MMData``, built with the batch mechanism of every modality (reference data.py:144-225)."""

    def __init__(self, data, **kwargs):
        super(MMBatch, self).__init__(data, **kwargs)
        self.__sizes__ = None

    @property
    def batch_pointers(self):
        return np.cumsum(np.concatenate(([0], self.__sizes__))) if self.__sizes__ is not None else None

    @property
    def batch_items_sizes(self):
        return self.__sizes__ if self.__sizes__ is not None else None

    @property
    def num_batch_items(self):
        return len(self.__sizes__) if self.__sizes__ is not None else None

    def _like(self, data, modalities):
        out = MMBatch(data, **modalities)
        out.__sizes__ = self.__sizes__
        return out

    @staticmethod
    def from_mm_data_list(mm_data_list):
        assert isinstance(mm_data_list, list) and len(mm_data_list) > 0
        assert all(isinstance(mm_data, MMData) for mm_data in mm_data_list)
        assert all(set(mm_data.modalities.keys()) == set(mm_data_list[0].modalities.keys())
                   for mm_data in mm_data_list), "All MMData in the list must have the same modalities."
        # the 3D data
        data_list = [mm_data.data for mm_data in mm_data_list]
        Data, Batch = _geometric()
        if Data is not None and all(isinstance(d, Data) for d in data_list):
            data = Batch.from_data_list(data_list)
        else:
            data = collate_data(data_list)
        # the modality-specific data, by their own batch type
        modalities = {mod: data_mod.get_batch_type().from_data_list([mm_data.modalities[mod] for mm_data in mm_data_list])
                      for mod, data_mod in mm_data_list[0].modalities.items()}
        # __sizes__ allows to_mm_data_list() to recover the input list
        batch = MMBatch(data, **modalities)
        batch.__sizes__ = np.array([len(mm_data) for mm_data in mm_data_list])
        return batch

    def to_mm_data_list(self):
        if self.__sizes__ is None:
            raise RuntimeError('Cannot reconstruct multimodal data list from batch because the batch object was not '
                               'created using `MMBatch.from_mm_data_list()`.')
        if isinstance(self.data, (dict, SimpleNamespace)):
            data_list = uncollate_data(self.data, self.__sizes__)
        else:
            data_list = self.data.to_data_list()
        mods_dict_list = {mod: data_mod.to_data_list() for mod, data_mod in self.modalities.items()}
        mods_list_dict = [{mod: data_mod[i] for mod, data_mod in mods_dict_list.items()}
                          for i in range(self.num_batch_items)]
        return [MMData(data, **modalities) for data, modalities in zip(data_list, mods_list_dict)]
