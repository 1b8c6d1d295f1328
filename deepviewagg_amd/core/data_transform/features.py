"""PCAComputePointwise and EigenFeatures: the per-point geometric attributes the mapping build reads.

Mirror of the two pre-transforms every multimodal data config runs before MapImages (reference:
torch_points3d/core/data_transform/features.py:360-485 and :488-587).  ``PCAComputePointwise`` finds the
``num_neighbors`` nearest neighbours of every point with the exact HIP grid search (``ops.knn_query``; the reference's
KeOps branch is exact too, its FAISS IVF branch is approximate) and computes the PCA of every neighbourhood on the
device (``ops.pointwise_pca``, the reference's ``batch_pca`` per chunk on the CPU).  ``EigenFeatures`` turns the
eigenvalues into ``linearity``, ``planarity`` and ``scattering`` and the first eigenvector into ``norm``: a few
elementwise passes over [n, 3], plain torch.

``dropin.install()`` copies every public name of this module onto the reference's module, so the public namespace
is the two classes: everything else is imported under ``_`` names.
"""
import torch as _torch


def _apply(transform, data):
    if isinstance(data, list):
        return [transform._process(d) for d in data]
    return transform._process(data)


def _repr(obj):
    return f"{obj.__class__.__name__}({', '.join(f'{k}={v}' for k, v in obj.__dict__.items())})"


class PCAComputePointwise:
    """PCA of the ``num_neighbors``-nearest-neighbourhood of every point of ``data.pos``.  The neighbours are searched
    in ``data.full_pos`` when ``use_full_pos`` is set (see the reference's GridSampling3D), else in ``data.pos``.
    Writes ``data.eigenvalues`` [n, 3] (ascending, >= 0) and ``data.eigenvectors`` [n, 9] (three unit rows
    [v0 | v1 | v2]: ``[:, :3]`` is the normal) on the input's device.  The work runs on the current HIP device.

    Same constructor as the reference.  ``use_cuda``, ``use_faiss``, ``ncells``, ``nprobes`` and ``chunk_size`` are
    accepted and ignored: the search is exact and the PCA needs no chunking.  Radius neighbourhoods (``r``) are not
    implemented and raise."""

    def __init__(self, num_neighbors=40, r=None, use_full_pos=False, use_cuda=False, use_faiss=True, ncells=None,
                 nprobes=10, chunk_size=1000000):
        if r is not None:
            raise ValueError(
                f"PCAComputePointwise(r={r}): radius neighbourhoods (the reference's torch_points_kernels radius search) "
                f"are not implemented; use r=None for the exact K-NN of num_neighbors points")
        self.num_neighbors = num_neighbors
        self.r = r
        self.use_full_pos = use_full_pos
        self.use_cuda = use_cuda and _torch.cuda.is_available()
        self.use_faiss = use_faiss and _torch.cuda.is_available()
        self.ncells = ncells
        self.nprobes = nprobes
        self.chunk_size = chunk_size

    def _process(self, data):
        from ... import ops as _ops
        assert getattr(data, 'pos', None) is not None, "Data must contain a 'pos' attribute."
        assert not self.use_full_pos or getattr(data, 'full_pos', None) is not None, \
            "Data must contain a 'full_pos' attribute."
        query = data.pos
        search = data.full_pos if self.use_full_pos else data.pos
        device = _torch.device('cuda', _torch.cuda.current_device())
        search_dev = search.float().to(device)
        neighbors, _ = _ops.knn_query(query.float().to(device), search_dev, self.num_neighbors)
        eigenvalues, eigenvectors = _ops.pointwise_pca(search_dev, neighbors)
        dtype = query.dtype if query.is_floating_point() else _torch.float32
        data.eigenvalues = eigenvalues.to(device=query.device, dtype=dtype)
        data.eigenvectors = eigenvectors.to(device=query.device, dtype=dtype)
        return data

    def __call__(self, data):
        return _apply(self, data)

    def __repr__(self):
        return _repr(self)


class EigenFeatures:
    """Local geometric features from ``data.eigenvalues`` (l0 <= l1 <= l2) and ``data.eigenvectors``
    (see PCAComputePointwise), after [Yang et al. 2015] on the square roots v_i = sqrt(l_i), v2 shifted by 1e-6:
    ``norm`` = the first eigenvector, ``linearity`` = (v2 - v1) / v2, ``planarity`` = (v1 - v0) / v2,
    ``scattering`` = v0 / v2.  With ``temperature`` set, the three features go through a softmax of
    ``temperature`` x feature.  Same constructor and expressions as the reference."""

    def __init__(self, norm=True, linearity=True, planarity=True, scattering=True, temperature=None):
        self.norm = norm
        self.linearity = linearity
        self.planarity = planarity
        self.scattering = scattering
        self.temperature = temperature

    def _process(self, data):
        assert getattr(data, 'eigenvalues', None) is not None, "Data must contain an 'eigenvalues' attribute."
        assert getattr(data, 'eigenvectors', None) is not None, "Data must contain an 'eigenvectors' attribute."
        if self.norm:
            data.norm = data.eigenvectors[:, :3]
        root = data.eigenvalues.sqrt()
        v0, v1 = root[:, 0], root[:, 1]
        v2 = root[:, 2] + 1e-6
        feats = [(v2 - v1) / v2, (v1 - v0) / v2, v0 / v2]
        if self.temperature:
            e = (self.temperature * _torch.stack(feats, dim=1)).exp()
            e = e / e.sum(dim=1).view(-1, 1)
            feats = [e[:, 0], e[:, 1], e[:, 2]]
        for name, value in zip(('linearity', 'planarity', 'scattering'), feats):
            if getattr(self, name):
                setattr(data, name, value)
        return data

    def __call__(self, data):
        return _apply(self, data)

    def __repr__(self):
        return _repr(self)


# The classes of the reference's module that augment.py provides: kept out of the eagerly listed names above and served
# by name, as grid_transform.py serves ElasticDistortion.
_LAZY = ("Random3AxisRotation", "XYZFeature", "AddFeatsByKeys", "AddFeatByKey")


def __getattr__(name):
    if name in _LAZY:
        from . import augment as _augment
        return getattr(_augment, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
